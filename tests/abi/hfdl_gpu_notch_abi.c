/* The adaptive carrier canceller of include/hfdl_gpu.h and the setter include/hfdl_host.h adds for it, pinned as
 * tests/abi/hfdl_host_abi.c pins the rest: the record's size and offsets (the Python mirror rests on them), the state's size, the tap's
 * number and the four prototypes by type.  Not in the reference.  Compiled by tests/test_notch_cpu.py; syntax check only, nothing runs. */
#include <stddef.h>
#include <stdint.h>
#include "hfdl_host.h"
#include "hfdl_gpu.h"

_Static_assert(sizeof(hfdl_gpu_notch_stats) == 32, "hfdl_gpu_notch_stats is 32 bytes");
_Static_assert(offsetof(hfdl_gpu_notch_stats, blocks) == 0 && offsetof(hfdl_gpu_notch_stats, resets) == 8
		&& offsetof(hfdl_gpu_notch_stats, last_in_power) == 16 && offsetof(hfdl_gpu_notch_stats, last_out_power) == 20
		&& offsetof(hfdl_gpu_notch_stats, tap_energy) == 24, "the fields");
_Static_assert(HFDL_GPU_NOTCH_STATE_FLOATS == 2 * 32 + 2 * (24 + 32 - 1), "32 taps and the last D + L - 1 inputs, as (re, im)");
_Static_assert(HFDL_GPU_TAP_NOTCH_OUT == 10, "the tap's number");

static int (*const pinned_enable)(hfdl_gpu_frontend *, const int32_t *, int32_t, float) = hfdl_gpu_frontend_notch_enable;
static int (*const pinned_stats)(hfdl_gpu_frontend *, int32_t, hfdl_gpu_notch_stats *) = hfdl_gpu_frontend_notch_stats;
static int (*const pinned_rows)(int, const float *, int32_t, int32_t, float, float *, float *) = hfdl_gpu_notch_rows;
static int (*const pinned_set)(float, const int32_t *, int) = hfdl_frontend_set_notch;
int hfdl_gpu_notch_abi_unused(void) { return pinned_enable == 0 || pinned_stats == 0 || pinned_rows == 0 || pinned_set == 0; }
