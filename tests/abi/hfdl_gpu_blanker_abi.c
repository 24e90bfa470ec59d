/* The impulse-noise blanker of include/hfdl_gpu.h and the setter include/hfdl_host.h adds for it, pinned as tests/abi/hfdl_host_abi.c
 * pins the rest: the record's size and offsets (the Python mirror rests on them) and the four prototypes by type.  Not in the reference.
 * Compiled by tests/test_blanker_cpu.py; syntax check only, nothing runs. */
#include <stddef.h>
#include <stdint.h>
#include "hfdl_host.h"
#include "hfdl_gpu.h"

_Static_assert(sizeof(hfdl_gpu_blanker_stats) == 24, "hfdl_gpu_blanker_stats is 24 bytes");
_Static_assert(offsetof(hfdl_gpu_blanker_stats, blocks) == 0 && offsetof(hfdl_gpu_blanker_stats, samples_blanked) == 8
		&& offsetof(hfdl_gpu_blanker_stats, last_power) == 16 && offsetof(hfdl_gpu_blanker_stats, last_threshold) == 20, "the fields");

static int (*const pinned_enable)(hfdl_gpu_frontend *, float) = hfdl_gpu_frontend_blanker_enable;
static int (*const pinned_stats)(hfdl_gpu_frontend *, int32_t, hfdl_gpu_blanker_stats *) = hfdl_gpu_frontend_blanker_stats;
static int (*const pinned_block)(int, const void *, int32_t, int, float, float *, float *, uint64_t *) = hfdl_gpu_blank_block;
static int (*const pinned_set)(float) = hfdl_frontend_set_blanker;
int hfdl_gpu_blanker_abi_unused(void) { return pinned_enable == 0 || pinned_stats == 0 || pinned_block == 0 || pinned_set == 0; }
