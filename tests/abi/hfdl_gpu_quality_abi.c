/* The frame quality records of include/hfdl_gpu.h and the prototype include/hfdl_host.h adds for the frame log, pinned as
 * tests/abi/hfdl_host_abi.c pins the rest: the record's size and every field's offset (a caller's array of records, the Python mirror
 * and the device's stores all rest on them), the constants, and the four prototypes by type.  Not in the reference.  Compiled by
 * tests/test_quality_cpu.py; syntax check only, nothing runs. */
#include <stddef.h>
#include <stdint.h>
#include "hfdl_host.h"
#include "hfdl_gpu.h"

_Static_assert(sizeof(hfdl_gpu_frame_quality) == 744, "hfdl_gpu_frame_quality is 744 bytes");
_Static_assert(offsetof(hfdl_gpu_frame_quality, sample_index) == 0 && offsetof(hfdl_gpu_frame_quality, channel) == 8
		&& offsetof(hfdl_gpu_frame_quality, freq) == 12 && offsetof(hfdl_gpu_frame_quality, mode) == 16
		&& offsetof(hfdl_gpu_frame_quality, bitmask_lsb) == 20 && offsetof(hfdl_gpu_frame_quality, nsym) == 24
		&& offsetof(hfdl_gpu_frame_quality, segments) == 28 && offsetof(hfdl_gpu_frame_quality, train_bits_bad) == 32
		&& offsetof(hfdl_gpu_frame_quality, train_bits_total) == 36, "the integer fields");
_Static_assert(offsetof(hfdl_gpu_frame_quality, freq_err_hz) == 40 && offsetof(hfdl_gpu_frame_quality, rssi_db) == 44
		&& offsetof(hfdl_gpu_frame_quality, noise_floor_db) == 48 && offsetof(hfdl_gpu_frame_quality, sym_power) == 52
		&& offsetof(hfdl_gpu_frame_quality, err_power) == 56 && offsetof(hfdl_gpu_frame_quality, err_max) == 60
		&& offsetof(hfdl_gpu_frame_quality, gain_re) == 64 && offsetof(hfdl_gpu_frame_quality, gain_im) == 68
		&& offsetof(hfdl_gpu_frame_quality, seg_err_power) == 72, "the float fields");
_Static_assert(sizeof(((hfdl_gpu_frame_quality *)0)->seg_err_power) == 4 * HFDL_GPU_QUALITY_SEGMENTS_MAX, "one float per data segment");
_Static_assert(HFDL_GPU_QUALITY_SYMBOLS == 1u && HFDL_GPU_QUALITY_SEGMENTS_MAX == 168 && HFDL_GPU_QUALITY_SYMBOLS_MAX == 5040
		&& HFDL_GPU_QUALITY_SYMBOLS_MAX == 30 * HFDL_GPU_QUALITY_SEGMENTS_MAX && HFDL_GPU_QUALITY_RING_MAX == 65536, "the constants");

static int (*const pinned_enable)(hfdl_gpu_frontend *, int32_t, uint32_t) = hfdl_gpu_frontend_quality_enable;
static int (*const pinned_read)(hfdl_gpu_frontend *, hfdl_gpu_frame_quality *, float *, int32_t, int32_t *, uint32_t *, int) = hfdl_gpu_frontend_quality_read;
static int (*const pinned_batch)(int, const float *, const int32_t *, int32_t, hfdl_gpu_frame_quality *) = hfdl_gpu_frame_quality_batch;
static int (*const pinned_log)(const char *) = hfdl_frontend_set_frame_log;
int hfdl_gpu_quality_abi_unused(void) { return pinned_enable == 0 || pinned_read == 0 || pinned_batch == 0 || pinned_log == 0; }
