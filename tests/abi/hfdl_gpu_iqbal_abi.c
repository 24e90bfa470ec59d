/* The I/Q imbalance and DC corrector of include/hfdl_gpu.h and the setter include/hfdl_host.h adds for it, pinned as
 * tests/abi/hfdl_gpu_blanker_abi.c pins the blanker: the record's size and offsets (the Python mirror rests on them) and the five
 * prototypes by type.  Not in the reference.  Compiled by tests/test_iqbal_cpu.py; syntax check only, nothing runs. */
#include <stddef.h>
#include <stdint.h>
#include "hfdl_host.h"
#include "hfdl_gpu.h"

_Static_assert(sizeof(hfdl_gpu_iqbal_stats) == 48, "hfdl_gpu_iqbal_stats is 48 bytes");
_Static_assert(offsetof(hfdl_gpu_iqbal_stats, blocks) == 0 && offsetof(hfdl_gpu_iqbal_stats, refused) == 8
		&& offsetof(hfdl_gpu_iqbal_stats, kappa_re) == 16 && offsetof(hfdl_gpu_iqbal_stats, kappa_im) == 20
		&& offsetof(hfdl_gpu_iqbal_stats, dc_re) == 24 && offsetof(hfdl_gpu_iqbal_stats, dc_im) == 28
		&& offsetof(hfdl_gpu_iqbal_stats, power) == 32 && offsetof(hfdl_gpu_iqbal_stats, image_rejection_db) == 36
		&& offsetof(hfdl_gpu_iqbal_stats, valid) == 40 && offsetof(hfdl_gpu_iqbal_stats, hold) == 44, "the fields");

static int (*const pinned_enable)(hfdl_gpu_frontend *, int32_t, float) = hfdl_gpu_frontend_iqbal_enable;
static int (*const pinned_seed)(hfdl_gpu_frontend *, int32_t, float, float, float, float, int) = hfdl_gpu_frontend_iqbal_seed;
static int (*const pinned_stats)(hfdl_gpu_frontend *, int32_t, hfdl_gpu_iqbal_stats *) = hfdl_gpu_frontend_iqbal_stats;
static int (*const pinned_blocks)(int, const void *, int32_t, int32_t, int, float, const float *, int, float *, hfdl_gpu_iqbal_stats *) = hfdl_gpu_iqbal_blocks;
static int (*const pinned_set)(float) = hfdl_frontend_set_iq_correction;
int hfdl_gpu_iqbal_abi_unused(void) { return pinned_enable == 0 || pinned_seed == 0 || pinned_stats == 0 || pinned_blocks == 0 || pinned_set == 0; }
