/* The prototype include/hfdl_host.h adds for the channel baseband export, pinned as tests/abi/hfdl_host_abi.c pins the rest: a host
 * program compiled against it passes a directory, a list of int32_t frequencies in Hz, their count, the format (0 = cf32, 1 = cs16,
 * HFDL_GPU_EXPORT_* of include/hfdl_gpu.h) and the cs16 scale.  Not in the reference.  Compiled by tests/test_export_cpu.py; syntax
 * check only, nothing runs. */
#include <stdint.h>
#include "hfdl_host.h"
#include "hfdl_gpu.h"

static int (*const pinned)(const char *, const int32_t *, int32_t, int, float) = hfdl_frontend_set_iq_export;
_Static_assert(HFDL_GPU_EXPORT_CF32 == 0 && HFDL_GPU_EXPORT_CS16 == 1, "the formats hfdl_frontend_set_iq_export() takes");
_Static_assert(sizeof(hfdl_gpu_export_block) == 8, "hfdl_gpu_export_block is one uint64_t");
int hfdl_host_export_abi_unused(void) { return pinned == 0; }
