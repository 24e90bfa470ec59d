/* The prototypes include/hfdl_host.h adds for retuning a channel, pinned as tests/abi/hfdl_host_abi.c pins the rest: a host program
 * passes the two frequencies in Hz as int32_t, and for a scheduled request the signal time in seconds as a double in front of them;
 * hfdl_run_stats ends with the count of applied requests.  Not in the reference.  Compiled by tests/test_retune_device_cpu.py; syntax
 * check only, nothing runs. */
#include <stddef.h>
#include <stdint.h>
#include "hfdl_host.h"

static int (*const pinned_now)(int32_t, int32_t) = hfdl_frontend_retune;
static int (*const pinned_at)(double, int32_t, int32_t) = hfdl_frontend_schedule_retune;
_Static_assert(offsetof(struct hfdl_run_stats, retunes) + sizeof(uint64_t) == sizeof(struct hfdl_run_stats), "retunes is hfdl_run_stats' last member");
int hfdl_host_retune_abi_unused(void) { return pinned_now == 0 || pinned_at == 0; }
