// launch_timers.h -- internal: the event a launch site hands to the streams that wait for it, and the ledger of a front end's timed
// launches.  Named by frontend.h (the channelizer's launch sites) and demod.h (the demodulator's); the code is hfdl_gpu.cpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>
#include "hip_handles.h"
#include "kernels.h"

namespace hfdl {

// What the next stream waits for.  A launch site owns one fixed event; a TIMED launch carries a pooled start / stop pair on its dispatch
// (one dispatch carries one start and one stop), so its stop event doubles as its done event.  event() is what the newest launch
// signalled.  settle(), once everything queued is complete, puts the fixed event back in the pooled one's place before the pool hands
// that one out again: a completed event stands for "done" as well as any other.
struct DoneEvent {
	Event own;
	hipEvent_t cur = nullptr;
	hipEvent_t signal() { return cur = own; }                     // an untimed launch: its dispatch signals the fixed event
	hipEvent_t event() const { return cur ? cur : own.e; }
	bool pending() const { return cur != nullptr; }               // a launch has signalled it: there is something to wait for (not before the first launch)
	void settle() { if (cur) cur = own; }
};

// The timed kernel launches of a front end (hfdl_gpu_frontend_reset_timers), by stage in the order of hfdl_gpu_frontend_stage_times().
// A timed launch carries a start / stop event pair on its own dispatch (hipExtLaunchKernelGGL): no extra packet in the queue.  The
// pairs come from a pool filled outside any timed region and are read back and returned to it by the next drain (a sync / poll).
enum Stage { ST_FFT, ST_FOLD, ST_IFFT, ST_DEMOD, ST_DECODE, ST_N };
static_assert(ST_N == 5, "hfdl_gpu_frontend_stage_times() reports five stages");
struct LaunchTimers {
	struct Timed { Event start, stop; int blocks; };
	struct Totals { double ms = 0; int64_t launches = 0, blocks = 0; std::vector<Timed> pending; };     // read so far; launched, not yet read
	bool on = false;
	Totals stage[ST_N];
	std::vector<Timed> pool;            // free pairs, made by reset() outside any timed region
	int64_t fold_shapes[FOLD_MAX_BLOCKS + 1] = {};   // fold launches by block count
	double fold_shape_ms[FOLD_MAX_BLOCKS + 1] = {};  // ... and their kernel time
	Event first_fold;                   // start of the first timed fold since the reset: anchor of the steady-state step period
	double span_ms = 0;                 // first timed fold start -> last timed fold start
	int64_t fold_last_blocks = 0;       // blocks of the last timed fold

	// timing on: a pair from the pool (made here when a long run without a drain has used it up -- a timed launch is never silently
	// untimed) into `start` / `stop`.  Timing off: both are left as they are.
	int arm(Stage s, int blocks, hipEvent_t &start, hipEvent_t &stop);
	// ... for a launch other streams wait for: the stop event stands in as its done event; timing off, the launch signals `done`'s own
	int arm(Stage s, int blocks, DoneEvent &done, hipEvent_t &start)
	{
		hipEvent_t stop = done.signal();
		const int rc = arm(s, blocks, start, stop);
		done.cur = stop;
		return rc;
	}
	int drain();                // every timed launch is complete: add it up, the pairs go back to the pool
	int reset(bool enable);     // after a drain: every total to zero; timing on fills the pool with enough pairs for the launches between two drains
};

}  // namespace hfdl
