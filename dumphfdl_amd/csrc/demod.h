// demod.h -- host-side owner of the per-channel demodulator / burst decoder device state (K4 + K5) and of a closed half's way through
// them: from "this half is yours" (launch_half) to "these PDUs are ready" (collect_ready).  planner.h DemodOrder is the ordering rule.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstddef>
#include <memory>
#include <vector>
#include "../../include/hfdl_gpu.h"
#include "hip_handles.h"
#include "kernels.h"
#include "launch_timers.h"
#include "planner.h"

namespace hfdl {

struct ChanState;
struct ChanScalars;
struct FrameRec;

struct DemodImage;                          // demod_host.cpp: host image of the tables + the device image's resolved pointers

// Frame quality records (hfdl_gpu_frontend_quality_enable; quality.h): off = none, no launch.  One launch behind the burst decoder of
// every demodulator launch, on its stream; a ring claimed like the PDU ring, its counts snapshot behind the launch like h_snap.
struct FrameQuality {
	static constexpr int CHUNK = 32;        // records a collection copies per wait on its stream (with symbols: 1.3 MB)
	int ring = 0;
	uint32_t taken = 0, dropped = 0;
	DevArray<hfdl_gpu_frame_quality> d_recs;        // [ring]
	DevArray<float2> d_syms;                // [ring][5040] with HFDL_GPU_QUALITY_SYMBOLS, else null
	DevArray<int> d_counts;                 // [1] records produced, [2] frames dropped, [3] records taken by the host
	PinnedBuf<int> h_snap;                  // [2][4]: d_counts as of the end of the newest launch of half 0 / 1
	PinnedBuf<hfdl_gpu_frame_quality> h_recs;       // [CHUNK] bounce buffers of a collection
	PinnedBuf<float2> h_syms;               // [CHUNK][5040]
	Event ev_last;                          // recorded behind the newest quality launch and its snapshot
	bool launched = false;
};

// Members in the order streams, memory, events (destroyed in reverse, frontend.h).  Nothing here waits for the collection stream when it
// goes: ~hfdl_gpu_frontend() synchronises it with the front end's own streams, before any member of either is destroyed.
struct Demod {
	int nch = 0, outs = 0, cap = 0;         // cap = max 5400-sps samples per demodulator launch (`batch` blocks)
	int batch = 1;                          // blocks a launch can take: what was asked for, cut down by fit_batch
	int frames_per_chan = 1, data_slots = 2;        // frame records per channel and set, data slots per channel: from the launch's signal time (planner.h plan_frame_slots)
	uint32_t taken = 0, dropped = 0;
	DemodOrder order;                       // which frame queue, counter, wait and done event a launch gets; which snapshot a poll reads
	int bounce_cap = 0;
	int pdu_cap = 0;
	bool taps_on = true;                    // stage-tap buffers allocated
	bool taps_enabled = true;               // written by the kernel this block
	size_t lds_bytes = 0;
	// Collection runs beside the kernels: device -> host copies go through page-locked bounce buffers on a stream of their own.
	// (A synchronous hipMemcpy waits for the kernels in flight -- up to a whole demodulator launch, ~1 ms on the small geometries,
	// every time a PDU is collected: profiles/r03_experiments.md.)
	Stream st_collect;
	std::unique_ptr<DemodImage> img;
	DevBuf d_tables;                        // packed DemodTables image
	DevArray<ChanState> d_states;
	DevArray<float2> d_data;                // [nch][data_slots][5040] equalised data symbols, a ring of slots per channel
	DevArray<FrameRec> d_frames;            // [2][nch * frames_per_chan]: frames finished by the demodulator of an even / odd launch
	DevArray<int> d_counts;                 // [1] pdus produced, [2] pdus dropped, [3] pdus taken by the host, [4..7] frames queued, one counter per launch mod 4
	DevArray<hfdl_gpu_pdu> d_pdus;
	DevArray<int32_t> d_freqs;
	DevArray<ChanState> d_state_image;      // one ChanState as chan_state_init() makes it: allocated by the first retune, never otherwise
	PinnedBuf<ChanState> h_state_image;     // ... and where it is uploaded from (no pageable copy, no wait)
	std::vector<int> retuned;               // channels whose state reset is queued and not known to have run: stats_all() reports them fresh
	DevArray<float2> d_tap_rs, d_tap_mf, d_tap_sym;      // stage taps
	DevArray<float> d_tap_lvl;
	DevArray<int> d_tap_counts;             // [nch][2]
	PinnedBuf<int> h_snap;                  // [2][4]: d_counts as of the end of the newest launch of half 0 / 1
	PinnedBuf<hfdl_gpu_pdu> h_pdu_bounce;   // [bounce_cap]
	PinnedBuf<ChanScalars> h_stats_bounce;  // [nch]
	Event ev_dec[2];                        // decoder of an even / odd launch done: its frame queue and counter may be reused (made by the first such decoder)
	Event ev_retuned;                       // rides on the newest retune_demod_kernel (made by the first retune)
	// demodulator launch of the half in buffer 0 / 1 done (its decoder may start), the LAST launch of the half at [0]: the half is free
	DoneEvent dm[2][PLAN_MAX_HALF];
	Event ev_demod[3];                      // recorded behind the last burst decoder of a half, in turn (DemodOrder::decoded_event)
	uint64_t halves_launched = 0;           // order.halves as of the newest launch_half(): equal = the newest half's ev_demod has been recorded
	std::unique_ptr<FrameQuality> quality;  // null: off (its memory and its event go before the members above: nothing queued uses them then, quality_enable)

	Demod();
	~Demod();
	static int fit_batch(int outs, float resamp_rate, int want);     // blocks a launch can take at most, `want` or fewer (the block table, 16-bit output counts)
	static size_t workgroup_lds();          // LDS bytes of a demodulator workgroup: the same for every launch length
	int init(int nch, int outs, float resamp_rate, const int32_t *freqs, hipStream_t st, int batch_want = 1);
	// A closed half of `nblk` consecutive blocks -- chan_out [nblk][nch][outs], out_count [nblk][nch] -- `batch` blocks per launch, each
	// launch followed by its burst decoder.  Stream B first waits for `ready` (the half's channelizer output is there; null: it is
	// there already).  Every done event rides on its kernel's dispatch; timed launches take their pairs from `timers`.
	int launch_half(const float2 *chan_out, const int *out_count, int nblk, int half, hipEvent_t ready, hipStream_t st_b, hipStream_t st_d, LaunchTimers &timers);
	hipEvent_t half_read_event(int half) const { return dm[half][0].pending() ? dm[half][0].event() : nullptr; }      // what the inverse FFT into `half` waits for; null: nothing
	// What stream A waits for so that the next launch needs no wait of its own for the decoder of two launches ago (null: nothing, and
	// the launch needs none either).  Only with a decode stream of its own; the launch is told (DemodOrder::wait_on_a).
	hipEvent_t frames_free_event() { return order.wait_on_a() ? ev_dec[order.next_set()].e : nullptr; }
	void settle() { for (auto &half : dm) for (DoneEvent &d : half) d.settle(); }        // everything queued is complete
	int collect(hfdl_gpu_pdu *out, int32_t max, int32_t *n, hipStream_t st);                    // stream idle: everything produced
	// the pipeline keeps running: what the ring is known to hold once the last demodulator of the half before the newest is done --
	// waited for, or (wait = false) asked after: not done yet, nothing is taken
	int collect_ready(bool wait, hfdl_gpu_pdu *out, int32_t max, int32_t *n, hipStream_t st);
	int take(unsigned produced, hfdl_gpu_pdu *out, int32_t max, int32_t *n, hipStream_t st);
	// Retune of channel c (hfdl_gpu_frontend_retune_channel): prepare_retune() makes the state image (the first call allocates it and
	// queues its upload on `st_b`; nothing else changes if it fails); enqueue_retune() queues the state reset behind the demodulators
	// on `st_b` and the new PDU frequency behind the burst decoders on `st_d`.  From then on the channel's statistics are a fresh
	// channel's: until the reset is known to have run, stats_all() -- which waits for nothing -- reports the image's counters for it,
	// never the old ones, so a reader never sees a counter rise and then run backwards.
	int prepare_retune(hipStream_t st_b);
	void enqueue_retune(int c, int32_t freq, hipStream_t st_b, hipStream_t st_d);
	// Frame quality records.  quality_enable: ring = 0 turns them off; else a fresh, empty ring from the next launch queued on; either way
	// it first waits for the quality launches queued so far, and an allocation that fails leaves everything as it was.  quality_read:
	// the oldest records not taken yet that are KNOWN to be complete: it asks after the halves' last burst decoders (the quality launch
	// and its snapshot sit in front of the event they carry) and believes the snapshot DemodOrder allows, never waiting for a kernel.
	int quality_enable(int ring, bool symbols);
	int quality_read(hfdl_gpu_frame_quality *out, float *symbols, int32_t max, int32_t *n, uint32_t *dropped, hipStream_t st);
	int stats_all(hfdl_gpu_channel_stats *out, int n);
	int tap(int what, int channel, const void **src, size_t *nfloats);
	int stats(int channel, hfdl_gpu_channel_stats *out);
	int read_constants(void *tables, size_t tables_bytes, void *constants, size_t constants_bytes);   // laboratory read-back: sizeof(DemodTables), sizeof(HfdlConstants)
private:
	// the two kernels of launch `p`: K4 (`done` is signalled by its dispatch packet), then K5 + the PDU-ring snapshot of `half`; the
	// start / stop events ride on the dispatches (timing)
	int enqueue_demod(const DemodLaunch &p, const float2 *chan_out, const int *out_count, int nblk, hipStream_t st, hipEvent_t done, hipEvent_t start);
	int enqueue_decode(const DemodLaunch &p, int half, hipStream_t st, hipEvent_t start, hipEvent_t stop);
	int collect_snapshot(int slot, hfdl_gpu_pdu *out, int32_t max, int32_t *n, hipStream_t st);  // up to the end of the launch that wrote the slot
	bool decoded(int back);                 // the last burst decoder of the newest half (0), the one before (1), before that (2) is found done
};

}  // namespace hfdl
