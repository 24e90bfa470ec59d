// frontend.h -- internal: the front end behind the opaque hfdl_gpu_frontend of include/hfdl_gpu.h and what the translation units of the
// shim share (namespace hfdl; the launch ledger and the done events are launch_timers.h's).  hfdl_gpu.cpp is the pipeline,
// frontend_create.cpp builds a front end, frontend_query.cpp reads one, frontend_options.cpp holds the opt-in stages (switch, pipeline
// hook and reader of each; their state is declared here), demod_host.cpp owns its demodulator state and a closed half's
// way through demodulator and burst decoder (demod.h), stages.cpp holds the one-shot stage entry points (checks, staging
// and read-back; the kernels' launchers are beside the kernels), lab.cpp the laboratory build's switches, probes and stage.
#pragma once
#include <hip/hip_runtime.h>
#include <complex>
#include <deque>
#include <memory>
#include <vector>
#include "../../include/hfdl_gpu.h"
#include "hip_handles.h"
#include "kernels.h"
#include "planner.h"
#include "retune_launch.h"
#include "launch_timers.h"
#include "demod.h"
#include "spectrum.h"
#include "export_ring.h"
#include "blanker.h"
#include "iqbal.h"
#include "notch.h"
#include "real_input.h"

namespace hfdl {

int select_device(int device);        // checks the index and the architecture, hipSetDevice
int check_channel_span(int32_t sample_rate, int32_t nrx, int c, int32_t freq, int r, int32_t centre);     // channel c on `freq` inside +-fs/2 of the centre of its receiver r
long env_long(const char *name, long lo, long hi, long otherwise);
inline int ilog2(int x) { int l = 0; while ((1 << l) < x) l++; return l; }
inline size_t sample_bytes(int fmt) { return fmt == SFMT_CS16 ? 4 : fmt == SFMT_CU8 ? 2 : 8; }
bool is_library_pinned(const void *p, size_t bytes);     // inside a range handed out by hfdl_gpu_host_alloc()

// The A/B switches of the measurement scripts, read by ONE function (lab.cpp).  They exist in the laboratory build only (-DHFDL_LAB,
// libhfdl_gpu_lab.so): the product build returns these defaults and carries neither a getenv nor a knob's name for them.
struct LabConfig {
	int fold_tile = -1;            // HFDL_GPU_FOLD_TILE: index of the fold tiling to use instead of the first that fits
	int fold_slices = 0;           // HFDL_GPU_FOLD_SLICES (BatchOverrides::fold_slices)
	int cu_split = 0;              // HFDL_GPU_CU_SPLIT = k (2 .. 8): the demodulator's stream on every k-th CU, the channelizer's on the others
	bool cu_partition = false;     // HFDL_GPU_CU_PARTITION=1: the planner's CU partition of the fold-bound geometries (planner.h plan_cu_partition)
	int fft_stream = -1;           // HFDL_GPU_FFT_STREAM 0 / 1: every forward FFT on stream A / on a stream of their own, instead of "by where the block lies" (their own stream where the CU partition applies)
	bool decode_stream = true;     // HFDL_GPU_DECODE_STREAM: the burst decoders on a stream of their own
	int fold_bound = -1;           // HFDL_GPU_FOLD_BOUND 0 / 1: instead of "128 channels and more"
	bool fold_ramp = true;         // HFDL_GPU_FOLD_RAMP=0: every half the full size from the start
};
LabConfig read_lab_config();

struct HostFftPlan {
	FftPlan p{};
	DevBuf tw[3];
	int build(int n);
};
int upload_twiddles(int r, DevBuf &out);

// One-shot stages (stages.cpp).  finish_stage: the stage's launches are queued on the null stream -- wait for them and report what they
// left.  StageFrames: K5's inputs for `nframes` frames whose data symbols lie back to back in `symbols` -- frame i is channel i, slot 0
// of `data` ([nframes][2][MAX_DATA_SYMBOLS]), unit levels, sample index i -- and the decoder's constants (scrambler, constellations).
int finish_stage();
struct StageFrames {
	DevBuf frames, data, scrambler;
	int upload(const float *symbols, const int32_t *modes, const int32_t *bitmask_lsb, int32_t nframes);
};

// ---------------------------------------------------------------- front end

// History of finished interval rows (hfdl_gpu_frontend_spectrum_history): a ring of `rows` accumulator sets in HBM.  Row i lives in
// slot i % rows; the monitor's launch adds every block into the open row's slot (spectrum.h row_acc), so closing a row is host
// bookkeeping alone: the next launch targets the next slot with its "start over" bit set, which is also how row i + rows takes the
// slot over from row i.  ev[slot] rides on every launch into the slot: once a row is closed, its slot's event stands for "the row's
// last launch has run" until the slot is re-targeted.
struct SpectrumHistory {
	static constexpr int CHUNK = 8;     // rows a collection copies per wait on its stream
	int rows = 0, interval = 0;         // interval > 0: a row closes by itself after that many blocks
	DevBuf acc, peak;                   // [rows][nrx][bins] float2 / float (peak with MAXHOLD)
	PinnedBuf<float> host;              // bounce buffer of a collection: [CHUNK] x ([bins] float2 + [bins] float)
	std::vector<Event> ev;              // [rows]
	std::vector<hfdl_gpu_spectrum_row> info;    // [rows] the closed row each slot holds
	uint64_t open = 0;                  // index of the open row = rows closed so far
	uint64_t open_first = 0;            // the open row's first block ...
	uint32_t open_blocks = 0;           // ... and how many it has so far (0: its slot still holds row open - rows)
	uint64_t oldest() const { const uint64_t kept = (uint64_t)rows - (open_blocks ? 1 : 0); return open > kept ? open - kept : 0; }
	void close()
	{
		info[open % (uint64_t)rows] = hfdl_gpu_spectrum_row{ open, open_first, open_blocks, 0 };
		open++;
		open_blocks = 0;
	}
};

// Spectrum monitor (hfdl_gpu_frontend_spectrum_enable; spectrum.h): off = no monitor, no launch.  One launch per step behind the forward
// FFT's last pass.  A dispatch carries ONE stop event: `ev` without the history, the open row's slot event with it -- `last` is the one
// the newest launch carried, so a read waits for the newest launch without a packet of its own on the stream either way.
struct SpectrumMonitor {
	int bins = 0;
	uint32_t flags = 0;
	DevBuf acc;                         // [nrx][bins] float2 { sum, compensation } of the band powers
	DevBuf peak;                        // [nrx][bins] float with MAXHOLD
	PinnedBuf<float> host;              // bounce buffer of a read: [bins] float2 + [bins] float
	DevBuf scratch;                     // [nrx][N] float2 where the fold runs in the mixed domain: the one block's spectrum pass 3 makes for the monitor alone
	Event ev;
	hipEvent_t last = nullptr;          // null: no launch yet, or everything launched has been waited for
	hipEvent_t newest() const { return last ? last : ev.e; }
	uint64_t fresh = 0;                 // receivers whose accumulators the next launch overwrites (after enable / a read with reset)
	std::vector<uint64_t> blocks, first;        // [nrx] blocks accumulated since the receiver's last reset, index of the first of them
	std::unique_ptr<SpectrumHistory> hist;      // null: no history, no extra allocation, row_acc == nullptr
};

// Channel baseband export (hfdl_gpu_frontend_export_enable): off = none, no launch.  One launch per closed half on stream A, behind the
// half's inverse FFT / NCO launch, packs the selected channels' rows of the half's blocks into a ring in HBM (spectrum.h ExportJob);
// block b lives in slot b % R.  ev[i] rides on the dispatch of the launch on record i (export_ring.h), so "has block b been written"
// is a hipEventQuery and a collection never waits for a kernel stream.
struct ChannelExport {
	int nsel = 0, format = 0;
	float scale = 1.f;
	ExportRing ring;
	DevBuf channels;                    // [nsel] int32
	DevBuf samples, counts, power, clipped;     // [R][nsel][P] float2 / short2; [R][nsel] int32 / float / uint32
	size_t chunk = 1;                   // blocks a collection copies per wait on its stream
	PinnedBuf<char> host;               // its bounce buffer: [chunk] samples, then [chunk] counts, power, clipped
	std::vector<Event> ev;              // [R]
	std::vector<uint64_t> last_of;      // [R] last block of the launch on each record
	hipEvent_t newest = nullptr;        // what the newest launch carried (null: no launch yet)
};

// Impulse-noise blanker (hfdl_gpu_frontend_blanker_enable; blanker.h): never enabled = none, no launch.  The first stage of the input
// chain (frontend_options.cpp condition_input): two launches per step, `ev` on the second one's dispatch.  Turned off again (k2 = 0)
// the buffers stay until the front end goes.
struct Blanker {
	float k2 = 0.f;                     // (float)10^(threshold_db / 10); 0: off
	DevBuf partial;                     // [nrx][blank_chunks(input_size)] float
	DevBuf rec;                         // [nrx] BlankRecord
	PinnedBuf<BlankRecord> host;        // bounce buffer of a read: one record
	Event ev;
	uint64_t blocks = 0;                // steps blanked so far
};

// I/Q imbalance and DC corrector (hfdl_gpu_frontend_iqbal_enable; iqbal.h): never enabled = none, no launch.  The second stage of the
// input chain: one launch per step, `ev` on its dispatch -- what a read of the record, and a seed, wait for.  State and chunk sums live
// in two slots, written in turn (`step` counts the launches).  Turned off again the buffers stay until the front end goes.
struct Iqbal {
	std::vector<float> alpha;           // [nrx] 0: off
	bool any_on = false;
	uint64_t restart = 0;               // receivers whose next block is the first after an enable
	DevBuf partial;                     // [2][nrx][5][blank_chunks(input_size)] float
	DevBuf state;                       // [2][nrx] IqbalState
	DevBuf seed;                        // [nrx] IqbalSeed
	PinnedBuf<IqbalState> host;         // bounce buffer of a read: one record
	Event ev;
	uint64_t step = 0;                  // launches so far: launch i writes slot i & 1
	uint32_t seeds = 0;                 // generation of the newest seed
};

// Adaptive carrier canceller (hfdl_gpu_frontend_notch_enable; notch.h): never enabled = none, no launch.  One launch per closed half on
// stream B, in the half's hand-over to the demodulator (launch_canceller): it reads the half's rows of d_chan_all and leaves
// what the demodulator reads in `out`, a second buffer of d_chan_all's shape -- the channel export and stage tap 3 keep reading the
// channelizer's own output.  Stream order is the only ordering: the canceller of half h + 2 overwrites `out` behind the demodulators of
// half h, and the inverse FFT into a half waits for that half's last demodulator, which is queued behind the canceller that read it.
// `ev` rides on the launch's dispatch.  Turned off again (mu = 0) the buffers stay until the front end goes.
struct Notch {
	float mu = 0.f;                     // 0: off
	int nsel = 0;
	std::vector<bool> selected;         // [nch]
	DevBuf out;                         // [2][half_blocks][nch][outs] float2
	DevBuf sel;                         // [nch] int32: the selected channels, nsel of them
	DevBuf state;                       // [nch][NOTCH_STATE_FLOATS] float
	DevBuf rec;                         // [nch] NotchRecord
	PinnedBuf<NotchRecord> host;        // bounce buffer of a read: one record
	PinnedBuf<int32_t> host_sel;        // [nch] where an enable's selection is uploaded from ...
	Event staged;                       // ... recorded behind that upload: the next enable waits for it before it writes host_sel again
	bool staging = false;
	Event ev;
	bool launched = false;              // since the newest enable
};

// Retune (hfdl_gpu_frontend_retune_channel): what the first call allocates and later ones keep.  The new time-domain taps go through one
// of two page-locked buffers into `pad` (N points, zeroed once: only the first taps_length are ever written), and the tap FFT has a work
// buffer of its own -- d_work belongs to the chain of forward FFTs, which may be running on another stream.  staged[i] rides on the first
// pass of the tap FFT behind the copy out of stage[i]: the call's only host wait.  `done` rides on retune_channelizer_kernel.
struct Retune {
	DevBuf pad, work;
	DevBuf eo;                          // a real front end: the transforms of the even and the odd taps, 2 N' words (queue_real_taps)
	PinnedBuf<float2> stage[2];
	Event staged[2];
	DoneEvent done;
	uint64_t calls = 0;
	std::vector<float> lp;              // the low-pass prototype every channel's band-pass is made from (planner.h design_bandpass), kept between calls
	float lp_cut = -1.f;
};

}  // namespace hfdl

// One channel as create designs it (frontend_create.cpp): the channelizer constants and the taps_length time-domain taps of a channel of
// receiver `rx` on `freq`.  build_taps() and a retune call the same function, so a retuned channel's are a fresh create's bit for bit.
// lp / lp_cut: the caller's cache of the low-pass prototype (planner.h design_bandpass); taps == nullptr: the constants alone.  False: the
// planner refuses the shift.
bool design_channel(const hfdl_gpu_frontend *fe, int rx, int32_t freq, hfdl::ChanConst &k, std::complex<float> *taps, std::vector<float> &lp, float &lp_cut);
// A real front end (real_input.h): design_channel leaves taps_host_len() words, the even taps and then the odd ones, each a zero-padded
// input of the N'-point plan.  queue_real_taps queues, on `st`, their two transforms -- through `pad` (N' words, zero past taps_length)
// and `work` into eo[0 .. N') and eo[N' .. 2N') -- and the combine into padded slot `slot` of the tap buffer.  `host` is read by the two
// copies; `staged` (may be null) rides on the pass that reads `pad` last.  build_taps() and a retune both call it.
int queue_real_taps(hfdl_gpu_frontend *fe, const float2 *host, float2 *pad, float2 *work, float2 *eo, int slot, hipStream_t st, hipEvent_t staged);

// hfdl_gpu.cpp, for a change of setting: everything pushed so far goes on under the present one
int close_boundary(hfdl_gpu_frontend *fe);
// the opt-in stages' hooks (frontend_options.cpp): each one line of the pipeline, and nothing where its stage is off
void condition_input(hfdl_gpu_frontend *fe, hfdl::FftInputs &in, int &fmt, hipStream_t st);       // enqueue_fft: the input chain in front of pass 1
void launch_monitor(hfdl_gpu_frontend *fe, const float2 *spectrum, hipStream_t st);               // enqueue_fft: behind the forward FFT's last launch
const float2 *launch_canceller(hfdl_gpu_frontend *fe, int slot0, int nblk, hipEvent_t ready);     // launch_demod: the rows the demodulators read; null: off
int canceller_retuned(hfdl_gpu_frontend *fe, int channel);                                        // retune: the channel's canceller starts afresh
void launch_export(hfdl_gpu_frontend *fe, int slot0, int nblk);                                   // close_half: behind the inverse FFT

// Members are destroyed in reverse order of declaration: events first, then memory, then the streams (the destructor has synchronised
// them).  So: streams, then memory, then events.
struct hfdl_gpu_frontend {
	int device = 0;
	hfdl::Stream stream;                // A: forward FFTs of the uploaded blocks of the half being filled, then ONE fold and ONE inverse FFT / NCO launch per half
	hfdl::Stream stream_b;              // B: demodulator launches of half k-1, beside the forward FFTs and the fold of half k
	hfdl::Stream stream_d;              // D: burst decoders + PDU snapshots, off the demodulators' critical path (an alias of B only in a laboratory A/B run)
	hfdl::Stream stream_c;              // C, the input stream: whatever brings a block's samples to the transform -- the host -> device copy of a host block into the staging ring (up to n_stage - 1 blocks ahead of the blocks that compute), the forward FFT itself of a device-resident block, beside the fold of the half before
	hfdl::Stream stream_f;              // F: laboratory only (the CU partition, HFDL_GPU_FFT_STREAM=1): every forward FFT on a stream of its own; not created otherwise
	bool cu_partitioned = false;        // streams A, F and B are bound to disjoint sets of CUs (planner.h plan_cu_partition)
	bool own_decode_stream() const { return stream_d.owned; }
	hfdl::FftRule fft_rule = hfdl::FFT_RULE_INPUT;      // which side a block's forward FFT runs on (planner.h)
	hfdl::FftOrder order;               // ... and what orders it against its neighbours
	int side_of(bool on_device) const { return hfdl::fft_side(fft_rule, on_device); }
	hipStream_t fft_stream(int side) const { return side == hfdl::FFT_SERIAL ? stream.s : stream_f.owned ? stream_f.s : stream_c.s; }
	static constexpr int MAX_HALF = hfdl::FOLD_MAX_BLOCKS;      // blocks per half at most: what one fold launch can take (32)
	static constexpr int MAX_STAGE = HFDL_GPU_PREFETCH_MAX + 1;      // staging buffers for host input at most: uploads run at most 17 blocks ahead
	static_assert(MAX_HALF == hfdl::PLAN_MAX_HALF && MAX_STAGE == hfdl::PLAN_MAX_STAGE && HFDL_GPU_FOLD_BATCH_MAX == MAX_HALF, "include/hfdl_gpu.h, kernels.h and planner.h name the same limits");

	// ---- memory.  `mem` owns every buffer allocated at create; the typed pointers below are views into it.
	std::deque<hfdl::DevBuf> mem;
	template <typename T> hipError_t alloc(T *&view, size_t count)
	{
		mem.emplace_back();
		const hipError_t e = mem.back().alloc(sizeof(T) * count);
		view = mem.back().as<T>();
		return e;
	}
	hfdl::HostFftPlan fft;
	// (its own stream, memory and events, in that order: they go between the front end's events and its memory.  Safe, because the
	// destructor has synchronised every stream, the demodulator's collection stream among them, before the first member goes, and
	// nothing the front end owns is queued on that stream or waits for those events afterwards.)
	hfdl::Demod demod;                  // from "this half is yours" to "these PDUs are ready": the launches, their done events, what a poll reads
	int4 *d_rx = nullptr, *d_grp = nullptr;      // device copies: receiver table, fold group tables (kernels.h Geometry::grp_tab)
	float2 *d_hist[2] = { nullptr, nullptr }, *d_work = nullptr, *d_spec = nullptr, *d_taps = nullptr, *d_partial = nullptr;
	float2 *d_tw_m = nullptr;
	// Host input goes through a RING of n_stage = min(half_blocks + 2, MAX_STAGE) staging buffers in HBM: host block j is copied (stream
	// C) into buffer j % n_stage, which the forward FFT's first pass of block j - n_stage has finished reading -- that pass runs BEFORE the
	// fold of its half, so uploads run up to n_stage - 1 blocks ahead (a whole half of up to 16 blocks, 17 blocks of a 32-block half) and
	// never sit behind the fold (with two buffers, upload k+2 waited for FFT k, which waited for the fold of the half before: the link
	// idled a third of the time).
	int n_stage = 0;
	std::unique_ptr<hfdl::DevBuf> d_stage[MAX_STAGE];     // allocated (and grown) by the first copy that needs it
	size_t stage_cap[MAX_STAGE] = {};
	// Channelizer output, double-buffered between stream A and stream B in two HALVES of `half_blocks` blocks each:
	// [2][half_blocks][nch][outs].  The forward FFT of a block is queued when it is pushed; the fold and the inverse FFTs run when a
	// half is closed (full, or a sync / poll found it part-filled): ONE pass over the filter taps serves up to `fold_nb` blocks.
	// The demodulator then takes the half `batch` blocks per launch while the channelizer fills the other half.
	float2 *d_chan_all = nullptr;
	int *d_cnt_all = nullptr;           // [2][half_blocks][nch] outputs per channel of each block
	hfdl::ChanConst *d_cc = nullptr;
	int2 *d_win = nullptr;              // pruned fold: window of quads of alias rows per octet (kernels.h Geometry::fold_win)
	hfdl::NcoState *d_nco = nullptr;    // [nch] carried NCO state, owned by the forward FFT's rider workgroups (kernels.h NcoJob)
	hfdl::NcoState *d_nco_snap = nullptr;     // [half_blocks][nch] the state each block of the half starts from
	float2 *d_ph = nullptr, *d_ph_cont = nullptr;      // [half_blocks] NCO phasor tables [outs][nch] and the riders' segment hand-over [nch]
	std::unique_ptr<hfdl::SpectrumMonitor> mon;        // null: off
	float2 *monitor_scratch() const { return mon ? mon->scratch.as<float2>() : nullptr; }      // mixed domain: where pass 3 runs for the monitor alone (null: it does not run)
	std::unique_ptr<hfdl::ChannelExport> exp;          // null: off
	std::unique_ptr<hfdl::Retune> retune;              // null: no channel has been retuned
	std::unique_ptr<hfdl::Blanker> blank;              // null: never enabled
	std::unique_ptr<hfdl::Notch> notch;                // null: never enabled
	std::unique_ptr<hfdl::Iqbal> iqbal;                // null: never enabled
	// the input chain's one scratch, [nrx][input_size] cf32 (frontend_options.cpp condition_input has the rule): allocated by the first
	// enable of either stage, kept until the front end goes -- the forward FFT queued last may still be reading it
	hfdl::DevBuf chain_scratch;

	// ---- events
	hfdl::DoneEvent chan[2];            // channelizer output of this half ready (rides on the inverse FFT)
	hfdl::DoneEvent fft_done;           // the last forward FFT of a half on stream A: what the held-back demodulators wait for
	hfdl::DoneEvent spec[2];            // newest forward FFT BESIDE the fold (stream C / F) of the half in spectrum set 0 / 1 done (rides on its last pass): what the half's fold waits for
	hfdl::Event ev_switch;              // recorded on the stream of the forward FFT before, where a block's FFT runs on the other one
	hfdl::Event ev_stage_ready[MAX_STAGE];      // copy of the host block in this buffer done: what its forward FFT and input_done_upto() wait for
	hfdl::Event ev_stage_free[MAX_STAGE];       // pass 1 of the forward FFT that read this buffer done (rides on that dispatch): the copy stream may refill it
	hfdl::LaunchTimers timers;
	int settle_events();                // after a sync: read the timed launches back, every DoneEvent settles

	// ---- plain state
	uint64_t host_blocks = 0;           // host blocks whose copy has been queued (pushed or prefetched)
	uint64_t host_pushed = 0;           // ... of which this many have been pushed (or cancelled): the rest wait in the prefetch queue, oldest first
	const void *pf_ptr[MAX_STAGE] = {}; // prefetch queue entry of host block j at [j % n_stage]: the host pointer ...
	int pf_fmt[MAX_STAGE] = {};         // ... and its sample format
	// The copy of host block j signals ev_stage_ready[j % n_stage].  Copies run in order on one stream, so for a block more than
	// n_stage - 1 behind the newest (its event has been re-recorded since) the oldest event still its own block's implies it.
	hipEvent_t input_event(uint64_t host_block) const
	{
		const uint64_t newest = host_blocks - 1, span = (uint64_t)n_stage - 1;
		return ev_stage_ready[(newest - host_block <= span ? host_block : newest - span) % (uint64_t)n_stage];
	}
	int32_t sample_rate = 0, decimation = 0;
	// Real-sampled input (hfdl_gpu_frontend_create_real; real_input.h): real_rate = fs_r, 0 for a complex front end.  sample_rate and
	// rx_center then describe the equivalent complex stream (fs_r / 2, base + fs_r / 4), which is what everything else is planned for;
	// d_real [nrx][N'] takes pass 3's unshifted output, and the untangle launch behind it fills the block's spectrum slot.
	int32_t real_rate = 0;
	std::vector<int32_t> rx_base;       // [nrx] the RF frequency at 0 Hz of each receiver's samples
	float2 *d_real = nullptr;
	size_t taps_host_len() const { return real_rate ? 2 * (size_t)plan.taps_length : (size_t)plan.taps_length; }
	float tbw = 0;
	hfdl::Plan plan{};                  // shift = 0 geometry (src/fft.c:70-86)
	hfdl::Geometry geo{};
	std::vector<int32_t> freqs;
	// Receivers (hfdl_gpu_frontend_create_multi): one stream of input_size samples per receiver and step, channels receiver-major.  Every
	// per-block buffer of the forward FFT holds one transform per receiver: overlap history [2][nrx][overlap], work [nrx][N], spectra
	// [set][block][nrx][N], staging buffers [nrx][input_size]; from the fold on, everything is per channel as with one receiver.
	int nrx = 1;
	std::vector<int32_t> rx_center;     // [nrx] centre frequencies
	std::vector<int32_t> rx_of;         // [nch] receiver of each channel
	std::vector<hfdl::RxSpan> rx_span;  // [nrx] padded tap slots and channels of each receiver (planner.h plan_receiver_slots)
	std::vector<int4> rx_host;          // the same as the kernels read it (Geometry::rx_tab / rx_host)
	int slot_of(int c) const { return hfdl::receiver_slot(rx_span[(size_t)rx_of[(size_t)c]], c); }
	std::vector<hfdl::ChanConst> cc;
	int batch = 1;                      // blocks per demodulator launch
	int fold_nb = 1;                    // blocks per fold launch
	int half_blocks = 1;                // slots per half: a multiple of fold_nb, at least `batch` (planner.h plan_batches)
	// How many blocks close the half being filled.  A pipeline that starts empty closes its first half at `half_first` blocks (16 where a
	// half holds 32): the first fold launch is the sixteen-column form and the demodulators start 3 ms earlier; once a half has been
	// closed BY FILLING -- the caller pushes faster than it collects -- the next ones take all `half_blocks`.  Any sync / poll that closes
	// a half early (a drain) starts over.  Results do not depend on where the halves are cut (test_fold_batching_changes_nothing).
	int half_first = 1, half_target = 1;
	int cur_half = 0, batch_fill = 0;   // the half being filled and the blocks already in it (forward FFT queued, fold not yet)
	int last_slot = 0;                  // slot (half * half_blocks + index) of the newest channelized block: what HFDL_GPU_TAP_CHAN_OUT reads
	int last_index = 0;                 // its index inside the half: spectrum / phasor-table slot of the newest block
	float2 *chan_slot(int slot) const { return d_chan_all + (size_t)slot * (size_t)geo.nch * (size_t)geo.outs; }
	int *cnt_slot(int slot) const { return d_cnt_all + (size_t)slot * (size_t)geo.nch; }
	// spectra, NCO phasor tables and carried-state snapshots of a half: two sets (the forward FFTs of half k+1 fill one while the fold
	// and inverse FFTs of half k read the other); `set` = cur_half of the half they belong to
	int last_set = 0;                   // set of the newest channelized half: what the taps read
	float2 *spec_slot(int set, int i) const { return d_spec + ((size_t)set * (size_t)half_blocks + (size_t)i) * spec_stride(); }
	size_t spec_stride() const { return (size_t)nrx * (size_t)geo.n; }     // between the spectra of consecutive blocks (receiver r at + r N)
	float2 *ph_slot(int set, int i) const { return d_ph + ((size_t)set * (size_t)half_blocks + (size_t)i) * ph_stride(); }
	hfdl::NcoState *snap_slot(int set, int i) const { return d_nco_snap + ((size_t)set * (size_t)half_blocks + (size_t)i) * (size_t)geo.nch; }
	size_t partial_stride() const { return (size_t)geo.nch * (size_t)geo.slices * (size_t)geo.m; }
	size_t ph_stride() const { return (size_t)geo.nch * (size_t)geo.outs; }
	double prune_tol = 0.0;             // HFDL_GPU_FOLD_PRUNE: share of a filter's energy (as an amplitude ratio) the skipped alias rows may hold; 0 = fold every row
	int fold_rows_max = 0;              // the longest row window (0: every row is folded)
	bool fold_bound = false;            // many channels: the fold bounds the block and the demodulator launches of a half are placed under the NEXT half's fold
	uint64_t blocks = 0;
	hfdl::FftOutLayout tap_layout;
	int pending_demod_buf = -1;         // half whose demodulator launches are held back until the next half's forward FFTs are queued ...
	int pending_demod_nblk = 0;         // ... and the blocks in it

	~hfdl_gpu_frontend();
};
