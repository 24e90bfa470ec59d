// planner.h -- host-side (C++) block-geometry planner and filter design of the GPU front end.
//
// Product code (not the oracle): mirrors, expression by expression, the float/double mixing of the reference's
// init-time arithmetic, because bin shifts and tap phases depend on it:
//   fastddc_init                      src/fastddc.c:46-80
//   decimating_shift_addition_init    src/libcsdr_gpl.c:26-39
//   firdes_lowpass_f / firdes_bandpass_c / Hamming kernel   src/libcsdr.c:62-68,83-133
//   compute_fft_decimation_rate, compute_filter_relative_transition_bw   src/libcsdr.c:135-144
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>
#include <complex>

namespace hfdl {

struct Plan {
	int32_t pre, post, taps_min_length, taps_length, overlap, n, m, input_size, post_input_size, scrap, v;
	int32_t startbin, offsetbin;
	float pre_shift, post_shift, sindelta, cosdelta, rate;
};

inline int32_t pow2_above(int32_t x)
{
	int32_t p = 1;
	for (int i = 0; i < 31; i++, p <<= 1) if (x < p) return p;
	return -1;
}

inline int32_t fft_decimation_rate(int32_t fs, int32_t target)
{
	return pow2_above((int32_t)std::floor((float)fs / (float)target)) / 2;
}

inline float relative_transition_bw(int32_t fs, int32_t hz) { return (float)hz / (float)fs; }

inline bool plan_block(Plan &p, float transition_bw, int32_t decimation, float shift_rate)
{
	p.pre = 1; p.post = decimation;
	while (true) {
		float h = (float)p.post / 2;
		if (std::floor(h) != h || p.post / 2 == 1) break;
		p.post /= 2; p.pre *= 2;
	}
	int32_t tl = (int32_t)(4.0 / transition_bw);
	p.taps_min_length = (tl % 2 == 0) ? tl + 1 : tl;
	p.taps_length = pow2_above((int32_t)(std::ceil((double)(p.taps_min_length / (float)p.pre)) * p.pre)) + 1;
	p.n = pow2_above(p.taps_length * 4);
	while (p.n < p.pre) p.n *= 2;
	p.overlap = p.taps_length - 1;
	p.input_size = p.n - p.overlap;
	p.m = p.n / p.pre;
	p.v = p.n / p.overlap;
	const int32_t mid = p.n / 2;
	float sb = (float)mid + (float)mid * (-shift_rate) * 2;
	p.startbin = (int32_t)sb;
	p.startbin = (int32_t)(p.v * std::round((double)(p.startbin / (float)p.v)));
	p.offsetbin = p.startbin - mid;
	p.post_shift = p.pre * (shift_rate + ((float)p.offsetbin / p.n));
	p.pre_shift = p.offsetbin / (float)p.n;
	float r = p.post_shift * p.post;
	r *= 2;
	p.sindelta = (float)std::sin(r * M_PI);
	p.cosdelta = (float)std::cos(r * M_PI);
	p.rate = r;
	p.scrap = p.overlap / p.pre;
	p.post_input_size = p.m - p.scrap;
	return p.n > 2;
}

inline float hamming_w(float rate)
{
	rate = (float)(0.5 + rate / 2);
	return (float)(0.54 - 0.46 * std::cos(2 * M_PI * rate));
}

// windowed-sinc low-pass, sum-normalised (fp32 running sum as in the reference)
inline void design_lowpass(std::vector<float> &h, int32_t length, float cutoff)
{
	h.assign((size_t)length, 0.f);
	const int32_t mid = length / 2;
	h[mid] = (float)(2 * M_PI * cutoff * hamming_w(0));
	for (int32_t i = 1; i <= mid; i++) {
		float t = (float)((std::sin(2 * M_PI * cutoff * i) / i) * hamming_w((float)i / mid));
		h[mid - i] = t; h[mid + i] = t;
	}
	float sum = 0;
	for (int32_t i = 0; i < length; i++) sum += h[i];
	for (int32_t i = 0; i < length; i++) h[i] = h[i] / sum;
}

// complex band-pass taps of one channel: low-pass x e^{j theta_n}, theta accumulated in fp32 and wrapped to [0, 2 pi]
inline void design_bandpass(std::complex<float> *out, int32_t length, float lowcut, float highcut, std::vector<float> &lp_cache,
		float &lp_cache_cutoff)
{
	const float cutoff = (highcut - lowcut) / 2;
	if (lp_cache.size() != (size_t)length || lp_cache_cutoff != cutoff) {
		design_lowpass(lp_cache, length, cutoff);
		lp_cache_cutoff = cutoff;
	}
	const float center = (highcut + lowcut) / 2;
	float phase = 0;
	for (int32_t i = 0; i < length; i++) {
		float c = (float)std::cos((double)phase), s = (float)std::sin((double)phase);
		phase = (float)(phase + 2 * M_PI * center);
		while (phase > 2 * M_PI) phase = (float)(phase - 2 * M_PI);
		while (phase < 0) phase = (float)(phase + 2 * M_PI);
		out[i] = std::complex<float>(c * lp_cache[i], s * lp_cache[i]);
	}
}

// The padded channel layout of a front end of several receivers (hfdl_gpu_frontend_create_multi): the channels of receiver r are the
// global channels chan0 .. chan0 + nch - 1 (receiver-major), and in the filter-tap buffer they take the slots slot0 .. slot0 + nch - 1 of a
// run of `slots` = nch rounded up to a whole group of the tap layout (`group` = 8 for the octet layout, 1 for the plain one): no group of
// slots -- and so no fold workgroup, which takes whole groups -- holds channels of two receivers; the slots past nch carry zero taps.
// Returns the total number of slots (Geometry::nch_pad).
struct RxSpan { int32_t slot0, slots, chan0, nch; };
inline int32_t plan_receiver_slots(const int32_t *nch_per_rx, int32_t nrx, int32_t group, std::vector<RxSpan> &out)
{
	out.assign((size_t)nrx, RxSpan{});
	int32_t slot = 0, chan = 0;
	for (int32_t r = 0; r < nrx; r++) {
		const int32_t n = nch_per_rx[r];
		out[(size_t)r] = RxSpan{ slot, (n + group - 1) / group * group, chan, n };
		slot += out[(size_t)r].slots;
		chan += n;
	}
	return slot;
}
inline int32_t receiver_slot(const RxSpan &r, int32_t channel) { return r.slot0 + (channel - r.chan0); }

// The fold's workgroup tables (the octet layout; kernels.h Geometry::grp_tab): for every workgroup width pw = 1 .. pw_max octets, at
// (pw - 1) * noct, the full groups of pw octets of every receiver, receiver after receiver, then the octets each receiver has left over
// -- the order the fold launchers hand them out in.  An entry: first octet, receiver, end of the receiver's channel slots, channel - slot.
struct FoldGroup { int32_t octet, rx, slot_end, to_chan; };
inline std::vector<FoldGroup> fold_group_tables(const std::vector<RxSpan> &rx, int32_t noct, int32_t pw_max)
{
	std::vector<FoldGroup> t((size_t)pw_max * (size_t)noct, FoldGroup{});
	for (int32_t pw = 1; pw <= pw_max; pw++) {
		FoldGroup *e = t.data() + (size_t)(pw - 1) * (size_t)noct;
		for (int rest = 0; rest < 2; rest++)
			for (size_t r = 0; r < rx.size(); r++) {
				const int32_t no = rx[r].slots / 8, first = rx[r].slot0 / 8;
				const FoldGroup v{ 0, (int32_t)r, rx[r].slot0 + rx[r].nch, rx[r].chan0 - rx[r].slot0 };
				if (!rest) for (int32_t gi = 0; gi < no / pw; gi++) { *e = v; e->octet = first + gi * pw; e++; }
				else for (int32_t o = no / pw * pw; o < no; o++) { *e = v; e->octet = first + o; e++; }
			}
	}
	return t;
}

// ---------------------------------------------------------------- create-time batching and slicing rules

// Slices of alias rows per (channel group, bin group): each slice is a workgroup of its own and leaves a partial sum that the inverse
// FFT adds up.  A CU holds ONE matrix-pipe fold workgroup at a time (one 384 / 420-register wave per SIMD), so every workgroup
// generation pays its dispatch, its first loads and its stores with an idle matrix pipe: as few and as long-lived workgroups as fill
// the chip.  256 channels need no slicing (cfg3: 2048 workgroups of 512 quads at one slice; against round 1's rule of
// channels x slices >= 1024 -- four slices -- the 32-block fold takes 5.7 instead of 6.8 ms alone, 0.203 instead of 0.22 ms per block
// in the pipeline, and a quarter of the partial sums are written and read back: profiles/r06_experiments.md); fewer channels are
// sliced until channels x slices >= 256, a slice keeping at least 8 alias rows.
inline int pick_slices(int nch, int rows)
{
	int s = 1;
	while (s * 2 <= rows / 8 && nch * s < 256) s *= 2;
	return s;
}

// What the environment (the shim reads it; include/hfdl_gpu.h documents the names) and the laboratory build ask for; 0 / false = not asked
struct BatchOverrides {
	int demod_batch = 0;        // HFDL_GPU_DEMOD_BATCH 1..32: taken as it is
	int fold_batch = 0;         // HFDL_GPU_FOLD_BATCH 1..32
	bool pruned = false;        // HFDL_GPU_FOLD_PRUNE: one slice, the row windows are the parallelism
	int fold_slices = 0;        // laboratory A/B: slices of alias rows per channel and bin (a power of two; a slice keeps at least 16 rows)
	bool no_ramp = false;       // laboratory A/B: every half the full size from the start
};

struct BatchPlan {
	int slices;                 // Geometry::slices
	int fold_nb;                // blocks per fold launch
	int batch_want;             // blocks per demodulator launch to ask Demod::init for (what it keeps is demod_fit(batch_want))
	int half_blocks;            // slots per half: a multiple of fold_nb, at least the demodulator batch
	int half_first;             // blocks that close the first half after a drain
	int n_stage;                // staging buffers for host input
};

constexpr int PLAN_MAX_HALF = 32;       // blocks per half at most: what one fold launch can take (kernels.h FOLD_MAX_BLOCKS)
constexpr int PLAN_MAX_STAGE = 18;      // staging buffers at most: uploads run at most 17 blocks ahead (HFDL_GPU_PREFETCH_MAX + 1)

// n / input_size / pre: the block geometry (Plan).  fold_bound: the fold bounds the block (128 channels and more).  demod_fit(want):
// blocks a demodulator launch can take, `want` or fewer (Demod::fit_batch: the block table, 16-bit output counts).
template <typename Fit>
inline BatchPlan plan_batches(int nch, int nrx, int n, int input_size, int sample_rate, int pre, bool fold_bound, Fit demod_fit, const BatchOverrides &ov)
{
	BatchPlan b{};
	b.slices = pick_slices(nch, pre);
	if (ov.fold_slices > 0 && (ov.fold_slices & (ov.fold_slices - 1)) == 0 && pre % ov.fold_slices == 0 && pre / ov.fold_slices >= 16) b.slices = ov.fold_slices;
	if (ov.pruned) b.slices = 1;

	// Blocks per fold launch.  The filter taps are 99.9 % of a block's bytes on the fold-bound geometries (cfg3: 16 GiB of taps against
	// a 64 MiB spectrum) and they are the same for every block: when blocks are pushed faster than they are collected (file replay,
	// catching up, the bench) the spectra of up to `fold_nb` consecutive blocks are folded in ONE pass over the taps on the matrix pipe
	// (fold_kernels.hip).  Every block's sums are bit-identical to a launch of its own (fixed FMA chain per bin); a caller that polls
	// or syncs after every block (live input) still gets one launch per block: a sync / poll closes the half as it is.
	// 32 where the fold bounds the block (128 channels and more): two column groups of the sixteen-column matrix instruction per loaded tap
	// operand.  A launch costs about its matrix time plus its memory time (fold_kernels.hip, profiles/r06_experiments.md), so a block's share
	// shrinks with the blocks per byte of taps: 0.20 ms per block at 32 against 0.245 at 16 in the pipeline.  The
	// first half after a drain closes at 16 (half_first).  Where the demodulator bounds the block (fewer than 128 channels: the taps are a
	// few hundred MiB and a fold launch takes 0.2 ms whatever it folds) a long half only adds fill, drain and latency: 8, as in round 4
	// (cfg2: 0.1545 against 0.1595 ms per block over 256 blocks)
	b.fold_nb = ov.fold_batch ? ov.fold_batch : (fold_bound ? 32 : 8);      // 1 = a pass over the taps per block

	// Blocks per demodulator launch.  Every launch pays fixed costs: the barrier packet in front of it (~11 us), ~25 KiB of tables and
	// state staged into LDS and written back, and two chunks of pipeline fill and drain -- ~40 us against ~210 us of recurrence per
	// cfg2 block.  When blocks arrive faster than they are demodulated (file replay, catching up) consecutive blocks are therefore handed
	// to ONE launch, which treats them as one longer stretch of samples -- the per-channel state is carried sample by sample, so the
	// result is that of block-by-block processing.  A caller that waits for its PDUs after every block (live input: poll / sync) still
	// gets a launch per block: a partial batch is launched by any call that needs the results.  Bounds (Demod::fit_batch): the kernel's
	// block table (a whole half) and output counts that fit 16 bits.  Neither the LDS (a workgroup's per-sample arrays are rings,
	// demod_lds.h) nor the frames a channel finishes in a launch bound it: the frame queue and the channels' data slots are sized from
	// the launch's signal time (plan_frame_slots below).
	// A half that closes full is one launch: the larger of a second's worth of blocks (at most 8) and the fold's launch.
	int want = (int)std::floor(1.0 / ((double)input_size / (double)sample_rate));
	want = std::max(1, std::min(8, want));
	want = std::max(want, b.fold_nb);
	if (ov.demod_batch) want = ov.demod_batch;                              // 1 = a launch per block
	want = demod_fit(want);
	if (nrx > 1) {
		// The per-block buffers of the forward FFT scale with the receivers (spectra: two sets x half x K x N cf32; staging ring, overlap
		// history, work): a half holds at most 32 x 2^23 / (K N) blocks -- the single-receiver cfg3 footprint (32 blocks of 2^23 bins),
		// known to fit.  Where that binds, the fold batch (and with it the half and the staging ring) shrinks, never below one block, and
		// the demodulator batch is clamped to the half.
		const int64_t cap = std::max<int64_t>(1, ((int64_t)32 << 23) / ((int64_t)nrx * (int64_t)n));
		if (cap < std::max(b.fold_nb, want)) {
			b.fold_nb = (int)std::min<int64_t>(b.fold_nb, cap);
			want = std::min(want, b.fold_nb);
		}
	}
	if (!ov.demod_batch && want < b.fold_nb) {
		// even launches: a half of 8 blocks at up to 7 per launch is two launches of 4, not 7 + 1 (cfg2: 5.5 against 5.8 Gsamples/s); an
		// explicit HFDL_GPU_DEMOD_BATCH is taken as it is
		const int launches = (b.fold_nb + want - 1) / want;
		want = (b.fold_nb + launches - 1) / launches;
	}
	b.batch_want = want;
	const int batch = demod_fit(want);
	b.half_blocks = std::min(PLAN_MAX_HALF, ((std::max(b.fold_nb, batch) + b.fold_nb - 1) / b.fold_nb) * b.fold_nb);
	// A pipeline that starts empty closes its first half at 16 blocks where a half holds 32: the first fold launch is the sixteen-column
	// form and the demodulators start 3 ms earlier (the front end's half_target)
	b.half_first = (fold_bound && b.half_blocks > 16 && !ov.no_ramp) ? 16 : b.half_blocks;
	b.n_stage = std::min(b.half_blocks + 2, PLAN_MAX_STAGE);      // a 32-block half is not uploaded a whole half ahead: 17 blocks of link time cover a 6 ms fold five times over
	return b;
}

// ---------------------------------------------------------------- what a demodulator launch can take

// 5400-sps samples a launch of `batch` blocks produces at most: `outs` channelizer samples per block and channel at most, resampled by `rate`
inline int demod_launch_samples(int outs, int batch, float rate) { return (int)((double)outs * (double)batch * (double)rate + 8); }
// Blocks a launch can take, `want` or fewer, by the block table (a whole half) and the output counts: the timing recovery yields at most two
// outputs per sample in the long run, and the running count of a launch's outputs is kept in 16 bits per sample in LDS (demod_lds.h cum[]).
// cfg3's 32 blocks fit (2 x 31 734); a geometry whose half holds more than 6 s of signal is cut.
inline int fit_output_counts(int outs, float rate, int want)
{
	int batch = std::max(1, std::min(PLAN_MAX_HALF, want));
	while (batch > 1 && 2 * demod_launch_samples(outs, batch, rate) > 65535) batch--;
	return batch;
}

// ---------------------------------------------------------------- frames a launch can finish, and how long their symbols must stay

// A demodulator launch covers up to t_launch seconds of signal (T_L) and can finish several frames of one channel.  The frames of
// launch i are queued in the frame queue of set i & 1 and decoded by the burst decoder of launch i, which reads their data symbols from
// the channel's ring of data slots: a finished frame keeps its slot, the next frame takes the next one.
//   T_F  the shortest distance between two frame ends of a channel.  The framer finds a frame by its A sequences and needs no prekey:
//        2 A + M1 + M2 + nine T + 72 data segments = 3771 symbols at 1800 Bd, 2.095 s (a frame on the air, prekey included, lasts 2.344 s).
//   F    frame records per channel and set: ends at least T_F apart, so at most floor(T_L / T_F) + 1 of them lie in one launch.
//   S    data slots per channel.  The slot of a frame that ended in launch i is written again by the S-th frame after it, whose data
//        follow the end of the (S - 1)-th: at least (S - 1) T_F later.  The burst decoder of launch i is only known to be done when the
//        demodulator of launch i + 2 starts (DemodOrder below, hazard 1: the wait goes there and nowhere earlier), so the write must not fall
//        into launch i or i + 1: those cover less than 2 T_L of signal behind the frame's end.  (S - 1) T_F >= 2 T_L holds with
//        S = floor(2 T_L / T_F) + 2; one slot fewer and a frame that ends at the start of launch i loses its symbols to a frame of
//        launch i + 1 (tests/hostsim/frame_slots_check.cpp steps both).
// One second of signal per launch gives F = 1 and S = 2, a 32-block launch of cfg3 (5.9 s) F = 3 and S = 7 (72 MB of symbols).
constexpr double PLAN_MIN_FRAME_S = 3771.0 / 1800.0;
struct FrameSlots { int per_channel, data_slots; };       // F, S
inline FrameSlots plan_frame_slots(double t_launch, double t_frame = PLAN_MIN_FRAME_S)
{
	return FrameSlots{ (int)std::floor(t_launch / t_frame) + 1, (int)std::floor(2.0 * t_launch / t_frame) + 2 };
}

// ---------------------------------------------------------------- which stream a block's forward FFT runs on

// A block's forward FFT runs either SERIAL -- on stream A, in front of the fold of its own half and behind the fold of the half before --
// or BESIDE: on the input stream (stream C; the laboratory's stream F), while stream A folds the half before.  The forward FFT is
// HBM-bound and the fold bound on the matrix pipe, so a block that is already in HBM goes beside; a block that was uploaded keeps its FFT
// on stream A, where the staging ring and the demodulator hold-back are tuned for it (a copy stream busy with kernels would put the
// uploads behind them).  Chosen per push.  The laboratory build can put every FFT on one side (HFDL_GPU_FFT_STREAM).
enum FftSide { FFT_SERIAL = 0, FFT_BESIDE = 1 };
enum FftRule { FFT_RULE_INPUT, FFT_RULE_SERIAL, FFT_RULE_OWN };     // by where the block lies / all on stream A / all on stream F
inline int fft_side(FftRule rule, bool on_device) { return rule == FFT_RULE_INPUT ? (on_device ? FFT_BESIDE : FFT_SERIAL) : rule == FFT_RULE_OWN ? FFT_BESIDE : FFT_SERIAL; }

// What the launch of one forward FFT has to do besides the launch, and what the closing of a half has to.  The forward FFTs form a chain
// (overlap history, work buffer, NCO state) and share two sets of spectra / phasor tables / snapshots with the fold and inverse FFT:
//   - consecutive FFTs on one stream are ordered by it; an FFT on the other stream than the one before first waits for everything queued
//     on that stream so far (wait_switch)
//   - the first FFT of a half, BESIDE: its set was last read by the fold and inverse FFT two halves ago, on stream A (wait_set_free);
//     SERIAL, stream A orders it
//   - the first fold after a drain runs alone, with everything behind it waiting for it: forward FFTs beside it would only slow it down
//     (20 blocks into an idle pipeline: 16 + 4, and the four blocks' FFTs took 0.2 ms out of the fold of the sixteen).  The first FFT of the
//     SECOND half since a drain, BESIDE, therefore waits for the inverse FFT of the first (wait_first_fold) -- where it would be on stream A
//   - the fold of a half waits for the newest BESIDE FFT of that half, if there is one (HalfClosePlan::wait_input)
//   - held-back demodulators (fold-bound geometries, launch_demod): a half's launches are held back only if its newest FFT ran SERIAL --
//     the next half is then expected in front of the fold as well -- and go behind the LAST serial FFT of the next half, which carries the
//     event they wait for (hold_after).  A BESIDE FFT carries no such event: it launches what is held back at once, in front of
//     itself (flush_before), so that nothing ever waits for an event no launch will signal
//   - a retune (hfdl_gpu_frontend_retune_channel) closes the half being filled, which puts stream A behind every forward FFT queued so
//     far wherever it ran (the fold of a half follows its FFTs), and then rewrites one channel's constants and carried NCO state on
//     stream A: the first FFT after it, BESIDE, waits for the event that kernel carries (wait_retune); SERIAL, stream A orders it, and
//     a later BESIDE one then finds it behind wait_switch
struct FftPushPlan { int side; bool wait_switch, wait_set_free, wait_first_fold, flush_before, hold_after, wait_retune; };
struct HalfClosePlan { bool wait_input, hold_back; };
struct FftOrder {
	int prev_side = -1;             // side of the newest forward FFT; -1: none since everything queued was waited for
	bool half_beside = false;       // an FFT of the half being filled ran BESIDE
	int halves = 0;                 // halves closed since everything queued was waited for
	bool retuned = false;           // a retune's kernel is queued on stream A and no forward FFT has been ordered behind it yet
	// fill: blocks already in the half being filled, target: blocks that close it, held_back: the half before waits for its demodulators
	FftPushPlan push(int side, int fill, int target, bool held_back)
	{
		FftPushPlan p{};
		p.side = side;
		p.wait_switch = prev_side >= 0 && prev_side != side;
		p.wait_set_free = side == FFT_BESIDE && fill == 0;
		p.wait_first_fold = side == FFT_BESIDE && fill == 0 && halves == 1;
		p.flush_before = side == FFT_BESIDE && held_back;
		p.hold_after = side == FFT_SERIAL && held_back && fill + 1 == target;
		p.wait_retune = side == FFT_BESIDE && retuned;
		retuned = false;
		prev_side = side;
		half_beside = half_beside || side == FFT_BESIDE;
		return p;
	}
	// a half of at least one block is closed; launch_now: the caller wants its demodulators at once (a sync / poll, a demodulator-bound geometry)
	HalfClosePlan close(bool launch_now)
	{
		const HalfClosePlan c{ half_beside, !launch_now && prev_side == FFT_SERIAL };
		half_beside = false;
		halves++;
		return c;
	}
	void retune() { retuned = true; }                   // the half being filled has been closed (close()) and the retune's kernel queued
	void drained() { prev_side = -1; halves = 0; retuned = false; }      // every stream has been synchronised
};

// ---------------------------------------------------------------- a closed half's way through demodulator and burst decoder

// A half handed to the demodulator is taken in k launches of up to `batch` blocks, numbered i = 0, 1, .. over the front end's life; each
// is a demodulator kernel on stream B and then its burst decoder, with the 16-byte snapshot of the PDU ring's counts behind it, on
// stream D (a stream of their own; in a laboratory A/B run D is B).  The frames the demodulator of launch i finishes are queued in frame
// queue set i mod 2 and counted in frame counter i mod 4; the decoder of launch i reads both and zeroes the counter of launch i + 2,
// whose users before (launch i - 2) are done -- no memset launch per block, no counter shared by two kernels that can overlap.  The
// snapshot goes to the slot of the launch's HALF (0 / 1).  The contract -- four hazards, none of which may lose a frame or a PDU or
// show one half-written:
//   1. the demodulator of launch i does not start before the decoder of launch i - 2 is done: it reuses that decoder's frame queue, and
//      that decoder zeroes its counter.  D = B: stream order.  Else launch i carries the wait on stream B in front of its kernel
//      (wait_decoder) -- unless it is a half's first launch and stream A has taken the wait in front of the half's inverse FFT
//      (wait_on_a(): where the demodulator bounds the block stream A has the slack and B then needs ONE barrier packet between
//      consecutive demodulators; the front end decides when, Demod remembers that it did).  So "the decoder of launch i is done" is
//      established no later than the start of the demodulator of launch i + 2, and nowhere earlier: plan_frame_slots above rests on it
//   2. the decoder of launch i waits for the demodulator of launch i: for the done event the launch carries, unless D = B
//   3. the inverse FFT into a half waits for the last demodulator launch that read that half: the half's done event 0 -- the launches
//      of a half carry its done events k - 1 .. 0 (done_event), the LAST one event 0, however many there are
//   4. a poll that leaves the pipeline running (hfdl_gpu_frontend_poll_pdus_ready) waits for, or asks after, the last DEMODULATOR of
//      the half before the newest (poll_half) and reads a snapshot slot only when the decoders that write it are done: that half's own
//      slot if its last decoder is found done too; else the slot of the half before THAT, if its last decoder is found done and the
//      slot is another one -- the newest half's decoders, which write it next, sit behind the unfinished one on their stream; else
//      none (snapshot_slot).  The demodulator the poll waited for says nothing about the decoder of the launch before it (hazard 1
//      reaches two launches back), and with one launch per half that is the half whose slot is read: so it is asked after.  A half's
//      last decoder carries one of three events in turn (decoded_event): the newest half's record leaves the two before it alone
// tests/hostsim/demod_order_check.cpp runs the rule inside a front end reduced to launches and waits over every short call sequence.
struct DemodLaunch { int set, counter, zeroed; bool wait_decoder; int done_event; };
struct DemodOrder {
	uint64_t launches = 0;          // demodulator launches so far = the index of the next one (channelize-only blocks launch none)
	bool own_decode = false;        // the burst decoders have a stream of their own
	bool waited_on_a = false;       // stream A has taken the next launch's wait for the decoder of two launches ago
	uint64_t halves = 0;            // halves handed to the demodulator so far (launched or held back)
	int newest = -1, before = -1, before2 = -1;     // the newest of them, the one before it and the one before that (0 / 1; -1: none)
	void hand_over(int half) { before2 = before; before = newest; newest = half; halves++; }
	int decoded_event(int back) const { return halves > (uint64_t)back ? (int)((halves - 1 - (uint64_t)back) % 3) : -1; }     // of the newest half (0), the one before (1), before that (2); -1: none
	int next_set() const { return (int)(launches & 1); }        // the decoder whose event wait_on_a() is about
	// stream A takes the next launch's wait (own_decode only); false: there is no such decoder yet, nothing to wait for
	bool wait_on_a() { waited_on_a = true; return launches >= 2; }
	// launch l of the k a half is taken in
	DemodLaunch launch(int l, int k)
	{
		const uint64_t i = launches++;
		const DemodLaunch p{ (int)(i & 1), (int)(i & 3), (int)((i + 2) & 3), own_decode && i >= 2 && !(l == 0 && waited_on_a), k - 1 - l };
		waited_on_a = false;
		return p;
	}
	int poll_half() const { return before; }                    // -1: fewer than two halves, nothing is known to be done
	// the slot a poll reads: the last decoder of poll_half() found done / not, that of the half before it found done / not; -1: none
	// (a channelize-only half in between gives consecutive halves the same slot: the newer one's decoders may be writing it)
	int snapshot_slot(bool decoded, bool older_decoded) const
	{
		const int older = before2 >= 0 && before2 != before ? before2 : -1;
		return decoded ? (before != newest ? before : older) : older_decoded ? older : -1;
	}
};

// ---------------------------------------------------------------- the CU partition of the fold-bound geometries

// Where the fold bounds the block, the demodulator's latency-bound waves and the fold's matrix waves are kept off each other's SIMDs:
// an fp32 matrix instruction holds a SIMD's vector issue while it runs, and beside a stream of them a demodulator wave takes 3.4 - 4.3 x
// its cycles.  The demodulator's stream (B) gets ceil(channels / workgroups per CU) CUs, rounded up to an equal
// share of every XCD; the channelizer's streams (A, F) get the rest.  A device of PLAN_CUS CUs in PLAN_XCDS XCDs; a CU mask counts
// them either XCD-major (CU i in XCD i / 32) or XCD-interleaved (XCD i % 8): seen as 32 rows of 8, an XCD is a band of four rows in one
// numbering and a column in the other.  Cell q of band m is row 4 m + q % 4, column (m + q % 4 + 2 (q / 4)) % 8: the cells of a band are
// distinct, and over the eight bands every (q % 4, q / 4) lands in every column once -- `per_xcd` CUs in every band and in every column.
constexpr int PLAN_CUS = 256, PLAN_XCDS = 8, PLAN_CU_LDS = 160 * 1024;
constexpr int PLAN_DEMOD_WG_PER_CU = 4;     // at most: a demodulator workgroup puts one wave on every SIMD, its register budget is a fifth of a SIMD's
struct CuPartition {
	bool on = false;
	int wg_per_cu = 0, demod_cus = 0;
	uint32_t mask_fold[PLAN_CUS / 32] = {}, mask_demod[PLAN_CUS / 32] = {};
};
inline CuPartition plan_cu_partition(int nch, size_t demod_lds, bool fold_bound)
{
	CuPartition p;
	if (!fold_bound || nch < 1 || demod_lds == 0 || demod_lds > (size_t)PLAN_CU_LDS) return p;
	p.wg_per_cu = std::min<int>(PLAN_DEMOD_WG_PER_CU, (int)((size_t)PLAN_CU_LDS / demod_lds));
	const int cus = (nch + p.wg_per_cu - 1) / p.wg_per_cu, per_xcd = (cus + PLAN_XCDS - 1) / PLAN_XCDS;
	if (per_xcd > PLAN_CUS / PLAN_XCDS / 2) return p;        // more than half the device: the channels run beside the fold as they are
	for (int m = 0; m < PLAN_XCDS; m++)
		for (int q = 0; q < per_xcd; q++) {
			const int i = (4 * m + (q & 3)) * 8 + ((m + (q & 3) + 2 * (q >> 2)) & 7);
			p.mask_demod[i >> 5] |= 1u << (i & 31);
		}
	for (int w = 0; w < PLAN_CUS / 32; w++) p.mask_fold[w] = ~p.mask_demod[w];
	p.demod_cus = per_xcd * PLAN_XCDS;
	p.on = true;
	return p;
}

// ---------------------------------------------------------------- the pruned fold's row windows (HFDL_GPU_FOLD_PRUNE = tolerance)

// A channel's filter is a band-pass M / 2 bins wide with a Hamming-window stop band: of the p = N / M alias rows the fold adds up, all
// but the few around the pass band hold taps below fp32 resolution of the sum (cfg3: rows 32 or more from the pass band hold 3.7e-8 of
// the filter's energy as an amplitude ratio -- less than half an ulp).  From the taps' energy per (row, slot),
// en[r * npad + c]: per channel the smallest window of rows around the pass band outside which less than tol^2 of the filter's energy
// lies; the workgroup of an octet folds the circular hull of its eight channels' windows in quads of rows (what one matrix instruction
// takes), rounded up to whole look-ahead groups of two quads.  Returns per octet { first quad, count } (slots nch .. npad - 1 only fill
// an octet up) and, in *rows_max, the longest window in rows.
struct RowWindow { int32_t first, count; };
inline std::vector<RowWindow> fold_row_windows(const std::vector<float> &en, int p, int npad, int nch, double tol, int *rows_max)
{
	// per channel: the window grows from the row that holds the most energy, towards the richer neighbour, until the rows outside
	// hold less than tol^2 of the total (rows picked by energy alone would scatter: the fp32 transform that made the taps left its
	// rounding noise in every row, and the largest noise rows lie anywhere)
	std::vector<std::vector<char>> keep((size_t)npad, std::vector<char>((size_t)p, 0));
	for (int c = 0; c < nch; c++) {
		double tot = 0;
		int peak = 0;
		for (int r = 0; r < p; r++) { tot += en[(size_t)r * npad + c]; if (en[(size_t)r * npad + c] > en[(size_t)peak * npad + c]) peak = r; }
		auto e_at = [&](int r) { return (double)en[(size_t)((r % p + p) % p) * npad + c]; };
		int lo = peak, hi = peak;                         // window [lo, hi], indices unwrapped
		double left = tot - e_at(peak);
		while (hi - lo + 1 < p && left > tol * tol * tot) {
			if (e_at(lo - 1) > e_at(hi + 1)) left -= e_at(--lo); else left -= e_at(++hi);
		}
		for (int r = lo; r <= hi; r++) keep[(size_t)c][(size_t)((r % p + p) % p)] = 1;
	}
	auto hull = [&](int c0, int c1) {                   // circular hull of the rows kept by channels [c0, c1), in QUADS of rows (first quad, count)
		const int nq = p / 4;
		std::vector<char> any((size_t)nq, 0);
		int kept = 0;
		for (int c = c0; c < c1; c++) for (int r = 0; r < p; r++) if (keep[(size_t)c][(size_t)r] && !any[(size_t)(r >> 2)]) { any[(size_t)(r >> 2)] = 1; kept++; }
		if (kept == 0) return RowWindow{ 0, 2 };         // channels that only fill the octet up: zero taps, any two quads
		int best_len = 0, best_end = 0;                  // the longest circular run of quads nobody keeps
		for (int q = 0; q < nq; q++) {
			if (any[(size_t)q] || !any[(size_t)((q + nq - 1) % nq)]) continue;      // q = first quad of a gap
			int len = 0;
			while (len < nq && !any[(size_t)((q + len) % nq)]) len++;
			if (len > best_len) { best_len = len; best_end = (q + len) % nq; }
		}
		int count = nq - best_len;
		count = std::min(nq, (count + 1) & ~1);          // whole look-ahead groups of two quads
		return RowWindow{ best_len ? best_end : 0, count };
	};
	std::vector<RowWindow> w((size_t)(npad / 8));
	*rows_max = 0;
	for (size_t i = 0; i < w.size(); i++) { w[i] = hull(8 * (int)i, 8 * (int)i + 8); *rows_max = std::max(*rows_max, 4 * w[i].count); }
	return w;
}

}  // namespace hfdl
