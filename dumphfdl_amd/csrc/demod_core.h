// demod_core.h -- per-channel HFDL demodulator, one block of channelizer output per call (gfx950, device only).
//
// Replaces the body of hfdl_decoder_thread after fastddc_inv_cc (reference src/hfdl.c:676-892):
// msresamp -> AGC -> matched filter -> symsync -> Costas -> LMS equaliser -> M-PSK slicer -> preamble
// correlator / framer.
//
// Mapping: ONE WORKGROUP OF FOUR WAVEFRONTS PER CHANNEL, the waves forming a software pipeline over chunks of DM_CHUNK
// 5400-sps samples.  The reference runs these stages as one serial loop; three of them are genuine recurrences (the AGC gain,
// the symbol-timing loop, the carrier loop + equaliser + framer FSM) and each costs a lone wavefront a few hundred cycles per
// sample in dependent-instruction latency.  They only feed FORWARD -- resampler -> AGC -> timing recovery -> carrier/equaliser/framer --
// with one rare exception, so they run concurrently on the four SIMDs of the CU (WAVE_RESAMPLER, WAVE_AGC, WAVE_TIMING, WAVE_CARRIER):
//
//   wave 3   arbitrary resampler (msresamp_crcf_execute; no recurrence: a lane per output) of chunk s+1, and the channelizer samples
//            of chunk s+3 fetched from HBM into an LDS ring
//   wave 0   AGC recurrence (agc_crcf_execute) + matched filter (lanes over outputs) of chunk s
//   wave 1   symsync_crcf of chunk s-1: every output gathers its 18-tap windows from LDS, four dot products per DPP row reduction
//   wave 2   Costas loop, equaliser, slicer, framer FSM of chunk s-2 (demod_logic.h on_symbol)
//
// Every per-sample array the waves hand on is a power-of-two ring indexed by the sample's index in the launch (demod_lds.h): the LDS a
// workgroup takes does not depend on the launch's length.  A wave is held back when it would overwrite what a later stage -- or a
// restart of the timing recovery -- can still read; all distances are measured from wave 2's progress.
//
// The exception: the framer resets the timing loop (symsync_crcf_reset at the end of a frame, on a failed preamble search,
// on carrier run-away: src/hfdl.c:714,751,969).  Wave 1 therefore runs AHEAD speculatively; when wave 2 hits a reset at
// sample k it publishes k, and wave 1 restarts at k+1 from the reset state, which is fully determined (empty matched-filter
// window, the last 18 matched-filter samples in the derivative window, initial loop scalars).  Results are those of the
// serial order, sample for sample; resets are rare (once per frame), so the re-run costs nothing measurable.
// The waves meet at one workgroup barrier per chunk and exchange progress through a double-buffered LDS mailbox (demod_lds.h PipeMail):
// in a step every wave works on what the mailbox of the step before allowed it, lane 0 publishes how far it got, and after the barrier
// all four read the same PipeProgress.
#pragma once
#include <hip/hip_runtime.h>
#include "demod_logic.h"
#include "demod_lds.h"

namespace hfdl {

constexpr int DM_WAVES = 4, DM_THREADS = 64 * DM_WAVES;      // (chunk and ring sizes: demod_lds.h)
constexpr int WAVE_AGC = 0, WAVE_TIMING = 1, WAVE_CARRIER = 2, WAVE_RESAMPLER = 3;      // the pipeline's stages by wave: the order of PipeMail::busy[]

// ---- DPP helpers (GFX9 encodings): all row-local, a row = 16 lanes ----
__device__ __forceinline__ float dpp_row_shr1(float old, float src)      // lane i <- src[i-1]; lane 0 of every row <- old
{
	return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(src), 0x111, 0xf, 0xf, false));
}
__device__ __forceinline__ float dpp_row_shl1(float old, float src)      // lane i <- src[i+1]; lane 15 of every row <- old
{
	return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(src), 0x101, 0xf, 0xf, false));
}
__device__ __forceinline__ float dpp_row_shl2(float old, float src)      // lane i <- src[i+2]; lanes 14, 15 of every row <- old
{
	return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(src), 0x102, 0xf, 0xf, false));
}
__device__ __forceinline__ float dpp_row_ror1(float src)                 // lane i <- src[i-1], lane 0 <- src[15] (inside the row)
{
	return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(src), 0x121, 0xf, 0xf, false));
}
// inclusive scan-sum inside every 16-lane row (lanes shifted in from outside the row read 0): lane 15 of a row ends up
// with the row's total.  One call reduces FOUR independent 16-term sums, one per row.
__device__ __forceinline__ float row_scan_sum(float v)
{
	int x = __float_as_int(v);
	x = __float_as_int(__int_as_float(x) + __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, true)));
	x = __float_as_int(__int_as_float(x) + __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, true)));
	x = __float_as_int(__int_as_float(x) + __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, true)));
	x = __float_as_int(__int_as_float(x) + __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, true)));
	return __int_as_float(x);
}
// inclusive scan-max inside every 16-lane row (lanes shifted in from outside the row read 0, so the result is max(0, ...)).
// v_max_f32 with the DPP operand, one instruction per step: written through the compiler's fmaxf each step is a DPP move, a
// canonicalising v_max x, x and the max itself.  (s_nop 1: the two wait states between a VALU write and a DPP read of the register.)
__device__ __forceinline__ float row_scan_max(float v)
{
	asm volatile("s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
			"s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
			"s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
			"s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\ts_nop 0"
			: "+v"(v));
	return v;
}
// x / 3.0f, correctly rounded, without the IEEE division sequence (12 instructions on the timing loop's output path): reciprocal
// multiply plus one FMA residual correction (Markstein); checked against true division over 6e4 random floats
__device__ __forceinline__ float div3(float x)
{
	const float c = 0x1.555556p-2f;
	const float q = x * c;
	return __builtin_fmaf(__builtin_fmaf(-3.0f, q, x), c, q);
}
__device__ __forceinline__ float lane_value(float v, int lane)           // wave-uniform copy of one lane (lane is uniform)
{
	return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// what the four waves share through LDS besides the sample rings
struct DemodShared {
	cf *outq;                      // symsync outputs of the launch, in order: output j at outq[j & (OUTQ_RING - 1)]
	int outq_cap;                  // outputs a launch may produce at most (the 16-bit counts of cum[]); beyond it they are dropped
	uint16_t *cum;                 // cum[k & DM_MASK] = outputs produced up to and including input sample k
	const float2 *sstab;           // [16 banks][64 lanes] {tap t, tap t+16} of the lane's row: rows 0,1 matched filter, rows 2,3 derivative
	ChanScalars *S;                // the channel's scalars; every wave owns a disjoint set of fields
	PipeMail *mbox;                // [2] progress mailbox, written in turn: step s uses mbox[s & 1]
	float *sink;                   // [64] write-only scratch, one word per lane
	cf *stage;                     // [64] the carrier wave's data symbols of one chunk (a chunk has at most 64 outputs)
};

// The mailbox of a step: mbox[step & 1], its offset worked out in ints.
__device__ __forceinline__ PipeMail &step_mail(PipeMail *mbox, int step)
{
	return *(PipeMail *)((int *)mbox + (int)(sizeof(PipeMail) / sizeof(int)) * (step & 1));
}

// ---------------- experiment builds: -DHFDL_DM_PROBE=2 .. 6 (profiles/probe_states.py, profiles/wave_cycles.py) ----------------
// Counters reported in the phase-cycle slots of the level tap, from PHASE_AHEAD on, over what the product puts there:
//   = 2  the carrier wave's cycles per framer state -- searching, equaliser training, data -- in three slots;  = 3  its outputs, likewise
//   = 4  wave 0's busy cycles (AGC + matched filter), = 5  wave 3's (resampler + input fetch), counted like the product's counters of
//        waves 1 and 2 from the step's start to the mailbox write
//   = 6  the sum over the steps of the longest of waves 0, 1, 2 in that step: what it leaves of the pipelined phase is the barrier and
//        mailbox step itself
// The product defines none of it: both types are empty then, and what demod_block() and carrier_chunk() call compiles to nothing.
#ifdef HFDL_DM_PROBE
struct StateProbe {                // = 2, = 3: per framer state
	unsigned long long search = 0, train = 0, data = 0;
	__device__ __forceinline__ unsigned long long now() const { return __builtin_amdgcn_s_memtime(); }
	__device__ __forceinline__ void iteration(unsigned long long t0, int fr_state)      // a general iteration begun at t0 in fr_state: one output
	{
		const unsigned long long dt = HFDL_DM_PROBE == 2 ? __builtin_amdgcn_s_memtime() - t0 : 1ull;
		if (fr_state == FR_A1) search += dt; else if (fr_state == FR_EQ_TRAIN) train += dt; else if (fr_state == FR_DATA_1 || fr_state == FR_DATA_2) data += dt;
	}
	__device__ __forceinline__ void frame_run(unsigned long long t0, bool training, int n_run)
	{
		const unsigned long long dt = HFDL_DM_PROBE == 2 ? __builtin_amdgcn_s_memtime() - t0 : (unsigned long long)n_run;
		if (training) train += dt; else data += dt;
	}
	__device__ __forceinline__ void search_run(int n_run) { if (HFDL_DM_PROBE == 3) search += (unsigned long long)n_run; }
};
struct StepClock {                 // = 4, 5, 6: per step of the pipeline
	unsigned long long t0 = 0, longest = 0;
	template <int WAVE> static constexpr bool clocks() { return (WAVE == WAVE_AGC && (HFDL_DM_PROBE == 4 || HFDL_DM_PROBE == 6)) || (WAVE == WAVE_RESAMPLER && HFDL_DM_PROBE == 5); }
	template <int WAVE> __device__ __forceinline__ void begin() { if (clocks<WAVE>()) t0 = __builtin_amdgcn_s_memtime(); }
	// behind the wave's mailbox write: into the wave's busy cycles, or (= 6) this step's into the mailbox
	template <int WAVE> __device__ __forceinline__ void end(unsigned long long &busy, PipeMail &mail, int lane) const
	{
		if (!clocks<WAVE>()) return;
		if (HFDL_DM_PROBE != 6) busy += __builtin_amdgcn_s_memtime() - t0;
		else if (lane == 0) mail.busy[WAVE] = (int)(__builtin_amdgcn_s_memtime() - t0);
	}
	// = 6, waves 1 and 2: they clock their steps for the product's counters already, from `since`
	template <int WAVE> __device__ __forceinline__ void end_since(unsigned long long since, PipeMail &mail, int lane) const
	{
		if (HFDL_DM_PROBE == 6 && lane == 0) mail.busy[WAVE] = (int)(__builtin_amdgcn_s_memtime() - since);
	}
	__device__ __forceinline__ void after_barrier(const PipeMail &mail)      // = 6: the step lasted as long as its longest wave
	{
		if (HFDL_DM_PROBE != 6) return;
		const int m01 = mail.busy[WAVE_AGC] > mail.busy[WAVE_TIMING] ? mail.busy[WAVE_AGC] : mail.busy[WAVE_TIMING];
		longest += (unsigned long long)(m01 > mail.busy[WAVE_CARRIER] ? m01 : mail.busy[WAVE_CARRIER]);
	}
	// all threads, behind the product's own phase cycles
	__device__ __forceinline__ void report(float *tap_level, int cap, int wave, int lane, unsigned long long busy, const StateProbe &sp) const
	{
		__syncthreads();
		float *slots = tap_level + phase_slot(cap, PHASE_AHEAD);
		if (HFDL_DM_PROBE == 2 || HFDL_DM_PROBE == 3) {
			if (wave == WAVE_CARRIER && lane == 0) { slots[0] = (float)sp.search; slots[1] = (float)sp.train; slots[2] = (float)sp.data; }
		} else if (HFDL_DM_PROBE == 4 || HFDL_DM_PROBE == 5) {
			if (wave == (HFDL_DM_PROBE == 4 ? WAVE_AGC : WAVE_RESAMPLER) && lane == 0) slots[0] = (float)busy;
		} else if (HFDL_DM_PROBE == 6) {
			if (wave == WAVE_CARRIER && lane == 0) slots[0] = (float)longest;
		}
	}
};
#else
struct StateProbe {
	__device__ __forceinline__ unsigned long long now() const { return 0ull; }
	__device__ __forceinline__ void iteration(unsigned long long, int) {}
	__device__ __forceinline__ void frame_run(unsigned long long, bool, int) {}
	__device__ __forceinline__ void search_run(int) {}
};
struct StepClock {
	template <int WAVE> __device__ __forceinline__ void begin() {}
	template <int WAVE> __device__ __forceinline__ void end(unsigned long long &, PipeMail &, int) const {}
	template <int WAVE> __device__ __forceinline__ void end_since(unsigned long long, PipeMail &, int) const {}
	__device__ __forceinline__ void after_barrier(const PipeMail &) {}
	__device__ __forceinline__ void report(float *, int, int, int, unsigned long long, const StateProbe &) const {}
};
#endif

// ---------------- wave 0: AGC + matched filter of samples [a0, a1) ----------------

template <bool TAPS>
__device__ __forceinline__ void agc_mf_chunk(float &g, float &y2, const DemodConst &T, const BlockIo &io, int a0, int a1, int lane)
{
	// agc_crcf_execute (src/hfdl.c:686): a per-sample gain recurrence, wave-uniform
	const float alpha = AGC_BANDWIDTH;
	const cf xin = (a0 + lane < a1 && lane < DM_CHUNK) ? io.rs[(a0 + lane) & DM_MASK] : cf{0.f, 0.f};      // the chunk, one sample per lane
	for (int k = a0; k < a1; k++) {
		cf x; x.x = lane_value(xin.x, k - a0); x.y = lane_value(xin.y, k - a0);
		cf y; y.x = x.x * g; y.y = x.y * g;
		const float e = y.x * y.x + y.y * y.y;
		y2 = (1.0f - alpha) * y2 + alpha * e;
		// exp(a ln y2) == 2^(a log2 y2): one v_log_f32 + one v_exp_f32 on the gain recurrence's critical path
		if (y2 > 1e-6f) g *= __builtin_amdgcn_exp2f(-0.5f * alpha * __builtin_amdgcn_logf(y2));
		if (g > 1e6f) g = 1e6f;
		io.agc[k & DM_AGC_MASK] = y;
		io.lvl[k & DM_MASK] = __builtin_amdgcn_rcpf(g);
	}
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	// 19-tap matched filter, lanes over the chunk's outputs (firfilt_crcf, src/hfdl.c:694-695).  The AGC ring's entries in front of
	// sample 0 hold the previous launch's last outputs (demod_block put mf_hist there).
	const int k = a0 + lane;
	if (k < a1) {
		float ar = 0, ai = 0;
		for (int t = 0; t < D_MF; t++) {
			const cf x = io.agc[(k - t) & DM_AGC_MASK];
			ar += T.mf[t] * x.x;
			ai += T.mf[t] * x.y;
		}
		cf v; v.x = ar; v.y = ai;
		const int p = k & DM_MASK;
		io.mf[p] = v;
		if (p >= DM_RING - SS_HIST) io.mf[p - DM_RING] = v;      // the mirror in front of entry 0 (demod_lds.h)
		if (TAPS) { io.tap_mf[k] = v; io.tap_level[k] = io.lvl[p]; }
	}
}

// ---------------- wave 3: arbitrary resampler, 24-bit fixed-point phase (msresamp_crcf_execute, src/hfdl.c:676) ----------------

// The launch's channelizer output: `nblk` blocks end to end, one stretch of samples g = 0 .. n_in - 1.  Sample g waits in
// ring[g & DM_IN_MASK] from when it is fetched until the resampler has gone past it; the entries in front of sample 0 hold the
// previous launch's last D_RS_TAPS - 1 samples (ChanArrays::rs_hist).
struct DemodInput {
	const cf *chan;                // this channel's samples of the launch's first block
	size_t blk_stride;             // from a block's samples to the next block's
	const int *ends;               // LDS [DM_MAX_BLOCKS]: samples up to and including each block (blocks past the launch's last add nothing)
	cf *ring;                      // LDS [DM_IN_RING]
	int n_in;
};

// The block the fetches have reached, wave-uniform: samples [start, end) are block b's.  The samples are fetched in ascending order, a
// chunk at a time, so the table is not searched per sample: a fetch starts from the cursor, only the lanes of a chunk that lie past the
// block at hand walk on from it (once per block), and the cursor is moved up once per chunk (advance()).
struct BlockCursor {
	int b = 0, start = 0, end = 0;
	__device__ __forceinline__ void begin(const DemodInput &in) { b = 0; start = 0; end = __builtin_amdgcn_readfirstlane(in.ends[0]); }
	// to the block that holds sample g (g wave-uniform, not below start); past the launch's last sample it stays in the last block
	__device__ __forceinline__ void advance(const DemodInput &in, int g)
	{
		g = __builtin_amdgcn_readfirstlane(g);
		while (g >= end && b < DM_MAX_BLOCKS - 1) { start = end; b++; end = __builtin_amdgcn_readfirstlane(in.ends[b]); }
	}
};

// sample g of the launch, start <= g < n_in
__device__ __forceinline__ cf input_sample(const DemodInput &in, const BlockCursor &at, int g)
{
	int b = at.b, start = at.start;
	if (__builtin_expect(g >= at.end, 0)) {
		int e = at.end;
		do { start = e; b++; e = in.ends[b]; } while (g >= e && b < DM_MAX_BLOCKS - 1);      // (g < n_in = ends[DM_MAX_BLOCKS - 1])
	}
	return in.chan[(size_t)b * in.blk_stride + (size_t)(g - start)];
}

// outputs [k0, k1), k1 - k0 <= 64: a lane per output
template <bool TAPS>
__device__ __forceinline__ void resample_outputs(uint32_t rs_phase, const DemodConst &T, const BlockIo &io, const cf *ring, int k0, int k1, int lane)
{
	const int k = k0 + lane;
	if (k < k1) {
		const uint64_t t = (uint64_t)rs_phase + (uint64_t)k * T.rs_step;
		const int i = (int)(t >> 24);
		const float *h = T.rs_h + ((t & 0xFFFFFFu) >> 16) * D_RS_TAPS;
		float ar = 0, ai = 0;
		for (int j = 0; j < D_RS_TAPS; j++) {
			const cf x = ring[(i - j) & DM_IN_MASK];
			ar += h[j] * x.x;
			ai += h[j] * x.y;
		}
		cf v; v.x = ar; v.y = ai;
		io.rs[k & DM_MASK] = v;
		if (TAPS) io.tap_resampled[k] = v;
	}
}

// ---------------- wave 1: symbol timing recovery (symsync_crcf_execute, src/hfdl.c:696) ----------------

// The filter windows are not kept anywhere: window sample `age` of input sample k is matched-filter output k - age, and the
// launch's matched-filter outputs sit in a mirrored LDS ring (demod_lds.h) whose SS_HIST entries before mf[0] hold, at the start of
// a launch, the previous launch's last 18 (padded with zeros: the "tap t + 16" products of lanes t >= 2 read them against a zero tap).  Every output GATHERS its taps with
// one LDS read per lane, issued one input sample ahead; nothing is shifted per input sample.  liquid's symsync_crcf_reset
// clears the matched-filter window only: `valid_from` is the first input sample whose matched-filter window entries count
// (older ones read as zero in rows 0, 1); ChanScalars.ss_head carries it from block to block (<= 0 at block start).
struct SymsyncRegs {
	float rate, del, tau, bf, q, qhat, v1;
	int b, decim, j;               // filter-bank index, decimation counter, running output index of the block
	int valid_from;
};

__device__ __forceinline__ void symsync_load(SymsyncRegs &r, const ChanScalars &s, const ChanArrays &a, const BlockIo &io, int lane)
{
	// history prefix: mf[-1 - age] = the window the previous block left (canonical array form: index 0 newest, 18 - age older)
	if (lane < SS_HIST) {
		cf v; v.x = 0.f; v.y = 0.f;
		if (lane < D_SS_TAPS) v = a.ss_dmf[lane == 0 ? 0 : D_SS_TAPS - lane];
		io.mf[-1 - lane] = v;
	}
	r.rate = s.ss_rate; r.del = s.ss_del; r.tau = s.ss_tau; r.bf = s.ss_bf; r.q = s.ss_q; r.qhat = s.ss_qhat; r.v1 = s.ss_v1;
	r.b = s.ss_b; r.decim = (int)s.ss_decim; r.j = 0;
	r.valid_from = s.ss_head;
}

// symsync_crcf_reset as the framer left it after input sample k0-1: loop scalars initial, matched-filter window empty
__device__ __forceinline__ void symsync_restart(SymsyncRegs &r, const DemodShared &sh, int k0)
{
	r.rate = HFDL_DM_SS_RATE0; r.del = HFDL_DM_SS_RATE0; r.tau = 0.f; r.bf = 0.f; r.q = 0.f; r.qhat = 0.f; r.v1 = 0.f;
	r.b = 0; r.decim = 0;
	r.j = k0 > 0 ? (int)sh.cum[(k0 - 1) & DM_MASK] : 0;
	r.valid_from = k0;
}

__device__ __forceinline__ void symsync_store(const SymsyncRegs &r, ChanScalars &s, ChanArrays &a, const BlockIo &io, int n_out, int lane)
{
	if (lane < D_SS_TAPS) a.ss_dmf[lane == 0 ? 0 : D_SS_TAPS - lane] = io.mf[((n_out - 1) & DM_MASK) - lane];      // reaches into the mirror (the prefix when n_out < 18)
	if (lane == 0) {
		s.ss_rate = r.rate; s.ss_del = r.del; s.ss_tau = r.tau; s.ss_bf = r.bf; s.ss_q = r.q; s.ss_qhat = r.qhat; s.ss_v1 = r.v1;
		s.ss_b = r.b; s.ss_decim = (uint32_t)r.decim;
		const int vf = r.valid_from - n_out;
		s.ss_head = vf < -64 ? -64 : vf;
	}
}

// Samples [k0, k1) of ONE turn of the ring (the caller cuts a chunk at the wrap).
// MASKED: some window entries of the chunk's first samples date from before the last timing-loop reset (only in the 18 samples after
// one); the common chunk runs the variant without the per-sample test and selects.
// This wave bounds every launch and is bound by its instruction count (profiles/r14_experiments.md), so the loop is laid out for the
// steady state -- an input sample yields one output or none:
//   - the first output of a sample is straight-line code; only a timing loop far off its rate (another output from the same sample)
//     enters the general loop behind it;
//   - the outputs go to the ring as the raw row totals: the division by three (liquid's 1 / k scaling) is the carrier wave's, two per
//     lane and chunk on what it loads (carrier_chunk) instead of two per output here;
//   - the filter-bank index is (int)(bf + copysign(largest float below 1/2, bf)): the same integer as (int)roundf(bf) for every float
//     (tests/hostsim/round_form_check.cpp compares all 2^32), three instructions instead of roundf's ten;
//   - one lane pointer stepped per sample serves both window reads.
template <bool MASKED>
__device__ __forceinline__ void symsync_chunk(SymsyncRegs &r, const DemodConst &T, const BlockIo &io, const DemodShared &sh, int k0, int k1, int lane)
{
	const int row = lane >> 4, t = lane & 15;
	// wp = &mf[k - 16 - t].component of this lane's row, k = the sample at hand: tap t + 16 of the window is wp[0], tap t is wp[32]
	const float *wp = (const float *)(io.mf - (k0 & ~DM_MASK) - t - 16) + (row & 1) + 2 * k0;
	const float2 *const hp = sh.sstab + lane;
	float2 h = hp[(r.b < 0 ? 0 : (r.b >= D_SS_NPFB ? D_SS_NPFB - 1 : r.b)) * 64];
	float w_lo = wp[32], w_hi = wp[0];
	// An output's two components are the row totals in lanes 15 (re) and 31 (im): those two lanes store them themselves with an ALL-lane
	// LDS write whose other lanes aim at a scratch word of their own -- no lane reads, no exec masking on the loop's path.  The
	// per-sample output counts collect in a register, one lane per input sample of the chunk, and go to LDS once per chunk.
	const bool out_lane = lane == 15 || lane == 31;
	char *const out_base = out_lane ? (char *)((float *)sh.outq + (lane == 31 ? 1 : 0)) : (char *)(sh.sink + lane);
	const uint32_t out_stride = out_lane ? (uint32_t)sizeof(cf) : 0u;
	int cum_v = 0;
	// one output from the window (wl, wh) through the filter bank h, and the loop's step to the next output's bank
	auto output_step = [&](float wl, float wh) {
		// four 18-tap dot products at once: row 0/1 = matched filter re/im, row 2/3 = derivative filter re/im
		const float p = row_scan_sum(h.x * wl + h.y * wh);
		if (__builtin_expect(r.j < sh.outq_cap, 1)) *(float *)(out_base + out_stride * (uint32_t)(r.j & (OUTQ_RING - 1))) = p;
		r.j++;
		const bool filter = r.decim == 2;        // wave-uniform: one scalar compare, one branch around the loop filter
		r.decim = filter ? 1 : r.decim + 1;
		if (filter) {
			const float mx = lane_value(p, 15), my = lane_value(p, 31);
			const float dx = lane_value(p, 47), dy = lane_value(p, 63);
			float q = mx * dx + my * dy;
			q = q > 1.0f ? 1.0f : (q < -1.0f ? -1.0f : q);
			r.q = q;
			const float v0 = q - T.lf_a1 * r.v1;
			r.qhat = T.lf_b0 * v0;
			r.v1 = v0;
			r.rate += T.ss_rate_adj * r.qhat;
			r.del = r.rate + r.qhat;
		}
		r.tau += r.del;
		r.bf = r.tau * (float)D_SS_NPFB;
		r.b = (int)(r.bf + __builtin_copysignf(0x1.fffffep-2f, r.bf));
	};
	for (int k = k0; k < k1; k++, wp += 2) {
		// the next input sample's window entries are fetched now, a whole iteration before they can be needed (sample k1 belongs to
		// the next chunk and may still be in the making: that value is never used)
		const float n_lo = wp[34], n_hi = wp[2];
		if (r.b < D_SS_NPFB) {
			float wl = w_lo, wh = w_hi;
			if (MASKED && k - (D_SS_TAPS - 1) < r.valid_from && row < 2) {          // matched-filter window entries from before the last reset are empty
				if (k - t < r.valid_from) wl = 0.f;
				if (k - t - 16 < r.valid_from) wh = 0.f;
			}
			output_step(wl, wh);
			if (__builtin_expect(r.b < D_SS_NPFB, 0)) {      // another output from this input sample (four at the most, as liquid's buffer)
				int produced = 1;
				do {
					h = hp[(r.b < 0 ? 0 : r.b) * 64];
					output_step(wl, wh);
					produced++;
				} while (r.b < D_SS_NPFB && produced < 4);
			}
		}
		r.tau -= 1.0f;
		r.bf -= (float)D_SS_NPFB;
		r.b -= D_SS_NPFB;
		const int lo = r.b > 0 ? r.b : 0;
		h = hp[(lo < D_SS_NPFB - 1 ? lo : D_SS_NPFB - 1) * 64];      // branch of the next input sample: fetched while the stores drain
		cum_v = (lane == k - k0) ? (r.j < 65535 ? r.j : 65535) : cum_v;
		w_lo = n_lo; w_hi = n_hi;
	}
	if (lane < k1 - k0) sh.cum[(k0 + lane) & DM_MASK] = (uint16_t)cum_v;
}

// ---------------- wave 2: carrier loop, equaliser, slicer, framer (src/hfdl.c:709-891) ----------------

struct CarrierRegs {
	float eu, ev, ex2, ewx, ewy;   // equaliser: lane 1 + t (t < 15) of rows 0 and 1 = tap t (0 oldest); row 0 holds (x, y), row 1 (y, -x)
	float px, py;                  // lane i < 16: PSK constellation entry i (demod_tables.h psk_pts)
};

// The carrier wave's slicer.  modem_demodulate_psk takes arg(x), subtracts pi (1 - 1/M) and walks a binary reference ladder:
// that IS the nearest constellation point by angle, i.e. the point with the largest Re(x conj(p)).  Here every lane of row 0
// holds one point of the table (demod_tables.h psk_pts): one multiply-add per lane, a row max, a compare -- instead of atan2f
// and the ladder (~45 instructions of the carrier loop's per-symbol critical path).  Decisions can differ from the atan2f form
// only when x is within rounding of a decision boundary, exactly as two atan2f implementations differ from each other; what
// leaves this function into the loop is the phase error against the chosen point.  (The decoded bits of data symbols come from
// the burst decoder's own soft de-mapper, which keeps the reference's arg() form.)
struct LaneSlicer {
	float px, py;                  // lane i < 16: table entry i
	int lane;
	__device__ __forceinline__ uint32_t operator()(int arity, cf x, float *phase_error) const
	{
		uint32_t sym;
		cf xh;
		if (arity == 1) {
			sym = (x.x > 0) ? 0 : 1;
			xh.x = sym ? -1.0f : 1.0f; xh.y = 0.0f;
		} else {
			const int M = 1 << arity, base = M - 2;
			const bool mine = lane >= base && lane < base + M;
			const float d = mine ? x.x * px + x.y * py : -1.0f;
			const float best = lane_value(row_scan_max(d), 15);        // >= 0: some point is within 90 degrees of x
			const unsigned long long hit = __builtin_amdgcn_fcmpf(d, best, 1 /* FCMP_OEQ */);       // lanes without a point hold -1: never equal
			int win = hit ? (int)__builtin_ctzll(hit) : base;           // NaN input: no lane compares equal
			const uint32_t lin = (uint32_t)(win - base);
			sym = lin ^ (lin >> 1);
			xh.x = lane_value(px, win); xh.y = lane_value(py, win);
		}
		if (phase_error) *phase_error = x.y * xh.x - x.x * xh.y;
		return sym;
	}
};

__device__ __forceinline__ void carrier_load(CarrierRegs &c, const ChanScalars &s, const ChanArrays &a, const DemodConst &T, int lane)
{
	c.px = lane < 16 ? T.psk_pts[2 * lane] : 0.f;
	c.py = lane < 16 ? T.psk_pts[2 * lane + 1] : 0.f;
	const int t = (lane & 15) - 1;                 // the window sits in lanes 1..15 of a row: a push is ONE row shift whose vacated lane 15 takes the new sample
	const bool act = t >= 0 && lane < 32, row1 = (lane >> 4) & 1;
	int j = s.eq_head + t; if (j >= D_EQ) j -= D_EQ;
	const cf e = act ? a.eq_buf[j] : cf{0.f, 0.f};
	c.eu = row1 ? e.y : e.x;
	c.ev = row1 ? -e.x : e.y;
	c.ex2 = act ? a.eq_x2[j] : 0.f;
	const cf w = act ? a.eq_w[t] : cf{0.f, 0.f};
	c.ewx = w.x; c.ewy = w.y;
}

__device__ __forceinline__ void carrier_store(const CarrierRegs &c, ChanArrays &a, int lane)
{
	if (lane >= 1 && lane <= D_EQ) {
		cf e; e.x = c.eu; e.y = c.ev;
		a.eq_buf[lane - 1] = e; a.eq_x2[lane - 1] = c.ex2;
		cf w; w.x = c.ewx; w.y = c.ewy;
		a.eq_w[lane - 1] = w;
	}
}

// sine and cosine of the carrier NCO's phase.  |phase| <= pi: the hardware sin/cos (argument in revolutions) needs no range reduction
__device__ __forceinline__ void nco_sincos(float phase, float &sp, float &cp)
{
#ifdef HFDL_DM_LIBM_TRIG              // experiment (profiles/r03_experiments.md): the library's accurate sincosf instead of v_sin / v_cos
	sincosf(phase, &sp, &cp);
#else
	const float rev = phase * 0.15915494309189535f;
	sp = __builtin_amdgcn_sinf(rev); cp = __builtin_amdgcn_cosf(rev);
#endif
}

#ifndef HFDL_DM_OUT_LANES            // timing-recovery outputs a chunk of the carrier wave takes at most (a smaller value makes every chunk take
#define HFDL_DM_OUT_LANES 64         // the cut: how that path was tested, profiles/r03_experiments.md)
#endif

// processes samples [k0, k1); returns the index of the sample during which the framer reset the timing loop (the wave stops
// after that sample), or -1.
// The loop runs over the timing-recovery OUTPUTS of the chunk, not over its input samples: two of three input samples yield an
// output, and a loop nest "per sample: level, noise-floor clock, output count; per output: ..." spends ~30 instructions and seven
// branches per input sample on bookkeeping -- a quarter of this wave's time.  The input sample an output belongs to is the first one
// whose cumulative output count exceeds the output's index (one compare across the lanes that hold the chunk's counts + s_ff1);
// what the reference does per input sample (the noise-floor estimator's clock while searching, src/hfdl.c:700-702; the sample
// counter) is caught up in closed form in front of every symbol that can change the framer state (those that go through on_symbol())
// and at the end of the chunk -- the state is the same for all the samples in between, it only changes on such symbols.
template <bool TAPS>
__device__ __forceinline__ int carrier_chunk(CarrierRegs &c, ChanScalars &s, ChanArrays &a, const DemodConst &T, const BlockIo &io, const DemodShared &sh,
		int k0, int &k1, int &nsym, int lane, StateProbe &probe)
{
	const int t = (lane & 15) - 1;
	const bool row1 = (lane >> 4) & 1, act = t >= 0 && lane < 32;
	int n = k1 - k0;                             // <= DM_CHUNK <= 64
	// the chunk's levels, output counts and (up to 64) timing-recovery outputs, one per lane: the loop below takes them with
	// v_readlane instead of a dependent LDS round trip per sample
	const float lv_l = (lane < n) ? io.lvl[(k0 + lane) & DM_MASK] : 0.f;
	const int cum_l = (lane < n) ? (int)sh.cum[(k0 + lane) & DM_MASK] : 0x7fffffff;
	const int jbase = k0 > 0 ? (int)sh.cum[(k0 - 1) & DM_MASK] : 0;
	cf oq_l = (jbase + lane < sh.outq_cap) ? sh.outq[(jbase + lane) & (OUTQ_RING - 1)] : cf{0.f, 0.f};
	oq_l.x = div3(oq_l.x); oq_l.y = div3(oq_l.y);      // the ring holds the timing recovery's raw row totals (symsync_chunk): out = total / 3
	{   // the chunk's outputs are taken from the 64 lanes of oq_l: a chunk that produced more (a timing loop far off its rate: up to four
		// outputs per input sample) is cut where they end, and k1 tells the caller
		const unsigned long long over = __ballot(lane < n && cum_l - jbase > HFDL_DM_OUT_LANES);
		if (__builtin_expect(over != 0, 0)) { n = (int)__builtin_ctzll(over); k1 = k0 + n; }      // n >= 1: one sample yields at most 4 outputs
	}
	int jstop = __builtin_amdgcn_readlane(cum_l, n - 1);
	if (jstop > sh.outq_cap) jstop = sh.outq_cap;
	const uint64_t cnt0 = s.sample_cnt;
	int kdone = 0;                               // input samples of the chunk whose per-sample bookkeeping is done: k0 .. k0 + kdone - 1
	int reset_at = -1;
	// Data symbols of a frame in progress go to HBM (the frame buffer the burst decoder reads) a chunk at a time: every lane writes the
	// (wave-uniform) symbol to the next slot of a 64-entry LDS stage, and one coalesced store per chunk moves them -- instead of a lane-0
	// store under an exec mask with its 64-bit address arithmetic per symbol.  A chunk's staged symbols are consecutive in one frame buffer
	// (a frame's data ends with the frame; the next frame's starts a preamble later).
	int staged = 0, stage_at = 0;                // symbols in the stage, frame-buffer index of the first
	auto flush_stage = [&]() {
		if (lane < staged) io.data[stage_at + lane] = sh.stage[lane];
		staged = 0;
	};
	// noise-floor estimator clock of input samples [kdone, upto] of the chunk (src/hfdl.c:700-702): it ticks while the framer searches, and
	// every 256th tick takes that sample's level.  The framer state is the same for all of them (no output in between).
	// Called in front of every symbol handed to on_symbol() (the only place the framer state changes) and at the end of the chunk, so
	// every sample is counted in the state the reference saw it in.
	auto catch_up = [&](int upto) {
		if (s.fr_state == FR_A1) {
			const uint32_t d = (uint32_t)(upto + 1 - kdone), c0 = s.nf_clk;
			uint32_t first = (NF_CLK_MASK - c0) & NF_CLK_MASK;          // ticks until the low byte reads 0xFF (0: a whole turn)
			if (first == 0) first = NF_CLK_MASK + 1;
			s.nf_clk = (uint32_t)__builtin_amdgcn_readfirstlane((int)(c0 + d));
			if (first <= d) {                                // at most once: d <= 64
				const float level = lane_value(lv_l, kdone + (int)first - 1);
				s.noise_floor = NF_KEEP * s.noise_floor + NF_TAKE * fminf(s.noise_floor, level) + NF_BIAS;
			}
		}
		kdone = upto + 1;
	};
	bool runaway = fabsf(s.dphi) > COSTAS_RUNAWAY_DPHI && s.fr_state == FR_A1;
	const int pair_sel = (lane & 1) << 2;        // byte offset of the pair's second output in a lane permute
	auto pair_step = [&](int j) {                // outputs j (off time) and j + 1 (on time) through the carrier NCO into the equaliser's window
		// A symbol's two timing-recovery outputs at once, the off-time one in the even lanes and the on-time one in the odd lanes:
		// one rotation (sin, cos, four products) and one two-lane move of the equaliser window serve both -- the window's newest
		// entries are lanes 14 (even: the off-time sample) and 15 (odd: the on-time sample) of its row.  Same arithmetic per
		// output as the single step below; only the carrier phase of each has to be stepped and wrapped on its own.
		const int sel = ((j - jbase) << 2) + pair_sel;
		cf oi;
		oi.x = __int_as_float(__builtin_amdgcn_ds_bpermute(sel, __float_as_int(oq_l.x)));
		oi.y = __int_as_float(__builtin_amdgcn_ds_bpermute(sel, __float_as_int(oq_l.y)));
		float ph1, ph2;
		{
			const float ph = s.phi + s.dphi;
			const float dn = ph - (float)(2.0 * M_PI), up = ph + (float)(2.0 * M_PI);
			ph1 = ph > (float)M_PI ? dn : (ph < -(float)M_PI ? up : ph);
		}
		{
			const float ph = ph1 + s.dphi;
			const float dn = ph - (float)(2.0 * M_PI), up = ph + (float)(2.0 * M_PI);
			ph2 = ph > (float)M_PI ? dn : (ph < -(float)M_PI ? up : ph);
		}
		s.phi = ph2;
		float sp, cp;
		nco_sincos((lane & 1) ? ph2 : ph1, sp, cp);
		cf r;
		r.x = oi.x * cp + oi.y * sp;
		r.y = oi.y * cp - oi.x * sp;
		const float x2n = r.x * r.x + r.y * r.y;
		const float x2n1 = lane_value(x2n, 0), x2n2 = lane_value(x2n, 1);
		const float x2o1 = lane_value(c.ex2, 1), x2o2 = lane_value(c.ex2, 2);
		const float nu = row1 ? r.y : r.x, nv = row1 ? -r.x : r.y;
		c.eu = dpp_row_shl2(nu, c.eu);
		c.ev = dpp_row_shl2(nv, c.ev);
		c.ex2 = dpp_row_shl2(x2n, c.ex2);
		s.eq_x2sum = s.eq_x2sum + x2n1 - x2o1;
		s.eq_x2sum = s.eq_x2sum + x2n2 - x2o2;
	};
	// eqlms_cccf_execute, sum conj(w_i) x_i: real part reduced in row 0, imaginary part in row 1, one scan
	auto equalise = [&]() {
		const float p = row_scan_sum(act ? c.ewx * c.eu + c.ewy * c.ev : 0.f);
		cf y; y.x = lane_value(p, 15); y.y = lane_value(p, 31);
		return y;
	};
	// eqlms_cccf_step(d = known T symbol, d_hat = y)
	auto train_step = [&](cf y) {
		const float tv = t_symbol(s.T_idx) * ((s.bitmask & 1u) ? -1.0f : 1.0f);
		const float er = tv - y.x, ei = -(0.0f - y.y);
		const float bx = row1 ? -c.ev : c.eu, by = row1 ? c.eu : c.ev;       // the window sample (x, y) in either row
		const float pr = er * bx - ei * by, pi = er * by + ei * bx;
		c.ewx = c.ewx + EQ_STEP * pr / s.eq_x2sum;
		c.ewy = c.ewy + EQ_STEP * pi / s.eq_x2sum;
	};
	// The in-frame run.  Tried at the start of the chunk and at the end of every iteration that leaves the framer outside the search: the
	// searching framer's iterations pay one scalar compare for it and share no block with it.
	auto in_frame_run = [&](int &j) {
		if (!(s.symsync_out_idx & 1u) && j + 1 < jstop && s.fr_state >= FR_EQ_TRAIN && s.symbols_wanted > 1 && s.s_state == SAMPLER_SYMBOLS) {
			// Inside a frame, between two framer transitions: the next symbols_wanted - 1 symbols are all handled alike (training symbols
			// into the equaliser's update, data symbols into the stage), the framer state stands still and the timing-recovery outputs
			// stay paired.  They run here as one tight loop -- the same statements in the same order as the general iteration below
			// takes for each of them (pair step, equaliser, training step, decision, carrier loop, sampler, signal level), without its
			// state tests: what selects the path is constant over the run, and the counters move once, after it.  Everything that can
			// end the run (the frame's next transition, the chunk's last output, a full frame buffer, an equaliser still filling)
			// is decided here, in front of it, and left to the general iteration.
			const bool train = s.fr_state == FR_EQ_TRAIN;
			int n_run = (jstop - j) >> 1;
			if (n_run > s.symbols_wanted - 1) n_run = s.symbols_wanted - 1;
			if ((!train || s.eq_full) && (!s.use_data || s.data_n + n_run <= MAX_DATA_SYMBOLS)) {
				if (s.use_data && staged == 0) stage_at = s.data_slot * MAX_DATA_SYMBOLS + s.data_n;
				const unsigned long long t_run = probe.now();
				int ki = 0;
				for (int i = 0; i < n_run; i++, j += 2) {
					pair_step(j);
					const cf y = equalise();
					if (train) { train_step(y); s.T_idx++; }
					if (TAPS && lane == 0) io.tap_symbols[nsym] = y;
					nsym++;
					ki = (int)__builtin_ctzll(__ballot(cum_l > j + 1));      // the input sample this symbol came from: never before the last one's
					const float level = lane_value(lv_l, ki);
					float perr;
					LaneSlicer{c.px, c.py, lane}(s.cur_arity, y, &perr);
					const float e = 0.5f * (fabsf(perr + COSTAS_ERR_LIMIT) - fabsf(perr - COSTAS_ERR_LIMIT));      // costas_cccf_adjust, :276-281
					s.err = e;
					s.phi += COSTAS_ALPHA * e;
					s.dphi += COSTAS_BETA * e;
					if (s.use_data) sh.stage[staged++] = y;
					else if (s.training_n < T_LEN) {
						a.training[s.training_n] = y;
						s.training_n++;
					}
					s.signal_level = (s.signal_level * s.frame_symbol_cnt + level) / (s.frame_symbol_cnt + 1.0f);
					s.frame_symbol_cnt += 1.0f;
				}
				if (ki >= kdone) kdone = ki + 1;      // the noise-floor clock stands still outside the search: nothing to catch up with
				s.eq_count += 2u * (uint32_t)n_run;
				s.symsync_out_idx += 2u * (uint32_t)n_run;
				s.symbol_cnt += (uint64_t)n_run;
				s.symbols_wanted -= n_run;
				if (s.use_data) s.data_n += n_run;
				probe.frame_run(t_run, train, n_run);
			}
		}
	};
	// The searching run, the sibling of the in-frame run.  Called behind a searching symbol that found nothing (the general iteration's
	// plain searching path, below): the following symbols are all alike as long as the outputs stay paired, the carrier loop holds and
	// nothing is found, and run here as one tight loop -- the same statements in the same order as the general iteration takes for each of
	// them (pair step, equaliser, BPSK decision into the 127-bit window, correlation, carrier loop), without its state tests: what selected
	// that path (searching, sampler on bits, BPSK, no countdown) is not changed by it, the output parity stays even, and the counters move
	// once, after the run.  The run ends in front of a run-away's single step and at the chunk's last pair, both left to the next general
	// iteration: `finished`, and (jo, y) is the run's last symbol (the caller's own if the run was empty).  It ends ON a detection or on the no-frame timeout: that symbol has gone
	// through the pair step and the equaliser, as it has in the general iteration before the correlation is known, and nothing else of it
	// is committed: `finished` is false and (jo, y) is that symbol, the caller's for on_symbol().  Placed there, not at the start of a
	// chunk, so that on_symbol() is inlined once and an iteration inside a frame pays nothing for the run.
	struct SearchRunEnd { bool finished; int jo; cf y; };
	auto search_run = [&](int &j, int jo, cf y) {
		bool finished = true;
		const uint64_t room = (uint64_t)(NO_FRAME_TIMEOUT_FRAMES * SINGLE_SLOT_FRAME_LEN) - 1u - s.symbol_cnt;      // searching symbols that may still go by without the timeout
		const int n_left = room > 64u ? 64 : (int)room;                  // (a chunk has at most 32 pairs)
		int n_run = 0;
		while (j + 1 < jstop && !runaway) {
			pair_step(j);
			jo = j + 1; j += 2;
			y = equalise();
			if (TAPS && lane == 0) io.tap_symbols[nsym] = y;
			nsym++;
			const bool neg = !(y.x > 0);
			const uint32_t bit = (neg ? 1u : 0u) ^ (s.bitmask & 1u);
			const uint64_t nhi = ((s.bits_hi << 1) | (s.bits_lo >> 63)) & 0x7FFFFFFFFFFFFFFFull, nlo = (s.bits_lo << 1) | bit;
			const int m = bits_correlate(nhi, nlo, T.a_hi, T.a_lo);
			n_run++;
			if (__builtin_expect(!(m > T.a1_lo && m < T.a1_hi && n_run <= n_left), 0)) { finished = false; break; }
			const float perr = y.y * (neg ? -1.0f : 1.0f) - y.x * 0.0f;
			const float e = 0.5f * (fabsf(perr + COSTAS_ERR_LIMIT) - fabsf(perr - COSTAS_ERR_LIMIT));
			s.err = e;
			s.phi += COSTAS_ALPHA * e;
			s.dphi += COSTAS_BETA * e;
			s.bits_hi = nhi; s.bits_lo = nlo;
			runaway = fabsf(s.dphi) > COSTAS_RUNAWAY_DPHI;
		}
		s.eq_count += 2u * (uint32_t)n_run;
		s.symsync_out_idx += 2u * (uint32_t)n_run;
		s.symbol_cnt += (uint64_t)(finished ? n_run : n_run - 1);      // the symbol that ended the run is on_symbol()'s to count
		probe.search_run(n_run);
		return SearchRunEnd{finished, jo, y};
	};
	int j = jbase;
	if (s.fr_state != FR_A1) in_frame_run(j);
	while (j < jstop) {
		const unsigned long long t_iter = probe.now();
		const int state_iter = s.fr_state;
		int jo;                                   // the output the rest of the iteration is about
		bool on_time;
		if (!(s.symsync_out_idx & 1u) && j + 1 < jstop && !runaway) {
			pair_step(j);
			s.eq_count += 2;
			jo = j + 1; j += 2; s.symsync_out_idx += 2;
			on_time = true;
		} else {
			cf oi;
			oi.x = lane_value(oq_l.x, j - jbase); oi.y = lane_value(oq_l.y, j - jbase);
			// costas_cccf_step + execute, :256-258, :284-292
			{   // selects, not branches: a taken branch costs a lone wave ~4 instruction slots (profiles/micro)
				const float ph = s.phi + s.dphi;
				const float dn = ph - (float)(2.0 * M_PI), up = ph + (float)(2.0 * M_PI);
				s.phi = ph > (float)M_PI ? dn : (ph < -(float)M_PI ? up : ph);
			}
			float sp, cp;
			nco_sincos(s.phi, sp, cp);
			cf r;
			r.x = oi.x * cp + oi.y * sp;
			r.y = oi.y * cp - oi.x * sp;
			if (__builtin_expect(runaway, 0)) {  // costas run-away while searching (src/hfdl.c:709-716); dphi only moves in on_symbol()
				s.dphi = s.phi = 0.f;
				symsync_reset(s, a);
				runaway = false;
			}
			// eqlms_cccf_push: the row moves down one lane and lane 15, which has no source inside the row, takes the new sample
			{
				const float x2n = r.x * r.x + r.y * r.y;
				const float x2o = lane_value(c.ex2, 1);
				const float nu = row1 ? r.y : r.x, nv = row1 ? -r.x : r.y;
				c.eu = dpp_row_shl1(nu, c.eu);
				c.ev = dpp_row_shl1(nv, c.ev);
				c.ex2 = dpp_row_shl1(x2n, c.ex2);
				s.eq_x2sum = s.eq_x2sum + x2n - x2o;
				s.eq_count++;
			}
			on_time = (s.symsync_out_idx & 1u) != 0;
			jo = j; j++; s.symsync_out_idx++;
		}
		if (on_time) {
			cf y = equalise();
			if (s.fr_state == FR_EQ_TRAIN) {
				bool run = true;
				if (!s.eq_full) { if (s.eq_count < (uint32_t)D_EQ) run = false; else s.eq_full = 1; }
				if (run) train_step(y);
				s.T_idx++;
			}
			if (TAPS && lane == 0) io.tap_symbols[nsym] = y;
			nsym++;
			// (The two straight-line copies of on_symbol()'s commonest paths below are guarded against drifting from it: the test-only strict
			// build runs EVERY symbol through on_symbol() in a serial loop with this pipeline's arithmetic forms emulated, and its PDUs must
			// equal this kernel's in every SNR bin -- tests/test_gpu_strict.py, strict_15 == shipped.)
			// The searching framer's symbol -- by far the commonest: a BPSK decision into the 127-bit window, the carrier loop's update, the
			// correlation against the A sequence, and nothing found.  Decided BEFORE anything is changed: such a symbol is finished here in
			// straight-line code; every other one (a detection, a frame in progress, the 13-frame re-centring) goes through on_symbol().
			bool plain = false;
			if (s.fr_state == FR_A1) {
				const bool neg = !(y.x > 0);
				const uint32_t bit = (neg ? 1u : 0u) ^ (s.bitmask & 1u);
				const uint64_t nhi = ((s.bits_hi << 1) | (s.bits_lo >> 63)) & 0x7FFFFFFFFFFFFFFFull, nlo = (s.bits_lo << 1) | bit;
				const int m = bits_correlate(nhi, nlo, T.a_hi, T.a_lo);
				if (__builtin_expect(m > T.a1_lo && m < T.a1_hi && s.s_state == SAMPLER_BITS && s.cur_arity == 1 && s.symbols_wanted <= 1
						&& s.symbol_cnt + 1 < (uint64_t)(NO_FRAME_TIMEOUT_FRAMES * SINGLE_SLOT_FRAME_LEN), 1)) {
					const float perr = y.y * (neg ? -1.0f : 1.0f) - y.x * 0.0f;      // modem phase error against (+-1, 0), as LaneSlicer writes it
					const float e = 0.5f * (fabsf(perr + COSTAS_ERR_LIMIT) - fabsf(perr - COSTAS_ERR_LIMIT));      // costas_cccf_adjust, :276-281
					s.err = e;
					s.phi += COSTAS_ALPHA * e;
					s.dphi += COSTAS_BETA * e;
					s.symbol_cnt++;
					s.bits_hi = nhi; s.bits_lo = nlo;
					runaway = fabsf(s.dphi) > COSTAS_RUNAWAY_DPHI;
					const SearchRunEnd end = search_run(j, jo, y);      // the searching symbols that follow, as one tight loop
					plain = end.finished; jo = end.jo; y = end.y;           // not finished: (jo, y) is on_symbol()'s
				}
			}
			else if (s.symbols_wanted > 1) {
				// A frame in progress, between two framer transitions (on_symbol() returns in front of its state switch): decision and
				// carrier loop update, the symbol to where the sampler wants it, the running signal level, the countdown -- the same
				// statements in the same order, laid out as one straight line instead of on_symbol()'s general control flow (which costs
				// this lone wave ten taken branches per symbol).  The framer state is not FR_A1 here and does not change.
				const int ki = (int)__builtin_ctzll(__ballot(cum_l > jo));
				if (ki >= kdone) kdone = ki + 1;      // the noise-floor clock stands still outside the search: nothing to catch up with
				const float level = lane_value(lv_l, ki);
				float perr;
				uint32_t bits = LaneSlicer{c.px, c.py, lane}(s.cur_arity, y, &perr);
				const float e = 0.5f * (fabsf(perr + COSTAS_ERR_LIMIT) - fabsf(perr - COSTAS_ERR_LIMIT));      // costas_cccf_adjust, :276-281
				s.err = e;
				s.phi += COSTAS_ALPHA * e;
				s.dphi += COSTAS_BETA * e;
				s.symbol_cnt++;
				if (s.s_state == SAMPLER_SYMBOLS) {
					if (s.use_data) {
						if (s.data_n < MAX_DATA_SYMBOLS) {
							if (staged == 0) stage_at = s.data_slot * MAX_DATA_SYMBOLS + s.data_n;
							sh.stage[staged++] = y;
							s.data_n++;
						}
					} else if (s.training_n < T_LEN) {
						a.training[s.training_n] = y;
						s.training_n++;
					}
				} else if (s.s_state == SAMPLER_BITS) {
					bits ^= s.bitmask;
					for (int b = 0; b < s.cur_arity; b++, bits >>= 1) {
						s.bits_hi = ((s.bits_hi << 1) | (s.bits_lo >> 63)) & 0x7FFFFFFFFFFFFFFFull;
						s.bits_lo = (s.bits_lo << 1) | (bits & 1u);
					}
				}
				s.signal_level = (s.signal_level * s.frame_symbol_cnt + level) / (s.frame_symbol_cnt + 1.0f);
				s.frame_symbol_cnt += 1.0f;
				s.symbols_wanted--;
				runaway = false;                     // it only counts while searching
				plain = true;
			}
			if (!plain) {
				if (staged) flush_stage();           // on_symbol() stores a data symbol itself: the stage holds consecutive symbols only
				// the input sample that produced this output: the first whose cumulative count exceeds j (lanes beyond the chunk hold INT_MAX)
				const int ki = (int)__builtin_ctzll(__ballot(cum_l > jo));
				if (ki >= kdone) catch_up(ki);       // before the framer state can change
				const float level = lane_value(lv_l, ki);
				s.sample_cnt = cnt0 + (uint64_t)ki;
				on_symbol(s, *sh.S, a, T, io, y, level, LaneSlicer{c.px, c.py, lane});
				runaway = fabsf(s.dphi) > COSTAS_RUNAWAY_DPHI && s.fr_state == FR_A1;
			}
		}
		probe.iteration(t_iter, state_iter);
		if (__builtin_expect(s.ev_flags != 0, 0)) {
			if (s.ev_flags & EV_EQ_RESET) {      // eqlms_cccf_reset ran (framer reset): mirror it in the register window
				c.eu = 0.f; c.ev = 0.f; c.ex2 = 0.f;
				c.ewx = act ? T.eq_h0[t >= 0 ? t : 0] : 0.f; c.ewy = 0.f;
				s.ev_flags &= ~(uint32_t)EV_EQ_RESET;
			}
			if ((s.ev_flags & EV_SS_RESET) != 0 && reset_at < 0) {
				// the timing loop was reset during this output's input sample: the outputs it had already produced from that sample still
				// go through (symsync_crcf_execute had returned them, src/hfdl.c:707-708), then the wave stops and wave 1 restarts after it
				const int kr = (int)__builtin_ctzll(__ballot(cum_l > jo));
				if (kr >= kdone) catch_up(kr);       // only after an off-time output (carrier run-away), which leaves the framer state alone
				reset_at = kr;
				int j1 = __builtin_amdgcn_readlane(cum_l, kr);
				if (j1 < jstop) jstop = j1;
			}
		}
		if (s.fr_state != FR_A1) in_frame_run(j);
	}
	if (staged) flush_stage();
	if (reset_at >= 0) {
		s.ev_flags = 0;
		s.sample_cnt = cnt0 + (uint64_t)reset_at + 1u;
		return k0 + reset_at;
	}
	if (kdone < n) catch_up(n - 1);              // input samples after the last output
	s.sample_cnt = cnt0 + (uint64_t)n;
	return -1;
}

// ---------------- one launch ----------------

// All DM_THREADS threads of the channel's workgroup call this.  On return the channel's arrays (LDS, `a`) and scalars (*sh.S)
// hold the state after the launch's samples.  Returns the number of 5400-sps samples produced.
// TAPS: the per-stage debug taps (DATADUMPS analogue) and the phase cycle counters are compiled in; the production launch uses the
// variant without them (fewer live pointers in the carrier wave, which is short of SGPRs as it is).  A tap is written by the lane
// that computes the sample, when it computes it.
template <bool TAPS>
__device__ inline int demod_block(ChanArrays &a, const DemodConst &T, const BlockIo &io, const DemodShared &sh, const DemodInput &in)
{
	const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
	ChanScalars &S = *sh.S;
	unsigned long long tR0 = __builtin_amdgcn_s_memtime();

	const uint32_t rs_phase = S.rs_phase;
	const int n_in = in.n_in;
	const uint64_t total = (uint64_t)n_in << 24;
	int n_out = 0;
	if ((uint64_t)rs_phase < total) n_out = (int)((total - rs_phase + T.rs_step - 1) / T.rs_step);
	if (n_out > io.cap - DM_PHASE_SLOTS) n_out = io.cap - DM_PHASE_SLOTS;      // cannot happen: cap is sized from the geometry (+8); the last level slots carry phase cycles
	auto need = [&](int k_end) { return resampler_inputs(rs_phase, T.rs_step, k_end, n_out, n_in); };
	// what the resampler leaves for the next launch, by wave 3 when it is done with the ring
	auto resampler_store = [&]() {
		cf nh;
		if (lane < D_RS_TAPS - 1) nh = in.ring[(n_in - 1 - lane) & DM_IN_MASK];       // reaches into the entries in front of sample 0 when n_in < 13
		__builtin_amdgcn_wave_barrier();
		if (lane < D_RS_TAPS - 1) a.rs_hist[lane] = nh;
		if (lane == 0) {
			S.rs_phase = (uint32_t)((uint64_t)rs_phase + (uint64_t)n_out * T.rs_step - total);
			if (TAPS) io.tap_counts[0] = n_out;
		}
	};

	// ---- ahead of the pipeline: the histories in front of sample 0 of the input and AGC rings, the channelizer samples of the first
	// three chunks, and the resampler's first chunk -- wave 0 starts on it at once
	if (tid < D_RS_TAPS - 1) in.ring[(-1 - tid) & DM_IN_MASK] = a.rs_hist[tid];
	if (wave == WAVE_TIMING && lane < D_MF - 1) io.agc[(-1 - lane) & DM_AGC_MASK] = a.mf_hist[lane];
	const int rs0 = n_out < DM_CHUNK ? n_out : DM_CHUNK;
	int in_loaded = need(rs0 + 2 * DM_CHUNK);
	BlockCursor at;
	at.begin(in);
	for (int g = tid; g < in_loaded; g += DM_THREADS) in.ring[g & DM_IN_MASK] = input_sample(in, at, g);
	if (TAPS && tid == 0) io.tap_counts[1] = 0;
	__syncthreads();
	if (wave == WAVE_RESAMPLER) resample_outputs<TAPS>(rs_phase, T, io, in.ring, 0, rs0, lane);
	__syncthreads();
	if (n_out < 1) {
		if (wave == WAVE_RESAMPLER) resampler_store();
		return 0;
	}

	unsigned long long tP0 = __builtin_amdgcn_s_memtime();
	// ---- the four-wave pipeline over chunks of DM_CHUNK samples.  Every wave runs its OWN copy of the step loop (same number
	// of barriers, same mailbox reads), so that only its own stage's state is live in its registers.
	unsigned long long busy = 0;
	int nsym = 0;
	StepClock clk;
	StateProbe states;
	PipeProgress pp;
	pp.rs_ready = rs0;
	if (wave == WAVE_RESAMPLER) {
		for (int step = 0; pp.s3_done < n_out; step++) {
			PipeMail &mail = step_mail(sh.mbox, step);
			clk.begin<WAVE_RESAMPLER>();
			int to = pp.rs_ready;
			if (to < n_out) {
				to = resampler_advance(pp, n_out);
				// the samples two chunks further on are asked for first and put into the ring last
				const int hi = need(resampler_fetch_ahead(to, n_out));
				at.advance(in, in_loaded);            // the block of the first sample this step fetches
				cf nx[2];
#pragma unroll
				for (int u = 0; u < 2; u++) {
					const int g = in_loaded + 64 * u + lane;
					nx[u] = g < hi ? input_sample(in, at, g) : cf{0.f, 0.f};
				}
				resample_outputs<TAPS>(rs_phase, T, io, in.ring, pp.rs_ready, to, lane);
#pragma unroll
				for (int u = 0; u < 2; u++) {
					const int g = in_loaded + 64 * u + lane;
					if (g < hi) in.ring[g & DM_IN_MASK] = nx[u];
				}
				for (int g = in_loaded + 128 + lane; g < hi; g += 64) in.ring[g & DM_IN_MASK] = input_sample(in, at, g);      // (a chunk spans fewer than 65 samples)
				if (hi > in_loaded) in_loaded = hi;
			}
			if (lane == 0) mail.rs_ready = to;
			clk.end<WAVE_RESAMPLER>(busy, mail, lane);
			__syncthreads();
			pp.read(&mail);
		}
		resampler_store();
	} else if (wave == WAVE_AGC) {
		float agc_g = S.agc_g, agc_y2 = S.agc_y2;
		for (int step = 0; pp.s3_done < n_out; step++) {
			PipeMail &mail = step_mail(sh.mbox, step);
			clk.begin<WAVE_AGC>();
			int to = agc_advance(pp);
			if (to > pp.mf_ready) agc_mf_chunk<TAPS>(agc_g, agc_y2, T, io, pp.mf_ready, to, lane); else to = pp.mf_ready;
			if (lane == 0) mail.mf_ready = to;
			clk.end<WAVE_AGC>(busy, mail, lane);
			__syncthreads();
			pp.read(&mail);
		}
		cf nh;
		if (lane < D_MF - 1) nh = io.agc[(n_out - 1 - lane) & DM_AGC_MASK];       // reaches into the entries in front of sample 0 when n_out < 18
		__builtin_amdgcn_wave_barrier();
		if (lane < D_MF - 1) a.mf_hist[lane] = nh;
		if (lane == 0) { S.agc_g = agc_g; S.agc_y2 = agc_y2; }
	} else if (wave == WAVE_TIMING) {
		SymsyncRegs ss;
		symsync_load(ss, S, a, io, lane);
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
		__builtin_amdgcn_wave_barrier();
		for (int step = 0; pp.s3_done < n_out; step++) {
			PipeMail &mail = step_mail(sh.mbox, step);
			const unsigned long long tb = TAPS ? __builtin_amdgcn_s_memtime() : 0ull;
			if (pp.restart) symsync_restart(ss, sh, pp.ss_ready);
			const int to = timing_advance(pp);
			for (int k0 = pp.ss_ready; k0 < to;) {
				const int k1 = (k0 | DM_MASK) + 1 < to ? (k0 | DM_MASK) + 1 : to;      // a chunk that crosses the ring's wrap: two pieces
				if (__builtin_expect(k0 - (D_SS_TAPS - 1) < ss.valid_from, 0)) symsync_chunk<true>(ss, T, io, sh, k0, k1, lane);
				else symsync_chunk<false>(ss, T, io, sh, k0, k1, lane);
				k0 = k1;
			}
			if (lane == 0) mail.ss_ready = to;
			if (TAPS) { busy += __builtin_amdgcn_s_memtime() - tb; clk.end_since<WAVE_TIMING>(tb, mail, lane); }
			__syncthreads();
			pp.read(&mail);
		}
		if (pp.restart) symsync_restart(ss, sh, n_out);      // a reset during the launch's last sample
		symsync_store(ss, S, a, io, n_out, lane);
	} else {
		CarrierRegs cr;
		ChanScalars s3 = S;               // wave 2's working copy: it owns every field but the resampler / AGC / timing-loop ones
		s3.ev_flags = 0;
		carrier_load(cr, s3, a, T, lane);
		for (int step = 0; pp.s3_done < n_out; step++) {
			PipeMail &mail = step_mail(sh.mbox, step);
			const unsigned long long tb = TAPS ? __builtin_amdgcn_s_memtime() : 0ull;
			int to = carrier_advance(pp);         // (carrier_chunk cuts it where more than 64 timing-recovery outputs end)
			int reset_at = -1;
			if (to > pp.s3_done) reset_at = carrier_chunk<TAPS>(cr, s3, a, T, io, sh, pp.s3_done, to, nsym, lane, states); else to = pp.s3_done;
			if (lane == 0) { mail.s3_done = reset_at >= 0 ? reset_at + 1 : to; mail.s3_reset = reset_at >= 0; }
			if (TAPS) { busy += __builtin_amdgcn_s_memtime() - tb; clk.end_since<WAVE_CARRIER>(tb, mail, lane); }
			__syncthreads();
			pp.read(&mail);
			clk.after_barrier(mail);
		}
		carrier_store(cr, a, lane);
		if (lane == 0) {
			// every field wave 2 owns (the timing-loop scalars it touched through symsync_reset() are wave 1's)
			S.phi = s3.phi; S.dphi = s3.dphi; S.err = s3.err;
			S.eq_x2sum = s3.eq_x2sum; S.eq_count = s3.eq_count; S.eq_full = s3.eq_full; S.eq_head = 0;
			S.bits_hi = s3.bits_hi; S.bits_lo = s3.bits_lo;
			S.training_n = s3.training_n; S.data_n = s3.data_n; S.use_data = s3.use_data; S.data_slot = s3.data_slot;
			S.symbol_cnt = s3.symbol_cnt; S.sample_cnt = s3.sample_cnt;
			S.s_state = s3.s_state; S.fr_state = s3.fr_state; S.cur_arity = s3.cur_arity;
			S.symbols_wanted = s3.symbols_wanted; S.T_idx = s3.T_idx;
			S.bitmask = s3.bitmask; S.symsync_out_idx = s3.symsync_out_idx; S.nf_clk = s3.nf_clk;
			S.frame_symbol_cnt = s3.frame_symbol_cnt; S.signal_level = s3.signal_level;
			S.noise_floor = s3.noise_floor;
			// (the fields only the framer's rare transitions touch were updated in place: on_symbol()'s `c`)
			S.ev_flags = 0;
			if (TAPS) io.tap_counts[1] = nsym;
		}
	}
	unsigned long long tP1 = __builtin_amdgcn_s_memtime();
	if (TAPS) {
		// phase cycles: what runs ahead of the pipeline, the whole pipelined phase (wall), wave 1 busy, wave 2 busy
		if (tid == 0) { io.tap_level[phase_slot(io.cap, PHASE_AHEAD)] = (float)(tP0 - tR0); io.tap_level[phase_slot(io.cap, PHASE_PIPELINE)] = (float)(tP1 - tP0); }
		if (wave == WAVE_TIMING && lane == 0) io.tap_level[phase_slot(io.cap, PHASE_TIMING_BUSY)] = (float)busy;
		if (wave == WAVE_CARRIER && lane == 0) io.tap_level[phase_slot(io.cap, PHASE_CARRIER_BUSY)] = (float)busy;
		clk.report(io.tap_level, io.cap, wave, lane, busy, states);
	}
	return n_out;
}

}  // namespace hfdl
