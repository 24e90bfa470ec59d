// demod_lds.h -- the sizes of the demodulator's LDS rings and the carve-up of a channel's workgroup (demod_kernels.hip, demod_core.h).
// Plain C++ over demod_logic.h's state structs: the kernel, the host-side size computation and tests/hostsim read the same constructor.
//
// Every per-sample array is a power-of-two RING indexed by the sample's index in the launch: a workgroup's LDS does not depend on how
// many blocks the launch takes (37 KiB: four workgroups per CU), and the batch is bounded by the block table and the 16-bit output
// counts alone (Demod::fit_batch).  What keeps a ring entry alive until its last reader is done is the distance the stages may run apart,
// all of them measured from the carrier wave's progress s3_done.  The rules are code, below the ring sizes they depend on:
// resampler_advance(), agc_advance(), timing_advance(), carrier_advance() say how far a stage may go in a step of the pipeline, and the
// step loops of demod_core.h demod_block call them (and keep no clamp of their own).  tests/hostsim/demod_pipe_check.cpp steps the four stages through the mailbox under
// adversarial schedules and checks that no ring entry is overwritten while it can still be read, and that every launch ends.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "demod_logic.h"

namespace hfdl {

#ifndef HFDL_DM_CHUNK
#define HFDL_DM_CHUNK 32
#endif
constexpr int DM_CHUNK = HFDL_DM_CHUNK;      // chunk: measured, profiles/r02_experiments.md
// The timing-recovery outputs travel from wave 1 to wave 2 through a RING of this many entries (round 6; until then a buffer of twice the
// launch's samples: 16 of the 46 bytes of LDS a sample cost).  Wave 1 never runs more than two chunks ahead of what wave 2 has finished
// (demod_block), a sample yields at most four outputs and wave 2 looks at 64 entries at a time: at most 2 x 32 x 4 + 64 entries are live.
constexpr int OUTQ_RING = 512;
static_assert((OUTQ_RING & (OUTQ_RING - 1)) == 0 && OUTQ_RING >= 2 * DM_CHUNK * 4 + 64 + 64, "ring: a power of two that holds what can be live");

constexpr int SS_HIST = 34;                  // matched-filter samples the timing recovery reads behind its current one (demod_core.h)
// Samples of the launch live at index & (DM_RING - 1): resampler output, matched-filter output, AGC level, cumulative output count.
constexpr int DM_RING = 256, DM_MASK = DM_RING - 1;
// The matched-filter ring is MIRRORED: its last SS_HIST entries are also kept right in front of entry 0, so that the SS_HIST samples
// behind any sample are consecutive in memory and the timing recovery's gathers need no wrap (a chunk that crosses the wrap is
// processed in two pieces).  An entry is overwritten DM_RING samples later, its mirror likewise: the writer must stay less than
// DM_RING - SS_HIST ahead of the oldest sample a restart can need.
constexpr int DM_MF_AHEAD = DM_RING - 2 * DM_CHUNK, DM_RS_AHEAD = DM_RING - DM_CHUNK;
static_assert(DM_MF_AHEAD + SS_HIST <= DM_RING && DM_MF_AHEAD >= 3 * DM_CHUNK, "matched-filter ring: history survives, and the pipeline in step (three chunks ahead) is never held back");
static_assert(DM_RS_AHEAD <= DM_RING && DM_RS_AHEAD >= DM_MF_AHEAD + DM_CHUNK, "resampler ring");
// AGC outputs are read by the matched filter of the same wave only: a chunk and D_MF - 1 samples of history
constexpr int DM_AGC_RING = 64, DM_AGC_MASK = DM_AGC_RING - 1;
static_assert(DM_AGC_RING >= DM_CHUNK + D_MF - 1 && DM_CHUNK <= 64, "AGC ring");
// Channelizer samples of the launch (its blocks end to end), fetched from HBM up to three chunks of resampler outputs ahead: at a
// resampling rate > 0.5 a chunk of outputs spans fewer than 2 DM_CHUNK + 1 inputs, plus D_RS_TAPS - 1 of history
constexpr int DM_IN_RING = 256, DM_IN_MASK = DM_IN_RING - 1;
static_assert(DM_IN_RING >= 3 * (2 * DM_CHUNK + 1) + D_RS_TAPS, "input ring");
// Blocks per launch at most (the block table in LDS): a whole half (planner.h PLAN_MAX_HALF), so that a half that closes full can be
// ONE launch.  The resampler wave does not search the table per sample: it carries the block at hand (demod_core.h BlockCursor).
constexpr int DM_MAX_BLOCKS = 32;
constexpr size_t DM_LDS_BUDGET = 40 * 1024;  // per workgroup: four to a CU's 160 KiB

// What the four waves tell each other at a step's barrier (demod_core.h demod_block).  Two of these in LDS, written in turn: a step's
// writers never meet the readers of the step before.  Every field has one writer, lane 0 of the wave named.
struct PipeMail {
	int mf_ready;                  // AGC + matched filter wave: matched-filter outputs [0, mf_ready) are in the ring
	int ss_ready;                  // timing-recovery wave: input samples [0, ss_ready) are through, their outputs in the output ring
	int s3_done;                   // carrier wave: input samples [0, s3_done) are finished for good
	int s3_reset;                  // carrier wave: nonzero = the framer reset the timing loop during sample s3_done - 1
	int rs_ready;                  // resampler wave: resampler outputs [0, rs_ready) are in the ring
	int busy[3];                   // experiment builds only (-DHFDL_DM_PROBE=6): this step's cycles of waves 0, 1, 2
};

// progress of the four stages as every wave sees it after a step's barrier
struct PipeProgress {
	int rs_ready = 0, mf_ready = 0, ss_ready = 0, s3_done = 0;
	bool restart = false;
	// (By pointer: ss_ready is loaded only when no reset is reported.  Through a reference the compiler may load it first and select.)
	__host__ __device__ inline void read(const PipeMail *m)
	{
		rs_ready = m->rs_ready;
		mf_ready = m->mf_ready;
		s3_done = m->s3_done;
		restart = m->s3_reset != 0;
		ss_ready = restart ? s3_done : m->ss_ready;    // a reset discards what wave 1 computed beyond the reset sample
	}
};

// ---- how far a stage may go in a step, from the progress of the step before.  A stage works on [its own mark, the value returned) when
// that is not empty, and publishes its mark unchanged otherwise.

// Resampler, while it has outputs left (rs_ready < n_out): a chunk of them, and never more than its ring holds beyond what the carrier
// wave has finished (never binds while the waves run in step).
__host__ __device__ inline int resampler_advance(const PipeProgress &pp, int n_out)
{
	int to = pp.rs_ready + DM_CHUNK < n_out ? pp.rs_ready + DM_CHUNK : n_out;
	if (to > pp.s3_done + DM_RS_AHEAD) to = pp.s3_done + DM_RS_AHEAD;
	return to;
}
// ... and the outputs whose channelizer samples it fetches in the step that produces [.., to): two chunks further on -- a round trip to HBM
// beside the fold takes as long as a chunk
__host__ __device__ inline int resampler_fetch_ahead(int to, int n_out) { return to + 2 * DM_CHUNK < n_out ? to + 2 * DM_CHUNK : n_out; }
// channelizer samples the outputs [0, k_end) need; the whole input once the last output is covered (the hand-over to the next launch reads its end)
__host__ __device__ inline int resampler_inputs(uint32_t rs_phase, uint32_t rs_step, int k_end, int n_out, int n_in)
{
	return k_end >= n_out ? n_in : (int)(((uint64_t)rs_phase + (uint64_t)(k_end - 1) * rs_step) >> 24) + 1;
}

// AGC + matched filter: a chunk of what the resampler has produced; the matched-filter ring keeps what a restart of the timing recovery
// can read (in step, the carrier wave is two chunks behind and this never binds).
__host__ __device__ inline int agc_advance(const PipeProgress &pp)
{
	int to = pp.mf_ready + DM_CHUNK < pp.rs_ready ? pp.mf_ready + DM_CHUNK : pp.rs_ready;
	if (to > pp.s3_done + DM_MF_AHEAD) to = pp.s3_done + DM_MF_AHEAD;
	return to;
}

// Timing recovery: a chunk of the matched filter's outputs, never more than two chunks ahead of what the carrier wave has finished: the
// output ring holds that much (in step, the carrier wave is exactly one chunk behind and this never binds; it does when a timing loop
// far off its rate makes the carrier wave cut its chunks short).
__host__ __device__ inline int timing_advance(const PipeProgress &pp)
{
	int to = pp.ss_ready + DM_CHUNK < pp.mf_ready ? pp.ss_ready + DM_CHUNK : pp.mf_ready;
	if (to > pp.s3_done + 2 * DM_CHUNK) to = pp.s3_done + 2 * DM_CHUNK;
	if (to < pp.ss_ready) to = pp.ss_ready;
	return to;
}

// Carrier wave: a chunk of what the timing recovery is through with.
__host__ __device__ inline int carrier_advance(const PipeProgress &pp)
{
	return pp.s3_done + DM_CHUNK < pp.ss_ready ? pp.s3_done + DM_CHUNK : pp.ss_ready;
}

// The last DM_PHASE_SLOTS entries of a channel's level tap carry the launch's cycle counters (HFDL_GPU_TAP_PHASE_CYCLES): a launch
// produces at most cap - DM_PHASE_SLOTS samples.
constexpr int DM_PHASE_SLOTS = 4;
enum PhaseSlot { PHASE_AHEAD = 0, PHASE_PIPELINE = 1, PHASE_TIMING_BUSY = 2, PHASE_CARRIER_BUSY = 3 };      // what runs ahead of the pipeline, the pipelined phase (wall), wave 1 busy, wave 2 busy
__host__ __device__ constexpr int phase_slot(int cap, PhaseSlot which) { return cap - DM_PHASE_SLOTS + (int)which; }

// LDS carve-up of a channel's workgroup, shared by the kernel and the host-side size computation
struct DemodLds {
	size_t arrays, scalars, sstab, mf, eq, m1, corr, mbox, blk, sink, stage, in, rs, agc, mfo, lvl, outq, cum, rs_h, total;
	__host__ __device__ explicit DemodLds(int cap)
	{
		size_t o = 0;
		auto take = [&](size_t bytes) { size_t at = o; o += (bytes + 15) & ~(size_t)15; return at; };
		arrays = take(sizeof(ChanArrays));
		scalars = take(sizeof(ChanScalars));
		sstab = take(sizeof(float) * 2 * D_SS_NPFB * 64);
		mf = take(sizeof(float) * 32);
		eq = take(sizeof(float) * 16);
		m1 = take(sizeof(uint64_t) * 16);
		corr = take(sizeof(float) * 128);
		mbox = take(2 * sizeof(PipeMail));             // the double-buffered progress mailbox
		blk = take(sizeof(int) * 2 * DM_MAX_BLOCKS);   // channelizer samples per block of the launch, then their running sums
		sink = take(sizeof(float) * 64);               // where the lanes of an all-lane LDS write that have nothing to say put it
		stage = take(sizeof(cf) * 64);                 // data symbols of the carrier wave's current chunk, on their way to HBM
#ifdef HFDL_DM_STRICT
		// the test-only serial loop indexes the launch's samples absolutely: whole-launch arrays, the input staged in agc + mfo
		in = 0;
		rs = take(sizeof(cf) * (size_t)cap);
		agc = take(sizeof(cf) * (size_t)cap);
		mfo = take(sizeof(cf) * ((size_t)cap + SS_HIST)) + sizeof(cf) * SS_HIST;
		lvl = take(sizeof(float) * (size_t)cap);
		cum = take(sizeof(uint16_t) * (size_t)cap);
#else
		(void)cap;
		in = take(sizeof(cf) * DM_IN_RING);
		rs = take(sizeof(cf) * DM_RING);
		agc = take(sizeof(cf) * DM_AGC_RING);
		mfo = take(sizeof(cf) * (SS_HIST + DM_RING + 1)) + sizeof(cf) * SS_HIST;      // mirror, ring, one entry the look-ahead read may touch
		lvl = take(sizeof(float) * DM_RING);
		cum = take(sizeof(uint16_t) * DM_RING);
#endif
		outq = take(sizeof(cf) * (size_t)OUTQ_RING);
		rs_h = take(sizeof(float) * D_RS_NPFB * D_RS_TAPS);
		total = o;
	}
};

}  // namespace hfdl
