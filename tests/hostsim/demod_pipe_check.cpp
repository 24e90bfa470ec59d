// The demodulator's pipeline driver on the host: the four stages of demod_core.h demod_block stepped through the double-buffered mailbox by
// the advance rules of demod_lds.h, which this file includes alone (the device qualifiers are defined here, as in partition_lds_check.cpp).
// What the rules do not decide is chosen adversarially: how many outputs the timing recovery yields per input sample (0 to 4), how many
// samples of what it is offered the carrier stage finishes (1 to DM_CHUNK, cut where more than 64 outputs end, as carrier_chunk does), and
// whether and where in its chunk it reports a reset of the timing loop.
//
// Every ring entry carries the index of the sample it holds.  A read of sample k must find k there, written before the step began or by
// the reading wave itself earlier in the step; and no wave writes an entry that another wave reads in the same step.  So an entry that
// is overwritten while it can still be read -- in that step or any later one the schedule reaches -- fails the run at that read.  Every
// step until the carrier stage has finished the launch must advance some stage.  Prints the number of steps checked and "ok".
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <vector>
#define __device__
#define __host__
static const struct { unsigned x; } threadIdx = { 0 };
static inline int atomicAdd(int *p, int v) { int o = *p; *p += v; return o; }
static inline int __popcll(unsigned long long x) { return __builtin_popcountll(x); }
static inline int __popc(unsigned x) { return __builtin_popcount(x); }
#include "demod_lds.h"

using namespace hfdl;

enum { W_AGC = 0, W_TIMING = 1, W_CARRIER = 2, W_RESAMPLER = 3, N_WAVES = 4 };      // demod_core.h WAVE_*

static const char *failed_ring = nullptr;
static long long failed_index = 0;
static int failed_line = 0;
#define FAIL(ring, k) do { if (!failed_ring) { failed_ring = (ring); failed_index = (k); failed_line = __LINE__; } return; } while (0)

// A ring of `size` entries indexed by a sample's (or an output's) index, which may be negative: the history in front of sample 0.
// Steps are numbered across launches and an entry remembers the launch that filled it, so that nothing is cleared between launches.
static int launch_no = 0;
struct Ring {
	const char *name;
	int size;
	struct Entry {
		long long tag = 0;            // the index it holds
		int launch = -1;              // ... of this launch
		long long wr_step = -1; int wr_wave = -1;          // who wrote it last, and when
		long long rd_step = -1; unsigned rd_waves = 0;     // the last step in which it was read, and by which waves
	};
	std::vector<Entry> e;
	Ring(const char *n, int sz) : name(n), size(sz), e(sz) {}
	Entry &at(long long k) { return e[(size_t)(k & (size - 1))]; }       // a power of two
	void prefill(long long k) { Entry &x = at(k); x.tag = k; x.launch = launch_no; }        // ahead of the pipeline, before its first barrier
	void read(long long k, int wave, long long step)
	{
		Entry &x = at(k);
		if (x.tag != k || x.launch != launch_no) FAIL(name, k);            // not there yet, or overwritten while it could still be read
		if (x.wr_step == step && x.wr_wave != wave) FAIL(name, k);         // another wave writes it in this very step
		if (x.rd_step != step) { x.rd_step = step; x.rd_waves = 0; }
		x.rd_waves |= 1u << wave;
	}
	void write(long long k, int wave, long long step)
	{
		Entry &x = at(k);
		if (x.rd_step == step && (x.rd_waves & ~(1u << wave))) FAIL(name, k);      // another wave reads what it held in this very step
		if (x.wr_step == step && x.wr_wave != wave) FAIL(name, k);
		x.tag = k; x.launch = launch_no; x.wr_step = step; x.wr_wave = wave;
	}
};

static uint64_t rng_state;
static uint32_t rnd()                           // xorshift64*
{
	rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
	return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}
static int rnd_below(int n) { return (int)(rnd() % (uint32_t)n); }

// what the adversary decides
struct Schedule {
	enum Outputs { STEADY, NONE, FOUR, RANDOM } outputs = STEADY;       // timing-recovery outputs per input sample
	int out_weights[5] = { 1, 1, 1, 1, 1 };                                // RANDOM: weights of 0 .. 4
	bool cut_to_one = false;                     // the carrier stage finishes one sample of every chunk
	int cut_percent = 0;                         // ... or, that often, any 1 .. n of them
	int reset_at_sample = -1;                    // a reset during this sample of the launch
	bool reset_every_chunk = false;              // a reset at the first sample of every chunk
	int reset_percent = 0;                       // ... or, that often, at any sample of the chunk
	uint32_t rs_phase = 0, rs_step = 1u << 24;   // the resampler's 24-bit fixed-point phase and step: a rate in (0.5, 1]
};

static int outputs_of(const Schedule &sc, int k)
{
	switch (sc.outputs) {
	case Schedule::STEADY: return k % 3 != 0;    // two of three input samples yield an output
	case Schedule::NONE: return 0;
	case Schedule::FOUR: return 4;
	default: {
		int total = 0;
		for (int w : sc.out_weights) total += w;
		int r = rnd_below(total);
		for (int i = 0; i < 5; i++) { if (r < sc.out_weights[i]) return i; r -= sc.out_weights[i]; }
		return 0; }
	}
}

static Ring r_in("DM_IN_RING input", DM_IN_RING), r_rs("DM_RING resampler output", DM_RING), r_agc("DM_AGC_RING", DM_AGC_RING),
	r_mf("DM_RING matched filter + mirror", DM_RING), r_lvl("DM_RING level", DM_RING), r_cum("DM_RING cum", DM_RING), r_outq("OUTQ_RING", OUTQ_RING);
static std::vector<int> cum;                    // outputs produced up to and including input sample k, as the timing recovery last wrote it

static long long steps_checked = 0, tick = 0;      // tick: steps numbered across launches, what runs ahead of a pipeline included

// one launch of n_out resampler outputs; failed_ring is set when an invariant broke or the launch did not end
static void launch(int n_out, const Schedule &sc)
{
	launch_no++;
	for (const Ring *r : { &r_in, &r_rs, &r_agc, &r_mf, &r_lvl, &r_cum, &r_outq }) if (r->size & (r->size - 1)) FAIL("a ring that is no power of two", r->size);
	cum.assign(n_out > 0 ? n_out : 1, 0);
	const int n_in = n_out > 0 ? (int)(((uint64_t)sc.rs_phase + (uint64_t)(n_out - 1) * sc.rs_step) >> 24) + 1 : 0;
	auto need = [&](int k_end) { return resampler_inputs(sc.rs_phase, sc.rs_step, k_end, n_out, n_in); };
	auto input_of = [&](int k) { return (long long)(((uint64_t)sc.rs_phase + (uint64_t)k * sc.rs_step) >> 24); };

	// ahead of the pipeline: the histories in front of sample 0, the channelizer samples of the first three chunks, the resampler's first chunk
	for (int t = 0; t < D_RS_TAPS - 1; t++) r_in.prefill(-1 - t);
	for (int t = 0; t < D_MF - 1; t++) r_agc.prefill(-1 - t);
	for (int t = 0; t < SS_HIST; t++) r_mf.prefill(-1 - t);             // symsync_load: the mirror in front of entry 0
	const int rs0 = n_out < DM_CHUNK ? n_out : DM_CHUNK;
	int in_loaded = need(rs0 + 2 * DM_CHUNK);
	for (int g = 0; g < in_loaded; g++) r_in.prefill(g);
	for (int k = 0; k < rs0; k++) {
		for (int j = 0; j < D_RS_TAPS; j++) r_in.read(input_of(k) - j, W_RESAMPLER, tick);
		r_rs.prefill(k);
	}
	if (failed_ring) return;
	if (n_out < 1) return;

	PipeMail mail[2] = {};
	PipeProgress pp;
	pp.rs_ready = rs0;
	int ss_j = 0;                                 // the timing recovery's running output index
	tick++;
	for (int nstep = 0; pp.s3_done < n_out; nstep++) {
		if (nstep > 4 * n_out + 16) FAIL("the launch does not end", pp.s3_done);
		const long long step = tick++;
		PipeMail &m = mail[nstep & 1];
		bool advanced = false;

		{	// resampler: its outputs read the input ring, then the samples two chunks further on go into it
			int to = pp.rs_ready;
			if (to < n_out) {
				to = resampler_advance(pp, n_out);
				if (to < pp.rs_ready || to > n_out || to - pp.rs_ready > DM_CHUNK) FAIL("resampler_advance", to);
				const int hi = need(resampler_fetch_ahead(to, n_out));
				for (int k = pp.rs_ready; k < to; k++) {
					const long long i = input_of(k), from = k > pp.rs_ready && input_of(k - 1) > i - D_RS_TAPS ? input_of(k - 1) + 1 : i - (D_RS_TAPS - 1);
					for (long long g = from; g <= i; g++) r_in.read(g, W_RESAMPLER, step);
					r_rs.write(k, W_RESAMPLER, step);
				}
				for (int g = in_loaded; g < hi; g++) r_in.write(g, W_RESAMPLER, step);
				if (hi > in_loaded) in_loaded = hi;
			}
			advanced |= to > pp.rs_ready;
			m.rs_ready = to;
		}
		{	// AGC + matched filter (agc_mf_chunk): the chunk from the resampler's ring, a lane per sample; AGC outputs and levels; then
			// the matched filter over the AGC ring, D_MF - 1 samples of history
			int to = agc_advance(pp);
			if (to > pp.rs_ready || to - pp.mf_ready > DM_CHUNK) FAIL("agc_advance", to);
			if (to < pp.mf_ready) to = pp.mf_ready;
			for (int k = pp.mf_ready; k < to; k++) r_rs.read(k, W_AGC, step);
			for (int k = pp.mf_ready; k < to; k++) { r_agc.write(k, W_AGC, step); r_lvl.write(k, W_AGC, step); }
			for (int k = pp.mf_ready - (D_MF - 1); k < to; k++) r_agc.read(k, W_AGC, step);
			for (int k = pp.mf_ready; k < to; k++) r_mf.write(k, W_AGC, step);
			advanced |= to > pp.mf_ready;
			m.mf_ready = to;
		}
		{	// timing recovery (symsync_chunk; after a reset symsync_restart): SS_HIST matched-filter samples behind its first
			if (pp.restart) { if (pp.ss_ready > 0) { r_cum.read(pp.ss_ready - 1, W_TIMING, step); ss_j = cum[pp.ss_ready - 1]; } else ss_j = 0; }
			const int to = timing_advance(pp);
			if (to < pp.ss_ready || to > pp.mf_ready || to - pp.ss_ready > DM_CHUNK) FAIL("timing_advance", to);
			if (to > pp.ss_ready) for (int k = pp.ss_ready - SS_HIST; k < to; k++) r_mf.read(k, W_TIMING, step);
			for (int k = pp.ss_ready; k < to; k++) {
				const int n = outputs_of(sc, k);
				for (int o = 0; o < n; o++) r_outq.write(ss_j++, W_TIMING, step);
				cum[k] = ss_j;
			}
			for (int k = pp.ss_ready; k < to; k++) r_cum.write(k, W_TIMING, step);
			advanced |= to > pp.ss_ready;
			m.ss_ready = to;
		}
		{	// carrier wave (carrier_chunk): levels, output counts (and the one in front of the chunk), the chunk's outputs
			int to = carrier_advance(pp), reset_at = -1;
			if (to > pp.ss_ready || to - pp.s3_done > DM_CHUNK) FAIL("carrier_advance", to);
			if (to < pp.s3_done) to = pp.s3_done;
			if (to > pp.s3_done) {
				const int k0 = pp.s3_done;
				int n = to - k0;
				for (int k = k0; k < to; k++) { r_lvl.read(k, W_CARRIER, step); r_cum.read(k, W_CARRIER, step); }
				int jbase = 0;
				if (k0 > 0) { r_cum.read(k0 - 1, W_CARRIER, step); jbase = cum[k0 - 1]; }
				for (int i = 0; i < n; i++) if (cum[k0 + i] - jbase > 64) { n = i; break; }      // cut where more than 64 outputs end
				if (n < 1) FAIL("a sample with more than 64 outputs", k0);
				if (sc.cut_to_one) n = 1;
				else if (rnd_below(100) < sc.cut_percent) n = 1 + rnd_below(n);
				if (sc.reset_at_sample >= k0 && sc.reset_at_sample < k0 + n) reset_at = sc.reset_at_sample;
				else if (sc.reset_every_chunk) reset_at = k0;
				else if (rnd_below(100) < sc.reset_percent) reset_at = k0 + rnd_below(n);
				if (reset_at >= 0) n = reset_at - k0 + 1;       // the outputs of the reset's sample still go through, then the wave stops
				for (int j = jbase; j < cum[k0 + n - 1]; j++) r_outq.read(j, W_CARRIER, step);
				to = k0 + n;
				advanced = true;
			}
			m.s3_done = to;
			m.s3_reset = reset_at >= 0;
		}
		if (failed_ring) return;
		if (!advanced) FAIL("no stage advances", step);
		pp.read(&m);                              // the barrier: every wave sees this step's progress
		steps_checked++;
	}
	// behind the pipeline: what the waves hand to the next launch
	if (pp.rs_ready != n_out || pp.mf_ready != n_out || pp.ss_ready != n_out || in_loaded != n_in) FAIL("a stage is not done when the carrier wave is", pp.s3_done);
	const long long after = tick++;
	for (int t = 0; t < D_RS_TAPS - 1; t++) r_in.read(n_in - 1 - t, W_RESAMPLER, after);            // resampler_store
	for (int t = 0; t < D_MF - 1; t++) r_agc.read(n_out - 1 - t, W_AGC, after);                     // mf_hist
	if (pp.restart) r_cum.read(n_out - 1, W_TIMING, after);                                         // a reset during the launch's last sample
	for (int t = 0; t < D_SS_TAPS; t++) r_mf.read(n_out - 1 - t, W_TIMING, after);                  // symsync_store
}

static int run(int n_out, const Schedule &sc, const char *what)
{
	launch(n_out, sc);
	if (!failed_ring) return 0;
	printf("fail (line %d): %s, index %lld: %s, launch of %d outputs, resampler step %u phase %u\n", failed_line, failed_ring, failed_index, what, n_out,
			(unsigned)sc.rs_step, (unsigned)sc.rs_phase);
	return 1;
}

int main()
{
	const int lengths[] = { 0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 5400 };
	// resampling rates 1, 0.864 (250 ksps channels: 5400 * 40 / 250 000), and the lowest a front end takes (just above 0.5)
	const uint32_t rs_steps[] = { 1u << 24, (uint32_t)((double)(1u << 24) / 0.864), (1u << 25) - 1u };
	for (int n_out : lengths) {
		for (uint32_t rs_step : rs_steps) {
			for (int o = 0; o < 3; o++) {
				Schedule sc;
				sc.rs_step = rs_step; sc.rs_phase = rs_step == 1u << 24 ? 0u : 0xABCDEFu;
				sc.outputs = o == 0 ? Schedule::STEADY : o == 1 ? Schedule::NONE : Schedule::FOUR;
				if (run(n_out, sc, "always in step")) return 1;
				Schedule one = sc; one.cut_to_one = true;
				if (run(n_out, one, "every chunk cut to one sample")) return 1;
				Schedule every = sc; every.reset_every_chunk = true;
				if (run(n_out, every, "a reset in every chunk")) return 1;
				// a reset at every sample in turn (of the long launch: every 37th, and the last 70), the launch's last sample included
				for (int r = 0; r < n_out; r += (n_out > 1000 && r < n_out - 70 ? 37 : 1)) {
					Schedule at = sc; at.reset_at_sample = r;
					if (run(n_out, at, "a reset at one sample")) return 1;
					if (n_out <= 65) { at.cut_to_one = true; if (run(n_out, at, "a reset at one sample, chunks cut to one")) return 1; }
				}
				Schedule last = sc; last.reset_at_sample = n_out - 1;
				if (run(n_out, last, "a reset during the last sample")) return 1;
			}
		}
	}
	const long long corners = steps_checked;
	rng_state = 0x9E3779B97F4A7C15ull;
	const int n_random = 100000;
	for (int i = 0; i < n_random; i++) {
		Schedule sc;
		const int n_out = rnd_below(256) == 0 ? 5400 : lengths[rnd_below(14)];
		sc.rs_step = rnd_below(4) == 0 ? rs_steps[rnd_below(3)] : (1u << 24) + (uint32_t)rnd_below((1 << 24) - 1);
		sc.rs_phase = (uint32_t)rnd_below(1 << 24);
		sc.outputs = Schedule::RANDOM;
		for (int &w : sc.out_weights) w = rnd_below(4) == 0 ? 0 : 1 + rnd_below(8);
		sc.out_weights[rnd_below(5)] += 1 + rnd_below(16);
		const int cuts[] = { 0, 5, 50, 100 }, resets[] = { 0, 2, 20, 100 };
		sc.cut_percent = cuts[rnd_below(4)];
		sc.reset_percent = resets[rnd_below(4)];
		if (run(n_out, sc, "random")) { printf("random launch %d\n", i); return 1; }
	}
	printf("%lld steps checked (%lld in the corner schedules, %d random launches)\nok\n", steps_checked, corners, n_random);
	return 0;
}
