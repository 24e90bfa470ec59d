// planner.h plan_batches with the demodulator's real bound (fit_output_counts: the block table and the 16-bit output counts, what
// Demod::fit_batch applies for the product's ring-buffered kernel): a half that closes full is ONE demodulator launch wherever the counts
// allow it.  tests/hostsim/batch_plan_check.cpp keeps checking the rule against stand-in bounds of 3 and 7 blocks.  Prints "ok".
#include <cstdio>
#include "planner.h"

using namespace hfdl;

#define CHECK(cond) do { if (!(cond)) { printf("fail line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

struct Geo { Plan p; int outs; float rate; };
static Geo geometry(int fs)
{
	Geo g;
	const int decimation = fft_decimation_rate(fs, 1800 * 3);
	plan_block(g.p, relative_transition_bw(fs, 250), decimation, 0.f);
	g.outs = (g.p.post_input_size + g.p.post - 1) / g.p.post + 1;       // (frontend_create.cpp)
	g.rate = (float)(1800 * 3) / ((float)fs / (float)decimation);
	return g;
}

static BatchPlan plan(int fs, int nch, int nrx, const BatchOverrides &ov = BatchOverrides(), int *kept = nullptr)
{
	const Geo g = geometry(fs);
	auto fit = [=](int want) { return fit_output_counts(g.outs, g.rate, want); };
	const BatchPlan b = plan_batches(nch, nrx, g.p.n, g.p.input_size, fs, g.p.pre, nch >= 128, fit, ov);
	if (kept) *kept = fit(b.batch_want);
	return b;
}

int main()
{
	int kept = 0;
	// cfg3: 40 Msps, 256 channels: 32 blocks of 0.1835 s make 31 734 samples at 5400 sps, twice that fits 16 bits
	const Geo g3 = geometry(40000000);
	CHECK(demod_launch_samples(g3.outs, 32, g3.rate) == 31734 && fit_output_counts(g3.outs, g3.rate, 32) == 32);
	BatchPlan b = plan(40000000, 256, 1, BatchOverrides(), &kept);
	CHECK(b.fold_nb == 32 && b.batch_want == 32 && kept == 32 && b.half_blocks == 32 && b.half_first == 16);
	// cfg2: 8 Msps, 32 channels: a half of 8 is one launch of 8
	b = plan(8000000, 32, 1, BatchOverrides(), &kept);
	CHECK(b.fold_nb == 8 && b.batch_want == 8 && kept == 8 && b.half_blocks == 8 && b.half_first == 8);
	// 250 ksps, a few channels (the test geometry): likewise
	b = plan(250000, 3, 1, BatchOverrides(), &kept);
	CHECK(b.fold_nb == 8 && b.batch_want == 8 && kept == 8 && b.half_blocks == 8);
	// eight receivers at 40 Msps: the half shrinks to 4 blocks and the launch with it; 64 receivers leave one block
	b = plan(40000000, 64, 8, BatchOverrides(), &kept);
	CHECK(b.fold_nb == 4 && b.batch_want == 4 && kept == 4 && b.half_blocks == 4);
	b = plan(40000000, 64, 64, BatchOverrides(), &kept);
	CHECK(b.fold_nb == 1 && b.batch_want == 1 && b.half_blocks == 1);
	// an override is taken as it is, up to what the counts allow: 32 at 250 ksps (3.67 s, and the half grows to hold it) ...
	BatchOverrides ov;
	ov.demod_batch = 32;
	b = plan(250000, 3, 1, ov, &kept);
	CHECK(b.batch_want == 32 && kept == 32 && b.fold_nb == 8 && b.half_blocks == 32);
	// ... with a fold launch of 32 the half is 32 without an override of the demodulator's
	ov = BatchOverrides();
	ov.fold_batch = 32;
	b = plan(250000, 3, 1, ov, &kept);
	CHECK(b.fold_nb == 32 && b.batch_want == 32 && kept == 32 && b.half_blocks == 32);
	// ... and where 32 blocks are more than 32 767 samples (128 ksps: blocks of 0.224 s) the launch is cut to the 27 that fit; a half of
	// 32 is then two launches of 16
	const Geo g2 = geometry(128000);
	CHECK(fit_output_counts(g2.outs, g2.rate, 32) == 27 && 2 * demod_launch_samples(g2.outs, 27, g2.rate) <= 65535 && 2 * demod_launch_samples(g2.outs, 28, g2.rate) > 65535);
	ov = BatchOverrides();
	ov.fold_batch = 32;
	b = plan(128000, 3, 1, ov, &kept);
	CHECK(b.fold_nb == 32 && b.batch_want == 16 && kept == 16 && b.half_blocks == 32);
	ov.demod_batch = 32;
	b = plan(128000, 3, 1, ov, &kept);
	CHECK(b.batch_want == 27 && kept == 27 && b.half_blocks == 32);
	// a launch per block on request
	ov = BatchOverrides();
	ov.demod_batch = 1;
	CHECK(plan(40000000, 256, 1, ov).batch_want == 1);
	// the frame records and data slots that go with these launches (plan_frame_slots): a second of signal keeps one record and two slots
	const FrameSlots f3 = plan_frame_slots(31734.0 / 5400.0), f1 = plan_frame_slots(0.93);
	CHECK(f3.per_channel == 3 && f3.data_slots == 7 && f1.per_channel == 1 && f1.data_slots == 2);
	printf("ok\n");
	return 0;
}
