// The create-time rules of planner.h on the host: plan_batches (slices, fold and demodulator batches, the multi-receiver cap, even launches,
// halves and the staging ring) against the figures DESIGN.md documents for the three benchmark geometries, and fold_row_windows (the pruned
// fold's per-octet windows) on made-up row energies.  The demodulator's own bound (Demod::fit_batch: what fits the LDS) is an input here,
// stated per geometry as DESIGN.md states it.  Prints "ok".
#include <cstdio>
#include <vector>
#include "planner.h"

using namespace hfdl;

#define CHECK(cond) do { if (!(cond)) { printf("fail line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

// the block geometry of a sample rate, as the front end plans it
static Plan geometry(int fs)
{
	Plan p;
	plan_block(p, relative_transition_bw(fs, 250), fft_decimation_rate(fs, 5400), 0.f);
	return p;
}

static BatchPlan plan(int fs, int nch, int nrx, int lds_fit, const BatchOverrides &ov = BatchOverrides())
{
	const Plan p = geometry(fs);
	return plan_batches(nch, nrx, p.n, p.input_size, fs, p.pre, nch >= 128, [=](int want) { return std::min(want, lds_fit); }, ov);
}

static int check_batches()
{
	// cfg3: 40 Msps, 256 channels; three blocks of it fit the demodulator's share of the LDS beside a fold workgroup
	BatchPlan b = plan(40000000, 256, 1, 3);
	CHECK(b.slices == 1 && b.fold_nb == 32 && b.batch_want == 3 && b.half_blocks == 32 && b.half_first == 16 && b.n_stage == 18);
	// cfg2: 8 Msps, 32 channels; seven blocks fit the LDS, a half of 8 is cut evenly into two launches of 4
	b = plan(8000000, 32, 1, 7);
	CHECK(b.fold_nb == 8 && b.batch_want == 4 && b.half_blocks == 8 && b.half_first == 8 && b.n_stage == 10);
	CHECK(32 * b.slices >= 256 && 32 * b.slices / 2 < 256 && geometry(8000000).pre / b.slices >= 8);
	// cfg1: one channel -- sliced as far as a slice keeps 8 alias rows, never more than the rows allow
	const int fs1 = 250000, pre1 = geometry(fs1).pre;
	b = plan(fs1, 1, 1, 8);
	CHECK(b.slices >= 1 && b.slices * 8 <= std::max(pre1, 8) && (b.slices * 2 > pre1 / 8 || b.slices >= 256));
	CHECK(b.fold_nb == 8 && b.half_blocks == 8 && b.half_first == 8 && b.batch_want >= 1 && b.batch_want <= 8);
	// eight receivers at 40 Msps: 32 x 2^23 / (8 N) = 4 blocks per fold launch instead of 8
	CHECK(plan(40000000, 64, 1, 3).fold_nb == 8);
	b = plan(40000000, 64, 8, 3);
	CHECK(geometry(40000000).n == 1 << 23);
	CHECK(b.fold_nb == 4 && b.half_blocks == 4 && b.batch_want <= 4 && b.n_stage == 6);
	// ... and one receiver more or less moves the cap: 64 receivers leave one block, two receivers of few channels are not capped
	CHECK(plan(40000000, 64, 64, 3).fold_nb == 1 && plan(40000000, 64, 64, 3).batch_want == 1);
	CHECK(plan(40000000, 64, 2, 3).fold_nb == 8);
	// an explicit HFDL_GPU_DEMOD_BATCH is taken as it is (no even cut), up to what fits
	BatchOverrides ov;
	ov.demod_batch = 7;
	b = plan(8000000, 32, 1, 7, ov);
	CHECK(b.batch_want == 7 && b.fold_nb == 8 && b.half_blocks == 8);
	ov.demod_batch = 1;
	CHECK(plan(40000000, 256, 1, 3, ov).batch_want == 1);
	// HFDL_GPU_FOLD_BATCH=1: a half holds `batch` blocks, one fold launch each
	ov = BatchOverrides();
	ov.fold_batch = 1;
	b = plan(40000000, 256, 1, 3, ov);
	CHECK(b.fold_nb == 1 && b.batch_want == 3 && b.half_blocks == 3 && b.half_first == 3 && b.n_stage == 5);
	b = plan(8000000, 32, 1, 7, ov);
	CHECK(b.fold_nb == 1 && b.batch_want == 7 && b.half_blocks == 7);
	// a fold batch that does not divide: the half is the next multiple that holds the demodulator batch, at most 32
	ov.fold_batch = 3;
	b = plan(8000000, 32, 1, 7, ov);
	CHECK(b.half_blocks % 3 == 0 && b.half_blocks >= 7 && b.half_blocks <= 32);
	// the pruned fold has one slice; the laboratory's ramp switch closes the first half at full size
	ov = BatchOverrides();
	ov.pruned = true;
	CHECK(plan(8000000, 32, 1, 7, ov).slices == 1);
	ov = BatchOverrides();
	ov.no_ramp = true;
	CHECK(plan(40000000, 256, 1, 3, ov).half_first == 32);
	return 0;
}

// energies en[r * npad + c] of p rows: `peak` gets 1, its neighbours at distance d get fall^d
static void put_channel(std::vector<float> &en, int p, int npad, int c, int peak, double fall)
{
	for (int r = 0; r < p; r++) {
		const int d = std::min((r - peak + p) % p, (peak - r + p) % p);
		double e = 1;
		for (int i = 0; i < d; i++) e *= fall;
		en[(size_t)r * npad + c] = (float)e;
	}
}

static int check_windows()
{
	const int p = 64, npad = 16, nch = 8, nq = p / 4;       // octet 0: eight channels; octet 1: padding only
	int rows_max = 0;
	// a single-peak channel (the others of its octet peak in the same row): the window holds the peak's quad, two quads long
	std::vector<float> en((size_t)p * npad, 0.f);
	for (int c = 0; c < nch; c++) put_channel(en, p, npad, c, 21, 1e-6);
	std::vector<RowWindow> w = fold_row_windows(en, p, npad, nch, 1e-2, &rows_max);
	CHECK(w.size() == 2);
	CHECK(w[0].count == 2 && (w[0].first == 21 / 4 || (w[0].first + 1) % nq == 21 / 4));
	CHECK(w[1].first == 0 && w[1].count == 2);             // an all-padding octet: any two quads
	CHECK(rows_max == 8);
	// a peak in the last row, its energy spilling into rows p - 2 and 0, 1: the window wraps p - 1 -> 0
	for (int c = 0; c < nch; c++) put_channel(en, p, npad, c, p - 1, 0.5);
	w = fold_row_windows(en, p, npad, nch, 0.2, &rows_max);
	CHECK(w[0].count >= 2 && w[0].count < nq);
	CHECK(w[0].first + w[0].count > nq);                    // runs past the last quad: into quad 0
	CHECK(w[0].first <= nq - 1 && (w[0].first + w[0].count - 1) % nq < w[0].first);
	// channels of one octet peaking in different rows: the window is their hull; counts even and <= p / 4; tol monotone
	for (int c = 0; c < nch; c++) put_channel(en, p, npad, c, 10 + 3 * c, 0.3);
	int last = 0;
	for (double tol : { 1e-1, 1e-2, 1e-3, 1e-4, 1e-6, 1e-9 }) {
		w = fold_row_windows(en, p, npad, nch, tol, &rows_max);
		CHECK(w[0].count % 2 == 0 && w[0].count >= 2 && w[0].count <= nq && rows_max == 4 * w[0].count);
		CHECK(w[0].count >= last);                          // a smaller tolerance never folds fewer rows
		// every channel's peak row lies inside the window
		for (int c = 0; c < nch; c++) CHECK(((10 + 3 * c) / 4 - w[0].first + nq) % nq < w[0].count);
		last = w[0].count;
	}
	CHECK(last == nq || last >= (10 + 3 * 7) / 4 - 10 / 4 + 1);
	// flat energy: nothing can be skipped, every quad is folded
	std::fill(en.begin(), en.end(), 1.f);
	w = fold_row_windows(en, p, npad, nch, 1e-3, &rows_max);
	CHECK(w[0].count == nq && rows_max == p);
	return 0;
}

int main()
{
	if (check_batches() || check_windows()) return 1;
	printf("ok\n");
	return 0;
}
