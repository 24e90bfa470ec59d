// iqbal_check.cpp -- the host build of dumphfdl_amd/csrc/iqbal.h: consecutive blocks of one receiver through the corrector from a fresh
// enable, in the documented order, for the tests to set against float64 (tests/test_iqbal_cpu.py) and against the device's words
// (tests/test_gpu_iqbal.py).
//   iqbal_check IN OUT N NBLOCKS ALPHA [KAPPA_RE KAPPA_IM DC_RE DC_IM HOLD]
// IN: NBLOCKS * N cf32 samples, already converted.  OUT: the NBLOCKS * N cf32 samples as they enter the transform, then NBLOCKS records
// (hfdl_gpu_iqbal_stats).  One line per block on stdout: "block mode depth" and the block's five sums as hex words.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "hfdl_gpu.h"
#include "iqbal.h"

int main(int argc, char **argv)
{
	if (argc != 6 && argc != 11) { fprintf(stderr, "usage: %s IN OUT N NBLOCKS ALPHA [KAPPA_RE KAPPA_IM DC_RE DC_IM HOLD]\n", argv[0]); return 2; }
	const long n = atol(argv[3]), nblocks = atol(argv[4]);
	const float alpha = (float)atof(argv[5]);
	if (n < 1 || n > hfdl::BLANK_N_MAX || nblocks < 1 || nblocks > hfdl::IQBAL_BLOCKS_MAX || !hfdl::iqbal_alpha_valid(alpha) || alpha == 0.f) { fprintf(stderr, "bad N, NBLOCKS or ALPHA\n"); return 2; }
	hfdl::IqbalSeed sd;
	memset(&sd, 0, sizeof(sd));
	if (argc == 11) {
		sd.k_re = (float)atof(argv[6]); sd.k_im = (float)atof(argv[7]); sd.m_re = (float)atof(argv[8]); sd.m_im = (float)atof(argv[9]);
		sd.gen = 1; sd.hold = atoi(argv[10]) != 0;
		if (!hfdl::iqbal_seed_valid(sd.k_re, sd.k_im, sd.m_re, sd.m_im)) { fprintf(stderr, "bad seed\n"); return 2; }
	}
	std::vector<float> x((size_t)(2 * n * nblocks)), y(x.size());
	FILE *f = fopen(argv[1], "rb");
	if (!f || fread(x.data(), sizeof(float), x.size(), f) != x.size()) { fprintf(stderr, "%s: not %ld samples\n", argv[1], n * nblocks); return 2; }
	fclose(f);
	std::vector<hfdl_gpu_iqbal_stats> rec((size_t)nblocks);
	hfdl::IqbalState s;
	memset(&s, 0, sizeof(s));
	float sum[5] = { 0.f, 0.f, 0.f, 0.f, 0.f };
	for (long b = 0; b < nblocks; b++) {
		const int mode = hfdl::iqbal_block(s, sum, sd, alpha, b == 0, x.data() + 2 * n * b, (int)n, y.data() + 2 * n * b);
		hfdl::iqbal_stats_of(s, &rec[(size_t)b]);
		uint32_t w[5];
		memcpy(w, sum, sizeof(w));
		printf("%ld %d %d %08x %08x %08x %08x %08x\n", b, mode, hfdl::blank_sum_depth((int)n), w[0], w[1], w[2], w[3], w[4]);
	}
	f = fopen(argv[2], "wb");
	if (!f || fwrite(y.data(), sizeof(float), y.size(), f) != y.size() || fwrite(rec.data(), sizeof(rec[0]), rec.size(), f) != rec.size() || fclose(f) != 0) { perror(argv[2]); return 2; }
	return 0;
}
