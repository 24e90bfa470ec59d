// real_input_check.cpp -- the host build of dumphfdl_amd/csrc/real_input.h (with planner.h, as the front end uses the two) for the tests to
// set against float64 (tests/test_real_input_cpu.py) and against the device's words (tests/test_gpu_real_input.py).
//   real_input_check plan FS_R BASE FREQ        one line: the planner mapping and the channel's plan_block record, floats as hex words
//   real_input_check taps FS_R BASE FREQ OUT    OUT: the L_r real-rate taps (cf32), then the 2 T words of the even / odd split
//   real_input_check pairs LOGN                 "ok" if the workgroups' ranges and mirrors cover every bin of N' = 2^LOGN exactly once
//   real_input_check untangle IN OUT LOGN       IN: Z, N' cf32; OUT: X by real_untangle / real_twiddle, N' cf32
//   real_input_check combine IN OUT LOGN        IN: FFT(h_even), FFT(h_odd), N' cf32 each; OUT: the stored words, N' cf32
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "planner.h"
#include "real_input.h"

using namespace hfdl;

static uint32_t word(float f) { uint32_t w; memcpy(&w, &f, 4); return w; }

static bool read_all(const char *path, std::vector<RealCf> &v)
{
	FILE *f = fopen(path, "rb");
	const bool ok = f && fread(v.data(), sizeof(RealCf), v.size(), f) == v.size();
	if (f) fclose(f);
	return ok;
}

static bool write_all(const char *path, const void *p, size_t bytes)
{
	FILE *f = fopen(path, "wb");
	const bool ok = f && fwrite(p, 1, bytes, f) == bytes;
	return f && fclose(f) == 0 && ok;
}

int main(int argc, char **argv)
{
	const char *mode = argc > 1 ? argv[1] : "";
	if ((!strcmp(mode, "plan") && argc == 5) || (!strcmp(mode, "taps") && argc == 6)) {
		const int32_t fs_r = atoi(argv[2]), base = atoi(argv[3]), freq = atoi(argv[4]);
		if (fs_r < REAL_RATE_MIN || (fs_r & 1) || !real_base_valid(fs_r, base)) { fprintf(stderr, "bad FS_R or BASE\n"); return 2; }
		const int32_t fs = real_equiv_rate(fs_r), centre = real_equiv_centre(fs_r, base), dec = fft_decimation_rate(fs, 1800 * 3);
		const float tbw = relative_transition_bw(fs, 250), shift = real_shift(fs_r, base, freq);
		Plan p0, p;
		if (!plan_block(p0, tbw, dec, 0.f) || !plan_block(p, tbw, dec, shift)) { fprintf(stderr, "planning failed\n"); return 1; }
		float lo, hi;
		real_band(fs_r, base, freq, dec, lo, hi);
		const int32_t Lr = real_taps_length(p0.taps_length);
		if (!strcmp(mode, "plan")) {
			printf("%d %d %d %08x %08x %d %d %d %d %d %d %d %d %d %d %d %08x %08x %08x %08x %08x\n", fs, centre, dec, word(tbw), word(shift), p.n, p.overlap,
					p.input_size, p.pre, p.post, p.m, p.scrap, p.post_input_size, p.taps_length, p.offsetbin, Lr, word(lo), word(hi), word(p.sindelta), word(p.cosdelta), word(p.rate));
			return 0;
		}
		std::vector<std::complex<float>> h((size_t)Lr + 2 * (size_t)p0.taps_length);
		std::vector<float> lp;
		float cut = -1.f;
		real_design_taps(fs_r, base, freq, dec, p0.taps_length, h.data(), h.data() + Lr, lp, cut);       // the function design_channel calls
		return write_all(argv[5], h.data(), sizeof(h[0]) * h.size()) ? 0 : 1;
	}
	if (!strcmp(mode, "pairs") && argc == 3) {
		const int logn = atoi(argv[2]), n = 1 << logn, C = real_chunk(n), G = real_groups(n);
		if (logn < 2 || logn > 24) return 2;
		std::vector<unsigned char> out((size_t)n, 0), in((size_t)n, 0);
		for (int w = 0; w < G; w++) {
			const int lo0 = real_lo0(n, w), hi0 = real_hi0(n, w);
			if ((lo0 & 1) || (hi0 & 1) || (C & 1) || lo0 + C > n / 2 || hi0 < n / 2) { printf("workgroup %d: ranges %d, %d of %d\n", w, lo0, hi0, C); return 1; }
			for (int e = 0; e < C; e++) {
				// what the kernel reads for the mirrors: hi[C - e] = Z[hi0 + C - e] (the last word by real_mirror(n, lo0)) and lo[C - e] = Z[lo0 + C - e]
				const int mlo = e ? hi0 + C - e : real_mirror(n, lo0), mhi = lo0 + C - e;
				if (mlo != real_mirror(n, lo0 + e) || mhi != real_mirror(n, hi0 + e) || mlo < 0 || mlo >= n || mhi < 0 || mhi >= n) { printf("workgroup %d element %d: mirrors %d, %d\n", w, e, mlo, mhi); return 1; }
				out[(size_t)(lo0 + e)]++; out[(size_t)(hi0 + e)]++;
				in[(size_t)mlo]++; in[(size_t)mhi]++;
			}
		}
		for (int i = 0; i < n; i++) if (out[(size_t)i] != 1 || in[(size_t)i] != 1) { printf("bin %d: written %d times, read as a mirror %d times\n", i, out[(size_t)i], in[(size_t)i]); return 1; }
		if (real_mirror(n, 0) != 0 || real_mirror(n, n / 2) != n / 2) return 1;
		printf("ok\n");
		return 0;
	}
	if ((!strcmp(mode, "untangle") || !strcmp(mode, "combine")) && argc == 5) {
		const int logn = atoi(argv[4]), n = 1 << logn;
		const bool comb = mode[0] == 'c';
		if (logn < 2 || logn > 24) return 2;
		std::vector<RealCf> z((size_t)n * (comb ? 2 : 1)), x((size_t)n);
		if (!read_all(argv[2], z)) { fprintf(stderr, "%s: short\n", argv[2]); return 2; }
		for (int k = 0; k < n; k++)
			x[(size_t)k] = comb ? real_tap_combine(z[(size_t)k], z[(size_t)(n + k)], real_twiddle(k, logn))
			                    : real_untangle(z[(size_t)k], z[(size_t)real_mirror(n, k)], real_twiddle(k, logn));
		return write_all(argv[3], x.data(), sizeof(x[0]) * x.size()) ? 0 : 1;
	}
	fprintf(stderr, "usage: %s plan|taps|pairs|untangle|combine ...\n", argv[0]);
	return 2;
}
