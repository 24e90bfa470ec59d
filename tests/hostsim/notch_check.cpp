// notch_check.cpp -- the host build of dumphfdl_amd/csrc/notch.h: the carrier canceller's rule in fp32 and in the documented order, for the
// tests to set against float64 (tests/test_notch_cpu.py) and against the device's 32 bits (tests/test_gpu_notch.py).
//   notch_check rows IN NCH N MU STATE_IN STATE_OUT OUT
//       IN: [NCH][N] cf32, every row a channel's next N samples; STATE_IN: [NCH][NOTCH_STATE_FLOATS] f32, or - for fresh channels;
//       writes the state after the rows and y [NCH][N]; one line per channel:
//       "rec CHANNEL blocks resets in_power out_power tap_energy" (the floats as hex bits)
//   notch_check stream IN MU COUNTS OUT
//       IN: one channel's samples in stream order, cut into rows as COUNTS says -- a file of int32 row lengths, or a number: rows of that
//       many samples, the last one shorter; OUT: y (or - to write nothing); one "rec ROW ..." line per row of a COUNTS file, then
//       "total rows resets finite max_tap_energy tap_energy" (finite: 1 if every output word is finite; the energies as decimals)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "notch.h"

using namespace hfdl;

template <typename T> static bool read_all(const char *path, std::vector<T> &v)
{
	FILE *f = fopen(path, "rb");
	if (!f) { perror(path); return false; }
	T buf[4096];
	size_t got;
	while ((got = fread(buf, sizeof(T), 4096, f)) > 0) v.insert(v.end(), buf, buf + got);
	fclose(f);
	return true;
}

static bool write_all(const char *path, const float *p, size_t n)
{
	FILE *f = fopen(path, "wb");
	if (!f) { perror(path); return false; }
	const bool ok = fwrite(p, sizeof(float), n, f) == n;
	return fclose(f) == 0 && ok;
}

static unsigned bits(float v) { unsigned b; memcpy(&b, &v, 4); return b; }

static void print_rec(long at, const NotchRecord &r)
{
	printf("rec %ld %llu %llu %08x %08x %08x\n", at, r.blocks, r.resets, bits(r.in_power), bits(r.out_power), bits(r.tap_energy));
}

int main(int argc, char **argv)
{
	if (argc == 9 && !strcmp(argv[1], "rows")) {
		const long nch = atol(argv[3]), n = atol(argv[4]);
		const float mu = (float)atof(argv[5]);
		std::vector<float> x, state;
		if (nch < 1 || n < 1 || !read_all(argv[2], x) || x.size() != (size_t)(2 * nch * n)) { fprintf(stderr, "rows: %s does not hold %ld x %ld samples\n", argv[2], nch, n); return 2; }
		if (!strcmp(argv[6], "-")) state.assign((size_t)nch * NOTCH_STATE_FLOATS, 0.0f);
		else if (!read_all(argv[6], state) || state.size() != (size_t)nch * NOTCH_STATE_FLOATS) { fprintf(stderr, "rows: bad state file\n"); return 2; }
		std::vector<float> y(x.size());
		for (long c = 0; c < nch; c++) {
			NotchRecord rec = {};
			notch_row(&state[(size_t)c * NOTCH_STATE_FLOATS], &x[(size_t)(2 * c * n)], n, mu, &y[(size_t)(2 * c * n)], rec);
			print_rec(c, rec);
		}
		return write_all(argv[7], state.data(), state.size()) && write_all(argv[8], y.data(), y.size()) ? 0 : 2;
	}
	if (argc == 6 && !strcmp(argv[1], "stream")) {
		const float mu = (float)atof(argv[3]);
		std::vector<float> x;
		std::vector<int32_t> counts;
		if (!read_all(argv[2], x)) return 2;
		const long total = (long)(x.size() / 2);
		char *end = nullptr;
		const long fixed = strtol(argv[4], &end, 10);
		const bool listed = *end != 0 || fixed < 1;
		if (listed) {
			if (!read_all(argv[4], counts)) return 2;
		} else for (long at = 0; at < total; at += fixed) counts.push_back((int32_t)(total - at < fixed ? total - at : fixed));
		std::vector<float> state(NOTCH_STATE_FLOATS, 0.0f), y(x.size());
		NotchRecord rec = {};
		float top = 0.0f;
		long at = 0, row = 0;
		for (int32_t c : counts) {
			if (c < 0 || at + c > total) { fprintf(stderr, "stream: the rows hold more than the %ld samples of %s\n", total, argv[2]); return 2; }
			notch_row(state.data(), &x[(size_t)(2 * at)], c, mu, &y[(size_t)(2 * at)], rec);
			if (listed) print_rec(row, rec);
			if (!(rec.tap_energy <= top)) top = rec.tap_energy;
			at += c;
			row++;
		}
		bool finite = true;
		for (long i = 0; i < 2 * at; i++) finite = finite && std::isfinite(y[(size_t)i]);
		printf("total %llu %llu %d %.9g %.9g\n", rec.blocks, rec.resets, finite ? 1 : 0, (double)top, (double)rec.tap_energy);
		if (strcmp(argv[5], "-") && !write_all(argv[5], y.data(), (size_t)(2 * at))) return 2;
		return 0;
	}
	fprintf(stderr, "usage: %s rows IN NCH N MU STATE_IN STATE_OUT OUT | stream IN MU COUNTS OUT\n", argv[0]);
	return 2;
}
