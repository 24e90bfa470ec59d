// quality_check.cpp -- the host build of the frame quality arithmetic (dumphfdl_amd/csrc/quality.h: the per-frame function the device
// runs, over an emulated wave) on frames read from a file.  tests/test_quality_cpu.py builds it with g++ -ffp-contract=off and compares
// its records with the float64 model (tests/quality_f64.py).
//   quality_check IN OUT     IN: int32 nframes, then per frame int32 mode and segments * 30 cf32;  OUT: nframes hfdl_gpu_frame_quality
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define __device__
#define __host__
static const struct { unsigned x; } threadIdx = { 0 };
static inline int atomicAdd(int *p, int v) { int o = *p; *p += v; return o; }
static inline int __popcll(unsigned long long x) { return __builtin_popcountll(x); }
static inline int __popc(unsigned x) { return __builtin_popcount(x); }

#include "../../dumphfdl_amd/csrc/quality.h"
#include "../../dumphfdl_amd/csrc/demod_tables.h"

using namespace hfdl;

int main(int argc, char **argv)
{
	if (argc != 3) { fprintf(stderr, "usage: quality_check IN OUT\n"); return 2; }
	FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
	if (!in || !out) { perror("quality_check"); return 2; }
	static DemodTables t;
	build_demod_tables(t, 0.6912f);
	int32_t nframes = 0;
	if (fread(&nframes, sizeof(nframes), 1, in) != 1 || nframes < 0) return 2;
	std::vector<cf> x((size_t)MAX_DATA_SYMBOLS);
	for (int f = 0; f < nframes; f++) {
		int32_t mode = -1;
		if (fread(&mode, sizeof(mode), 1, in) != 1 || mode < 0 || mode > 7) return 2;
		const size_t nsym = (size_t)mode_params(mode).segments * DATA_FRAME_LEN;
		if (fread(x.data(), sizeof(cf), nsym, in) != nsym) return 2;
		hfdl_gpu_frame_quality q;
		memset(&q, 0, sizeof(q));
		FrameRec fr;
		memset(&fr, 0, sizeof(fr));
		fr.mode = mode; fr.signal_level = 1.0f; fr.noise_floor = 1.0f;
		quality_header(fr, 0, q);
		quality_frame_host(mode, x.data(), &t.psk_pts[0][0], q);
		if (fwrite(&q, sizeof(q), 1, out) != 1) return 2;
	}
	fclose(in);
	return fclose(out) == 0 ? 0 : 2;
}
