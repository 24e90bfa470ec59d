// blanker_sum_check.cpp -- the host build of dumphfdl_amd/csrc/blanker.h: the block power in the documented order, for the tests to set
// against float64 (tests/test_blanker_cpu.py) and against the device's 32 bits (tests/test_gpu_blanker.py).
//   blanker_sum_check FILE N...     FILE: cf32 samples; for every N (a prefix of the file) one line "N depth P-as-hex-bits P k2(14 dB)-as-hex-bits"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "blanker.h"

int main(int argc, char **argv)
{
	if (argc < 3) { fprintf(stderr, "usage: %s FILE N...\n", argv[0]); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	std::vector<float> x;
	float buf[4096];
	size_t got;
	while ((got = fread(buf, sizeof(float), 4096, f)) > 0) x.insert(x.end(), buf, buf + got);
	fclose(f);
	for (int i = 2; i < argc; i++) {
		const long n = atol(argv[i]);
		if (n < 1 || n > hfdl::BLANK_N_MAX || (size_t)(2 * n) > x.size()) { fprintf(stderr, "N = %ld: outside 1 .. %zu\n", n, x.size() / 2); return 2; }
		const float P = hfdl::blank_block_power(x.data(), (int)n), k2 = hfdl::blank_k2(14.0f);
		uint32_t bits, kbits;
		memcpy(&bits, &P, 4);
		memcpy(&kbits, &k2, 4);
		printf("%ld %d %08x %.9g %08x\n", n, hfdl::blank_sum_depth((int)n), bits, (double)P, kbits);
	}
	return 0;
}
