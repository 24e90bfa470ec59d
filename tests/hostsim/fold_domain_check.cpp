// fold_domain_check.cpp -- host-side check of csrc/fold_domain.h, the index maps of the fold in the mixed FFT domain.  Compiled and run by
// tests/test_fold_mixed_domain_cpu.py (no GPU).
//   no argument: for every register-resident plan (l1, l2, l3 in 6 .. 8) and every log2(M) the predicate admits
//     * mixed_bin / natural_bin are inverse bijections of [0, M); sixteen consecutive j' are sixteen adjacent k2 of one k1
//     * (k2hi, n3) -> rho is a bijection onto [0, N / M); the tap row of (k2, n3) is the block's row of (k2, -n3 mod R3)
//     * every element (k1, k2, n3) of pass 2's output lands on its own cell of [g][rho][16], and that cell is the one the fold kernel reads for
//       (row rho, bin j'): rho * 16 + (j' / 16) * 16 pre + j' % 16 -- spelled here the way fft_rpass2 computes it (shifts of kb = k2 / 16)
//     and the predicate refuses what it must (a radix outside 64 .. 256, fewer than sixteen k2 per group, a k3 bit in the bin, a pruned fold).
//     Prints "<cells checked> ok" or the first violation.
//   `dump l1 l2 l3 logm`: one line "j j'" per bin, then one line "k2 n3 rho taprow" per (k2, n3): what the numpy model of the test is held to.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "fold_domain.h"

using namespace hfdl;

static int check(int l1, int l2, int l3, int logm, unsigned long long &cells)
{
	const int q = logm - l1, m = 1 << logm, r3 = 1 << l3, r2 = 1 << l2, r1 = 1 << l1, pre_log = l2 - q + l3, pre = 1 << pre_log;
	std::vector<char> seen((size_t)m, 0);
	for (int j = 0; j < m; j++) {
		const int jp = mixed_bin(j, l1);
		if (jp < 0 || jp >= m || seen[(size_t)jp]) { printf("bins: not a bijection at j %d (l1 %d logm %d)\n", j, l1, logm); return 1; }
		seen[(size_t)jp] = 1;
		if (natural_bin(jp, l1) != j) { printf("bins: natural_bin(mixed_bin(%d)) != %d\n", j, j); return 1; }
		// a group of sixteen: one k1, sixteen adjacent k2
		const int k1 = j & (r1 - 1), k2lo = j >> l1;
		if ((jp & 15) != (k2lo & 15) || (jp >> 4) != (k1 | ((k2lo >> 4) << l1))) { printf("bins: group order broken at j %d\n", j); return 1; }
	}
	if (mixed_bin(5, 0) != 5 || natural_bin(5, 0) != 5) { printf("l1 = 0 is not the identity\n"); return 1; }
	std::vector<char> cell((size_t)1 << (l1 + l2 + l3), 0);
	const int qh = q - 4;
	for (int k1 = 0; k1 < r1; k1++)
		for (int k2 = 0; k2 < r2; k2++)
			for (int n3 = 0; n3 < r3; n3++) {
				const int rho = mixed_row(k2, n3, q, l3), jp = mixed_bin(natural_bin_of(k1, k2, q, l1), l1);
				if (rho < 0 || rho >= pre) { printf("rows: rho %d outside [0, %d)\n", rho, pre); return 1; }
				if (mixed_tap_row(k2, n3, q, l3) != mixed_row(k2, (r3 - n3) % r3, q, l3)) { printf("rows: tap row of (%d, %d)\n", k2, n3); return 1; }
				// what the fold reads for (row rho, bin j')
				const size_t want = (size_t)rho * 16 + (size_t)(jp >> 4) * 16 * (size_t)pre + (size_t)(jp & 15);
				// what pass 2 stores: k2 = ka + 16 kb
				const int ka = k2 & 15, kb = k2 >> 4;
				const size_t got = ((size_t)k1 << (pre_log + 4)) + (size_t)n3 * 16 + (size_t)ka
					+ ((size_t)(kb & ((1 << qh) - 1)) << (l1 + pre_log + 4)) + ((size_t)(kb >> qh) << (l3 + 4));
				if (got != want || got >= cell.size() || cell[got]) { printf("cells: (%d, %d, %d) -> %zu, the fold reads %zu (l %d %d %d logm %d)\n", k1, k2, n3, got, want, l1, l2, l3, logm); return 1; }
				cell[got] = 1;
				cells++;
			}
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 6 && !strcmp(argv[1], "dump")) {
		const int l1 = atoi(argv[2]), l2 = atoi(argv[3]), l3 = atoi(argv[4]), logm = atoi(argv[5]), q = logm - l1;
		(void)l2;
		for (int j = 0; j < (1 << logm); j++) printf("%d %d\n", j, mixed_bin(j, l1));
		for (int k2 = 0; k2 < (1 << l2); k2++)
			for (int n3 = 0; n3 < (1 << l3); n3++) printf("%d %d %d %d\n", k2, n3, mixed_row(k2, n3, q, l3), mixed_tap_row(k2, n3, q, l3));
		return 0;
	}
	unsigned long long cells = 0;
	int plans = 0;
	for (int l1 = 6; l1 <= 8; l1++)
		for (int l2 = 6; l2 <= 8; l2++)
			for (int l3 = 6; l3 <= 8; l3++) {
				if (l1 + l2 + l3 > 22 && !(l1 == 8 && l2 == 8 && l3 >= 7)) continue;      // the large ones: the plans the library builds (2^23: 8 8 7, 2^24: 8 8 8)
				for (int logm = 4; logm <= 13; logm++) {
					const bool fits = mixed_fold_fits(l1, l2, l3, logm, false);
					if (fits != (logm - l1 >= 4 && logm <= l1 + l2)) { printf("predicate wrong at %d %d %d logm %d\n", l1, l2, l3, logm); return 1; }
					if (!fits) continue;
					// every admissible M up to N = 2^19; beyond, the two ends of the range and the 4096 bins of the large geometries
					if (l1 + l2 + l3 > 19 && logm != l1 + 4 && logm != 12 && logm != l1 + l2 && logm != 13) continue;
					if (check(l1, l2, l3, logm, cells)) return 1;
					plans++;
				}
			}
	if (mixed_fold_fits(8, 8, 7, 12, true) || mixed_fold_fits(5, 8, 8, 12, false) || mixed_fold_fits(8, 9, 7, 12, false) || mixed_fold_fits(8, 8, 5, 12, false)
			|| mixed_fold_fits(8, 8, 7, 11, false) || mixed_fold_fits(6, 6, 6, 13, false) || !mixed_fold_fits(8, 8, 7, 12, false) || !mixed_fold_fits(6, 6, 6, 11, false)) {
		printf("predicate wrong at a named case\n");
		return 1;
	}
	printf("%llu cells of %d plans ok\n", cells, plans);
	return 0;
}
