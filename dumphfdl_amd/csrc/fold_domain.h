// fold_domain.h -- the index maps of the fold in the MIXED domain: plain integer functions, for the kernels and for a
// host build alike (tests/hostsim/fold_domain_check.cpp includes this file and nothing else of the library).
//
// The forward FFT is N = R1 R2 R3 in three passes, k = k1 + R1 k2 + R1 R2 k3.  The fold adds, per channel, H[k] X[k] over all k with one
// k mod M.  With log2(M) = l1 + q, 4 <= q <= l2, that is k1 and the low q bits of k2 held fixed and a sum over the high bits of k2
// (k2hi) and ALL of k3 -- and pass 3 is a plain R3-point DFT over n3 at fixed (k1, k2), so by Parseval's relation for the DFT
//     sum_k3 H[k1,k2,k3] X[k1,k2,k3]  =  R3 sum_n3 T[k1,k2,(-n3) mod R3] Z[k1,k2,n3]
// with Z / T what pass 2 leaves of the block / of the channel's taps.  The fold contracts over the rows rho = (k2hi, n3) of pass 2's
// output instead of the rows a = (k2hi, k3) of pass 3's, and pass 3 is never run.
//   bins:  j = k1 + R1 k2lo (natural, what the inverse FFT wants)  <->  j' = 16 g + (k2lo & 15), the sixteen bins of a fold workgroup
//          being sixteen adjacent k2 of one k1 -- which is what a pass-2 workgroup holds.  g = k1 + R1 (k2lo >> 4).
//   rows:  rho = k2hi R3 + n3; the taps sit at rho = k2hi R3 + (-n3 mod R3), scaled by R3 (a power of two: exact)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HFDL_FOLD_HD __host__ __device__
#else
#define HFDL_FOLD_HD
#endif

namespace hfdl {

// natural bin j -> position j' in group order.  The low l1 + 4 bits (k1, then the low four bits of k2) are rotated: (k2 & 15, then k1).
// l1 = 0: the identity (the fold in the spectrum domain).
HFDL_FOLD_HD inline int mixed_bin(int j, int l1)
{
	if (l1 == 0) return j;
	const int mask = (1 << (l1 + 4)) - 1, f = j & mask;
	return (j & ~mask) | ((f & ((1 << l1) - 1)) << 4) | (f >> l1);
}
// ... and back
HFDL_FOLD_HD inline int natural_bin(int jp, int l1)
{
	if (l1 == 0) return jp;
	const int mask = (1 << (l1 + 4)) - 1, f = jp & mask;
	return (jp & ~mask) | ((f & 15) << l1) | (f >> 4);
}
// row of (k2, n3): q = log2(M) - l1 low bits of k2 belong to the bin
HFDL_FOLD_HD inline int mixed_row(int k2, int n3, int q, int l3) { return ((k2 >> q) << l3) | n3; }
// natural bin of (k1, k2)
HFDL_FOLD_HD inline int natural_bin_of(int k1, int k2, int q, int l1) { return k1 | ((k2 & ((1 << q) - 1)) << l1); }
// the row the taps of (k2, n3) are stored at: the block's row of (k2, -n3)
HFDL_FOLD_HD inline int mixed_tap_row(int k2, int n3, int q, int l3) { return mixed_row(k2, (-n3) & ((1 << l3) - 1), q, l3); }

// Where the front end folds in the mixed domain: the register-resident plan (every radix 64 .. 256), at least sixteen k2 per bin group,
// no k3 bit inside a bin, every alias row folded (the pruned fold's row windows live in a = (k2hi, k3))
HFDL_FOLD_HD inline bool mixed_fold_fits(int l1, int l2, int l3, int logm, bool pruned)
{
	const bool fast = l1 >= 6 && l1 <= 8 && l2 >= 6 && l2 <= 8 && l3 >= 6 && l3 <= 8;
	return fast && logm - l1 >= 4 && logm <= l1 + l2 && !pruned;
}

}  // namespace hfdl
