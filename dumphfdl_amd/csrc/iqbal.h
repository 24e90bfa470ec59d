// iqbal.h -- the wideband I/Q imbalance and DC corrector's rule, as plain inline functions host code can call (tests/hostsim/iqbal_check.cpp
// does), and the contract of its kernel (iqbal_kernels.hip, gfx950 only).  fp32 throughout, every product and sum written out in one order,
// never contracted into an FMA, so the host build and the device compute the same words.
//
// The model of the defect, per receiver: x = s + kappa conj(s) + m, with s the signal a perfect receiver would have delivered, kappa the
// gain and phase mismatch of the two mixer arms (|kappa| = 0.03 is an image 30 dB down) and m the DC offset.  s is PROPER -- E s^2 = 0,
// which every mix of carriers, noise and modulated signals away from 0 Hz is -- and has no mean.  With sigma^2 = E |s|^2:
//   E x                = m
//   C = E (x - m)^2    = E (s^2 + 2 kappa |s|^2 + kappa^2 conj(s)^2) = 2 kappa sigma^2
//   P = E |x - m|^2    = (1 + |kappa|^2) sigma^2
//   P^2 - |C|^2        = sigma^4 ((1 + |kappa|^2)^2 - 4 |kappa|^2) = sigma^4 (1 - |kappa|^2)^2
//   P + sqrt(P^2 - |C|^2) = 2 sigma^2                         (|kappa| < 1)
//   kappa              = C / (P + sqrt(P^2 - |C|^2))           exactly, whatever sigma
// and with d = x - m:  d - kappa conj(d) = s + kappa conj(s) - kappa conj(s) - |kappa|^2 s = (1 - |kappa|^2) s: the image is gone, the
// signal keeps its phase and loses 0.008 dB at |kappa| = 0.03.  One complex kappa corrects the part of the imbalance that is flat over
// the band; a frequency-dependent part stays.
//
// Block sums.  For the n NEW samples x of a receiver's block -- after the sample-format conversion, after the blanker if it is on -- five
// sums, each in blanker.h's fixed order (chunks of BLANK_CHUNK, BLANK_THREADS threads, BLANK_STEPS pair steps, xor butterfly, wave sums
// pairwise, chunk sums the same way; a sample past the end is (0, 0)):
//   0: re    1: im    2: re re - im im    3: re im + re im    4: re re + im im            (iqbal_terms)
// State.  A = (m, c2, p2): running averages of the block means of x, x^2 and |x|^2, and a block count k.  A block's means B = sums / (float)n
// enter as A <- A + g (B - A), g = max(alpha, 1 / (float)(k + 1)): the cumulative mean first, exponential afterwards.  A block whose sums
// are not all finite does not touch the state (iqbal_update, iqbal_advance).
// Estimate.  C = c2 - m^2, P = p2 - |m|^2, kappa as above (iqbal_estimate).  There is none while no block has been seen, when P is not
// finite or not positive, when P^2 - |C|^2 < 0, or when |C|^2 > 0.25 P^2: |C| = P is a real-valued stream, whose "image" is the signal
// itself, and the rule must never cancel a signal against its own conjugate.  |C| = 0.5 P is |kappa| = 2 - sqrt(3) = 0.268, an image 11 dB
// down: no receiver is that bad.  A block without an estimate is copied word for word and counted as refused.
// Apply.  Block b is corrected with the estimate from the blocks before b alone -- feed-forward, no loop: y = d - kappa conj(d), d = x - m
// (iqbal_apply).  The first block after an enable goes through uncorrected unless the state was seeded.  Because a block's own sums are
// known only when its launch ends, a block with a NaN or Inf in it is still corrected with the estimate before it (its finite samples
// are, a NaN stays one); it is refused only where there was no estimate anyway.  The block after it is corrected from the state before it.
// Seed and hold.  A caller presets (kappa, m): hold = 1 freezes them, a calibrated correction that no block changes; hold = 0 seeds the
// averages as if ONE block with this kappa and m had been seen, of the power of the first block that follows -- that block is
// corrected with the seed as given, and its own means then enter with weight max(alpha, 1 / 2).
//
// The state is per receiver and carried block by block in push order; forward FFTs run strictly one after the other whichever stream they
// are on (planner.h FftOrder), so results do not depend on how blocks are pushed, polled or batched.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "blanker.h"

namespace hfdl {

constexpr float IQBAL_ALPHA_MIN = 1.0f / 1024.0f, IQBAL_ALPHA_MAX = 1.0f;      // include/hfdl_gpu.h; 0 = off
constexpr float IQBAL_KAPPA_MAX = 0.25f;                                       // |kappa| of a seed at most
constexpr uint32_t IQBAL_K_MAX = 1u << 20;                                     // the block count saturates: 1 / (k + 1) is far below IQBAL_ALPHA_MIN there
constexpr int IQBAL_BLOCKS_MAX = 64;                                           // blocks of one hfdl_gpu_iqbal_blocks() call
enum { IQBAL_HAVE_SUMS = 1, IQBAL_SEEDED = 2, IQBAL_HOLD = 4, IQBAL_VALID = 8 };
enum { IQBAL_OFF = 0, IQBAL_REFUSED = 1, IQBAL_CORRECTED = 2 };                // what iqbal_advance says of the block at hand

// What a receiver carries from block to block, and the record of its newest block in the same 80 bytes.
struct IqbalState {
	float m_re, m_im, c2_re, c2_im, p2;        // A
	float seed_re, seed_im;                    // kappa of a seed or a hold (IQBAL_SEEDED / IQBAL_HOLD)
	uint32_t k, flags, gen;                    // blocks in A; IQBAL_*; the seed this state has taken (IqbalSeed::gen)
	uint32_t blocks, refused;                  // blocks that went through the corrector since the first enable, and those of them copied
	float k_re, k_im, d_re, d_im, P;           // what the newest block was corrected with (IQBAL_VALID), and P of that estimate
	uint32_t pad[3];
};
static_assert(sizeof(IqbalState) == 80, "twenty words");

// A preset waiting for the receiver's next block; gen 0 = none, any other value not equal to the state's = take it.
struct IqbalSeed {
	float k_re, k_im, m_re, m_im;
	uint32_t gen, hold, pad[2];
};

inline bool iqbal_alpha_valid(float alpha) { return alpha == 0.f || (alpha >= IQBAL_ALPHA_MIN && alpha <= IQBAL_ALPHA_MAX); }
inline bool iqbal_seed_valid(float k_re, float k_im, float m_re, float m_im)
{
	const double kk = (double)k_re * k_re + (double)k_im * k_im;
	return kk <= (double)IQBAL_KAPPA_MAX * IQBAL_KAPPA_MAX && fabs((double)m_re) <= 3.402823466e38 && fabs((double)m_im) <= 3.402823466e38;      // (a NaN fails each)
}

HFDL_BLANK_HD inline bool iqbal_finite(float v) { return fabsf(v) <= 3.402823466e38f; }

// the five terms of one sample
HFDL_BLANK_HD inline void iqbal_terms(float re, float im, float t[5])
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const float a = re * re, b = im * im, c = re * im;
	t[0] = re; t[1] = im; t[2] = a - b; t[3] = c + c; t[4] = a + b;
}

// y = d - kappa conj(d), d = x - m
HFDL_BLANK_HD inline void iqbal_apply(float re, float im, float k_re, float k_im, float m_re, float m_im, float &y_re, float &y_im)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const float d_re = re - m_re, d_im = im - m_im;
	const float a = k_re * d_re, b = k_im * d_im, c = k_im * d_re, e = k_re * d_im;
	const float i_re = a + b, i_im = c - e;            // kappa conj(d)
	y_re = d_re - i_re;
	y_im = d_im - i_im;
}

// A <- A + g (B - A) with the means B of a block of n samples whose five sums are all finite
HFDL_BLANK_HD inline void iqbal_update(IqbalState &s, const float sum[5], int n, float alpha)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const float fn = (float)n;
	float B[5];
	for (int q = 0; q < 5; q++) B[q] = sum[q] / fn;
	if (s.flags & IQBAL_SEEDED) {
		// the seed becomes one block of this block's own power (about its mean): C = 2 kappa sigma^2, P = (1 + |kappa|^2) sigma^2
		const float a = B[0] * B[0], b = B[1] * B[1];
		const float PB = B[4] - (a + b);
		if (!(PB > 0.f)) return;                       // nothing to weigh the seed with: it stays as it is
		const float kk = s.seed_re * s.seed_re + s.seed_im * s.seed_im;
		const float cn = (2.0f / (1.0f + kk)) * PB;
		const float ma = s.m_re * s.m_re, mb = s.m_im * s.m_im, mc = s.m_re * s.m_im;
		s.c2_re = cn * s.seed_re + (ma - mb);
		s.c2_im = cn * s.seed_im + (mc + mc);
		s.p2 = PB + (ma + mb);
		s.flags &= ~(uint32_t)IQBAL_SEEDED;
	}
	const float r = 1.0f / (float)(s.k + 1u), g = alpha > r ? alpha : r;
	float *A = &s.m_re;
	for (int q = 0; q < 5; q++) {
		const float d = B[q] - A[q], p = g * d;
		A[q] = A[q] + p;
	}
	if (s.k < IQBAL_K_MAX) s.k++;
}

// (kappa, m, P) of the state; false: there is no estimate (kappa = 0 then)
HFDL_BLANK_HD inline bool iqbal_estimate(const IqbalState &s, float &k_re, float &k_im, float &m_re, float &m_im, float &P)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	m_re = s.m_re; m_im = s.m_im; k_re = 0.f; k_im = 0.f; P = 0.f;
	if (s.flags & (IQBAL_SEEDED | IQBAL_HOLD)) { k_re = s.seed_re; k_im = s.seed_im; return true; }
	if (s.k == 0) return false;
	const float a = m_re * m_re, b = m_im * m_im, c = m_re * m_im;
	const float C_re = s.c2_re - (a - b), C_im = s.c2_im - (c + c);
	P = s.p2 - (a + b);
	if (!(P > 0.f) || !iqbal_finite(P)) return false;
	const float e = C_re * C_re, f = C_im * C_im;
	const float cc = e + f, PP = P * P, D = PP - cc;
	if (!(D >= 0.f) || cc > 0.25f * PP) return false;
	const float den = P + sqrtf(D);
	k_re = C_re / den;
	k_im = C_im / den;
	return true;
}

// does the step read the sums of the block before?  (uniform over a receiver's workgroups: asked of the state that block left)
HFDL_BLANK_HD inline bool iqbal_reads_sums(const IqbalState &s, float alpha, bool restart)
{
	return !restart && alpha > 0.f && (s.flags & IQBAL_HAVE_SUMS) && !(s.flags & IQBAL_HOLD);
}

// One step of a receiver's state: `s` as the block before left it becomes what this block leaves; prev = that block's five sums (read
// only where iqbal_reads_sums()); restart = the first block after an enable; sd = the receiver's seed slot.  Returns IQBAL_* and what
// to correct the block with.
HFDL_BLANK_HD inline int iqbal_advance(IqbalState &s, const float prev[5], int n, float alpha, bool restart, const IqbalSeed &sd,
		float &k_re, float &k_im, float &m_re, float &m_im)
{
	const bool on = alpha > 0.f, use = iqbal_reads_sums(s, alpha, restart);
	if (restart || !on) {
		IqbalState fresh;
		memset(&fresh, 0, sizeof(fresh));
		fresh.blocks = s.blocks; fresh.refused = s.refused;
		s = fresh;
	}
	float P = 0.f;
	k_re = k_im = m_re = m_im = 0.f;
	if (!on) return IQBAL_OFF;
	if (use && iqbal_finite(prev[0]) && iqbal_finite(prev[1]) && iqbal_finite(prev[2]) && iqbal_finite(prev[3]) && iqbal_finite(prev[4]))
		iqbal_update(s, prev, n, alpha);
	if (sd.gen != s.gen) {
		s.gen = sd.gen;
		if (sd.gen != 0) {
			s.m_re = sd.m_re; s.m_im = sd.m_im; s.c2_re = 0.f; s.c2_im = 0.f; s.p2 = 0.f;
			s.seed_re = sd.k_re; s.seed_im = sd.k_im;
			s.k = 1;
			s.flags = sd.hold ? IQBAL_HOLD : IQBAL_SEEDED;
		}
	}
	const bool valid = iqbal_estimate(s, k_re, k_im, m_re, m_im, P);
	s.flags = (s.flags & ~(uint32_t)IQBAL_VALID) | IQBAL_HAVE_SUMS | (valid ? IQBAL_VALID : 0);
	s.blocks++;
	if (!valid) s.refused++;
	s.k_re = k_re; s.k_im = k_im; s.d_re = m_re; s.d_im = m_im; s.P = P;
	return valid ? IQBAL_CORRECTED : IQBAL_REFUSED;
}

// ---- the whole order on the host

// the five sums of x = n converted samples (interleaved re, im), 1 <= n <= BLANK_N_MAX, in blanker.h's order
inline void iqbal_block_sums(const float *x, int n, float sum[5])
{
	const int G = blank_chunks(n);
	static thread_local float fin[5][BLANK_THREADS], v[5][BLANK_THREADS];
	for (int q = 0; q < 5; q++) for (int t = 0; t < BLANK_THREADS; t++) fin[q][t] = 0.0f;
	for (int w = 0; w < G; w++) {
		for (int t = 0; t < BLANK_THREADS; t++) {
			float acc[5] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
			for (int j = 0; j < BLANK_STEPS; j++) {
				const int64_t a = (int64_t)w * BLANK_CHUNK + 2 * BLANK_THREADS * j + 2 * t;
				float tu[5], tv[5];
				iqbal_terms(a < n ? x[2 * a] : 0.0f, a < n ? x[2 * a + 1] : 0.0f, tu);
				iqbal_terms(a + 1 < n ? x[2 * a + 2] : 0.0f, a + 1 < n ? x[2 * a + 3] : 0.0f, tv);
				for (int q = 0; q < 5; q++) acc[q] = acc[q] + (tu[q] + tv[q]);
			}
			for (int q = 0; q < 5; q++) v[q][t] = acc[q];
		}
		for (int q = 0; q < 5; q++) fin[q][w % BLANK_THREADS] = fin[q][w % BLANK_THREADS] + blank_tree256(v[q]);
	}
	for (int q = 0; q < 5; q++) sum[q] = blank_tree256(fin[q]);
}

// One block of one receiver as the kernel treats it: s and sum as the block before left them (sum: its five sums) become this block's;
// x = n converted samples, y = what enters the transform (y == x is fine).  Returns IQBAL_*.
inline int iqbal_block(IqbalState &s, float sum[5], const IqbalSeed &sd, float alpha, bool restart, const float *x, int n, float *y)
{
	float k_re, k_im, m_re, m_im, now[5];
	const int mode = iqbal_advance(s, sum, n, alpha, restart, sd, k_re, k_im, m_re, m_im);
	iqbal_block_sums(x, n, now);
	for (int i = 0; i < n; i++) {
		if (mode == IQBAL_CORRECTED) iqbal_apply(x[2 * i], x[2 * i + 1], k_re, k_im, m_re, m_im, y[2 * i], y[2 * i + 1]);
		else if (y != x) memcpy(y + 2 * i, x + 2 * i, 2 * sizeof(float));
	}
	memcpy(sum, now, sizeof(now));
	return mode;
}

// the image rejection an estimate implies, in dB: the image of the uncorrected stream lies |kappa|^2 below its signal
inline float iqbal_image_rejection_db(float k_re, float k_im)
{
	const double kk = (double)k_re * k_re + (double)k_im * k_im;
	return kk > 0.0 ? (float)(-10.0 * log10(kk)) : HUGE_VALF;
}

// a state as the record of its newest block (Stats = hfdl_gpu_iqbal_stats of include/hfdl_gpu.h)
template <typename Stats> inline void iqbal_stats_of(const IqbalState &s, Stats *out)
{
	memset(out, 0, sizeof(*out));
	out->blocks = s.blocks;
	out->refused = s.refused;
	out->kappa_re = s.k_re; out->kappa_im = s.k_im; out->dc_re = s.d_re; out->dc_im = s.d_im; out->power = s.P;
	out->valid = (s.flags & IQBAL_VALID) != 0;
	out->hold = (s.flags & IQBAL_HOLD) != 0;
	out->image_rejection_db = out->valid ? iqbal_image_rejection_db(s.k_re, s.k_im) : 0.f;
}

#if defined(__HIPCC__)
// One block of every receiver: receiver r reads n samples of format `fmt` at fresh[r] and leaves them, corrected (or copied: alpha[r] = 0,
// or no estimate), as cf32 at out + r * out_stride -- which may be where it read them, if they are cf32.  State and chunk sums live in
// two slots: this launch reads slot ^ 1 and writes slot, so no workgroup reads what another writes.
struct IqbalJob {
	const void *fresh[64] = {};         // (RECEIVERS_MAX of kernels.h)
	float alpha[64] = {};
	float2 *out = nullptr;
	int64_t out_stride = 0;
	float *partial = nullptr;           // [2][nrx][5][blank_chunks(n)]
	IqbalState *state = nullptr;        // [2][nrx]
	const IqbalSeed *seed = nullptr;    // [nrx]
	uint64_t restart = 0;               // bit r: receiver r starts afresh with this block
	int32_t n = 0, nrx = 1, fmt = 0, slot = 0;
};

// one launch on `st`, grid (chunks, receiver); `done` (optional) rides on the dispatch (hipExtLaunchKernelGGL): no barrier packet
void launch_iqbal(const IqbalJob &job, hipStream_t st, hipEvent_t done = nullptr);
#endif

}  // namespace hfdl
