// real_input.h -- real-sampled input (hfdl_gpu_frontend_create_real): the rule, as plain inline functions host code can call
// (tests/hostsim/real_input_check.cpp does), and the contract of its two kernels (real_kernels.hip, gfx950 only).  DESIGN.md section 4.16
// has the derivation.
//
// A direct-sampling receiver delivers REAL samples x[n] at fs_r; `base` is the RF frequency that appears at 0 Hz in them.  The front end
// is planned as the EQUIVALENT COMPLEX STREAM of half the rate, fs' = fs_r / 2 centred on centre' = base + fs_r / 4: plan_block(fs') gives
// N', overlap', input_size', pre', post', M, scrap, offsetbin and the NCO exactly as for a complex receiver.  A block is 2 input_size' new
// real samples behind 2 overlap' of history; read as interleaved pairs z[n] = x[2n] + j x[2n + 1] that is what the forward FFT's CS16 /
// CF32 loads and its history already do, and Z = FFT_N'(z) is the existing transform.  With W = exp(-2 pi i / 2N') and Z[N'] = Z[0]
//   X[k] = 1/2 [(Z[k] + conj Z[N' - k]) - j W^k (Z[k] - conj Z[N' - k])],   k = 0 .. N' - 1                       (real_untangle)
// is the 2N'-point DFT of the block on its non-negative frequencies (the Nyquist coefficient is dropped: no channel can sit there).  Bin k
// is base + k fs_r / 2N' = centre' + (k - N'/2) fs' / N': the natural order of X is the fftshifted order of the equivalent stream, so X
// goes into the block's spectrum slot as it is and everything behind it is unchanged.
// A channel's taps are designed at the REAL rate by the existing design_bandpass(): L_r = 2 overlap' + 1 of them, pass band
// (f + 1440 - base) / fs_r +- 0.25 / decimation' cycles per sample.  Their 2N'-point transform on bins 0 .. N' - 1 is
//   H[k] = FFT_N'(h_even)[k] + W^k FFT_N'(h_odd)[k],   h_even[m] = h[2m], h_odd[m] = h[2m + 1]
// and the stored word is H[k] / 2 (real_tap_combine): the inverse FFT divides by N', the real transform wants 2N'.
// The twiddle of bin k is one sincospif(k / N'): k / N' is exact in fp32 for every k < 2^24.  fp32 throughout, every product and sum
// written out in one order and never contracted into an FMA.
// Unlike blanker.h, iqbal.h and notch.h this header does NOT promise the host build's words for the spectra and the stored filters: the
// device's twiddle is fp32 sincospif, the host build's a double cos / sin rounded to fp32, and the two may differ in the last bit (the
// forward FFT in front is not bit-reproduced on the host either).  The device is held to float64 at the forward-FFT tests' gates.  What IS
// word for word the host build's: the planner mapping and the time-domain taps (real_design_taps), host arithmetic on both sides.
#pragma once
#include <math.h>
#include <stdint.h>
#include "planner.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HFDL_REAL_HD __host__ __device__
#else
#define HFDL_REAL_HD
#endif

namespace hfdl {

constexpr int32_t REAL_RATE_MIN = 21600;       // fs' >= 10 800: from there up channels decode (include/hfdl_gpu.h)
constexpr int REAL_THREADS = 256;
constexpr int REAL_CHUNK = 2 * REAL_THREADS;   // bins of each member range of a workgroup of the untangle, at most

struct RealCf { float x, y; };                 // a cf32 word on either side

// ---- pair indices.  X[i] needs Z[i] and Z[(N' - i) mod N'].  Workgroup w of real_groups(n) owns the bins lo0 .. lo0 + C - 1 of the lower
// half and hi0 .. hi0 + C - 1 of the upper (C = real_chunk(n)); the mirrors of its lower bins are hi0 + 1 .. hi0 + C -- its upper range
// and one word more -- and those of its upper bins lo0 + 1 .. lo0 + C.  So a workgroup loads two runs of C + 1 words, both ascending and
// both starting on a 16-byte boundary, and stores two runs of C.  k = 0 and k = N'/2 pair with themselves.
HFDL_REAL_HD inline int real_chunk(int n) { return n / 2 < REAL_CHUNK ? n / 2 : REAL_CHUNK; }
HFDL_REAL_HD inline int real_groups(int n) { return n / (2 * real_chunk(n)); }
HFDL_REAL_HD inline int real_lo0(int n, int w) { (void)n; return w * real_chunk(n); }
HFDL_REAL_HD inline int real_hi0(int n, int w) { return n - (w + 1) * real_chunk(n); }
HFDL_REAL_HD inline int real_mirror(int n, int i) { return (n - i) & (n - 1); }

// the twiddle's argument: W^k = (cos pi a, -sin pi a), a = k / N' (exact)
HFDL_REAL_HD inline float real_twiddle_arg(int k, int logn) { return (float)k * (1.0f / (float)(1 << logn)); }
HFDL_REAL_HD inline RealCf real_twiddle(int k, int logn)
{
	const float a = real_twiddle_arg(k, logn);
	RealCf w;
#if defined(__HIP_DEVICE_COMPILE__)
	float s, c;
	sincospif(a, &s, &c);
	w.x = c; w.y = -s;
#else
	w.x = (float)cos(M_PI * (double)a); w.y = (float)-sin(M_PI * (double)a);
#endif
	return w;
}

// X[k] from zk = Z[k], zm = Z[N' - k] and w = W^k
HFDL_REAL_HD inline RealCf real_untangle(RealCf zk, RealCf zm, RealCf w)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const float ax = zk.x + zm.x, ay = zk.y - zm.y;        // Z[k] + conj Z[N' - k]
	const float bx = zk.x - zm.x, by = zk.y + zm.y;        // Z[k] - conj Z[N' - k]
	const float tx = w.x * bx - w.y * by, ty = w.x * by + w.y * bx;       // W^k b
	RealCf o;
	o.x = 0.5f * (ax + ty);                                // a - j t
	o.y = 0.5f * (ay - tx);
	return o;
}

// the stored tap word of bin k from e = FFT(h_even)[k], o = FFT(h_odd)[k] and w = W^k
HFDL_REAL_HD inline RealCf real_tap_combine(RealCf e, RealCf o, RealCf w)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const float tx = w.x * o.x - w.y * o.y, ty = w.x * o.y + w.y * o.x;
	RealCf h;
	h.x = 0.5f * (e.x + tx);
	h.y = 0.5f * (e.y + ty);
	return h;
}

// ---- the planner mapping (host).  fs_r even.
inline int32_t real_equiv_rate(int32_t fs_r) { return fs_r / 2; }
inline int32_t real_equiv_centre(int32_t fs_r, int32_t base) { return base + fs_r / 4; }
// a base whose whole span base .. base + fs_r / 2 (and a carrier 1440 Hz above its top) is an int32, checked in 64 bits BEFORE the centre is formed
inline bool real_base_valid(int32_t fs_r, int32_t base) { return base >= -(1 << 30) && (int64_t)base + fs_r / 2 + 1440 <= INT32_MAX; }
// the equivalent stream's shift of a channel on `freq`, (centre' - (freq + 1440)) / fs' with centre' = base + fs_r / 4 taken exactly:
// where fs_r is a multiple of four this is the very quotient design_channel forms for a complex receiver on (fs', centre')
inline float real_shift(int32_t fs_r, int32_t base, int32_t freq)
{
	return (float)(2 * ((int64_t)base - ((int64_t)freq + 1440)) + fs_r / 2) / (float)fs_r;
}
inline int32_t real_taps_length(int32_t taps_length_eq) { return 2 * taps_length_eq - 1; }        // L_r = 2 overlap' + 1
// the pass band at the real rate, cycles per sample
inline void real_band(int32_t fs_r, int32_t base, int32_t freq, int32_t decimation_eq, float &lowcut, float &highcut)
{
	const float centre = (float)((int64_t)freq + 1440 - (int64_t)base) / (float)fs_r, half_bw = 0.25f / (float)decimation_eq;
	lowcut = centre - half_bw;
	highcut = centre + half_bw;
}
// the even / odd split: h[0 .. 2T - 2] -> out[0 .. T - 1] = h_even, out[T .. 2T - 2] = h_odd, out[2T - 1] = 0 (T = taps_length'), so
// each half is one zero-padded input of the existing N'-point plan
template <typename Cf> inline void real_split_taps(const Cf *h, int32_t taps_length_eq, Cf *out)
{
	const int32_t T = taps_length_eq;
	for (int32_t m = 0; m < T; m++) out[m] = h[2 * m];
	for (int32_t m = 0; m + 1 < T; m++) out[T + m] = h[2 * m + 1];
	out[2 * T - 1] = Cf();
}

// A channel's taps as a real front end designs them, in ONE function that the library (design_channel) and the host build
// (tests/hostsim/real_input_check.cpp) both call, so the words are the same by construction: the band at the real rate, the existing
// design_bandpass() with L_r taps into `full` (L_r words), and the split into `split` (2 T words).  lp / lp_cut: design_bandpass's cache.
inline void real_design_taps(int32_t fs_r, int32_t base, int32_t freq, int32_t decimation_eq, int32_t taps_length_eq,
		std::complex<float> *full, std::complex<float> *split, std::vector<float> &lp, float &lp_cut)
{
	float lo, hi;
	real_band(fs_r, base, freq, decimation_eq, lo, hi);
	design_bandpass(full, real_taps_length(taps_length_eq), lo, hi, lp, lp_cut);
	real_split_taps(full, taps_length_eq, split);
}

#if defined(__HIPCC__)
// What real_untangle_kernel takes: `in` = the unshifted transforms Z of the step's receivers, in_stride apart; `out` = the block's spectrum
// slot, receiver r at + r out_stride.  One launch per step behind pass 3, grid (real_groups(n), receivers).
struct RealUntangleJob { const float2 *in; float2 *out; int64_t in_stride, out_stride; int32_t n, logn, nrx; };
void launch_real_untangle(const RealUntangleJob &job, hipStream_t st, hipEvent_t done);
// What real_tap_combine_kernel takes: e, o = the unshifted N'-point transforms of a channel's even and odd taps; the words H[k] / 2 go to
// padded slot `slot` of the tap buffer in its layout (kernels.h tap_index_f: kind, rows of 2^m_log bins, rs_f floats per alias row).
struct RealTapJob { const float2 *e, *o; float *taps; size_t rs_f; int32_t n, logn, m_log, kind, slot; };
void launch_real_tap_combine(const RealTapJob &job, hipStream_t st);
#endif

}  // namespace hfdl
