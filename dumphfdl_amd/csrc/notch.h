// notch.h -- the per-channel adaptive carrier canceller's rule, as plain inline functions host code can call (tests/hostsim/notch_check.cpp
// does), and the contract of its kernel (notch_kernels.hip, gfx950 only).
//
// A normalised-LMS line canceller: the channel's own past, D samples back, predicts what is steady in it (a carrier), and the prediction
// is taken away.  For a selected channel, x[n] are its channelizer output samples in stream order, continuing across blocks.  The state
// is L = 32 complex taps w_k and the last D + L - 1 = 55 inputs, D = 24; all zero when the channel is enabled or retuned.  In fp32:
//   u_k[n] = x[n - D - k]                  k = 0 .. L - 1 (zero before the start)
//   s[n]   = sum_k conj(w_k) u_k[n]        per tap: re = wr ur + wi ui, im = wr ui - wi ur (notch_products), then the sum below
//   y[n]   = x[n] - s[n]                   what the demodulator reads
//   P[n]   = sum_k |u_k[n]|^2              per tap: ur ur + ui ui (notch_power_of), then the sum below
//   g      = mu / P[n],  t = g y[n]        one correctly rounded division, two products
//   w_k   += conj(t) u_k[n]                re += tr ur + ti ui, im += tr ui - ti ur (notch_update)
//                                          only if 0 < P[n] < Inf and both parts of y[n] are finite (notch_ok)
// Every product is rounded on its own: nothing is contracted into an FMA, on the device (the object is built with -ffp-contract=off) or
// here.  No tap leakage: ten million samples of noise, with and without a tone, leave sum |w|^2 far below the bound.
//
// The order of the three sums over k, a fixed function of L = 32: a binary tree over adjacent taps -- level m = 1, 2, 4, 8, 16 replaces
// v_k by v_k + v_(k xor m).  On the device lanes are taps and a level is one cross-lane move and one addition in every lane; both lanes
// of a pair compute a + b and b + a, the same 32 bits, so after five levels every lane holds the same sum without a broadcast
// (notch_tree32 is that tree on the host).
//
// No stuck state.  At the end of every row (a channel's samples of one block), E = sum_k |w_k|^2 in the same order; if E is not finite
// or exceeds NOTCH_RESET = 4 the taps are set to zero and the event is counted (a tracked tone gives about 1 / L per tone).  Together
// with the guard on the update no input can leave a channel stuck: a NaN or Inf sample never reaches the taps, spoils the output while
// it is in the delay line (the 32 samples from D after it on, the last D + L - 1 = 55 after it), and the 56th sample after it is normal
// again.  The reset is also what ends the one runaway met in practice: a front end's very first block starts with the channel filter's
// start-up ramp, some 60 samples rising from 1e-9 to the signal's level, P is 24 samples behind the sample it normalises for, and the
// taps reach sum |w|^2 of a few hundred within the row (tests/test_gpu_notch.py pins the one reset it costs).
//
// What the rest of the front end sees: the channel export and stage tap 3 read the channelizer's own output, the raw channel; the
// spectrum monitor sits in front of the channelizer and sees nothing of it; demodulator, burst decoder and the frame quality records
// see the cancelled samples.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HFDL_NOTCH_HD __host__ __device__
#else
#define HFDL_NOTCH_HD
#endif

namespace hfdl {

constexpr int NOTCH_L = 32;                                     // taps
constexpr int NOTCH_D = 24;                                     // decorrelation delay in samples
constexpr int NOTCH_HIST = NOTCH_D + NOTCH_L - 1;               // inputs kept
// a channel's state: w_k as (re, im), k = 0 .. 31, then the last 55 inputs as (re, im), NEWEST FIRST (include/hfdl_gpu.h names the size)
constexpr int NOTCH_STATE_FLOATS = 2 * NOTCH_L + 2 * NOTCH_HIST;
constexpr float NOTCH_MU_MIN = 1e-5f, NOTCH_MU_MAX = 0.05f;      // include/hfdl_gpu.h
constexpr float NOTCH_RESET = 4.0f;                             // sum |w|^2 above this (or not finite) at the end of a row: taps to zero

inline bool notch_mu_valid(float mu) { return mu >= NOTCH_MU_MIN && mu <= NOTCH_MU_MAX; }      // (false for NaN)

// What the canceller leaves per channel.  One writer: the wave that owns the channel.
struct NotchRecord {
	unsigned long long blocks, resets;  // rows cancelled and tap resets since the record was cleared
	float in_power, out_power;          // sum |x|^2 and sum |y|^2 of the newest row: from 0.0f, one sample after the other
	float tap_energy;                   // E of the newest row, as found (before a reset)
	float pad;
};

HFDL_NOTCH_HD inline float notch_power_of(float re, float im)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const float a = re * re, b = im * im;
	return a + b;
}

// conj(w) u
HFDL_NOTCH_HD inline void notch_products(float wr, float wi, float ur, float ui, float &pr, float &pi)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const float a = wr * ur, b = wi * ui, c = wr * ui, d = wi * ur;
	pr = a + b;
	pi = c - d;
}

HFDL_NOTCH_HD inline bool notch_finite(float v) { return fabsf(v) <= 3.402823466e38f; }
HFDL_NOTCH_HD inline bool notch_ok(float P, float yr, float yi) { return P > 0.0f && notch_finite(P) && notch_finite(yr) && notch_finite(yi); }

// w += conj(t) u
HFDL_NOTCH_HD inline void notch_update(float &wr, float &wi, float tr, float ti, float ur, float ui)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const float a = tr * ur, b = ti * ui, c = tr * ui, d = ti * ur;
	const float e = a + b, f = c - d;
	wr = wr + e;
	wi = wi + f;
}

// the tree on the host: v[0 .. 31] -> the sum (v is overwritten; every entry ends up holding it)
inline float notch_tree32(float *v)
{
	for (int m = 1; m < NOTCH_L; m <<= 1)
		for (int k = 0; k < NOTCH_L; k++)
			if (!(k & m)) { const float s = v[k] + v[k | m]; v[k] = s; v[k | m] = s; }
	return v[0];
}

// One row on the host: n samples x (interleaved re, im) of a channel whose state is `state` (NOTCH_STATE_FLOATS, updated) -> y; the
// record is updated as the kernel updates it.  n >= 0.
inline void notch_row(float *state, const float *x, int64_t n, float mu, float *y, NotchRecord &rec)
{
	float *w = state, *hist = state + 2 * NOTCH_L;
	float line[2 * NOTCH_HIST];         // a ring of the last 55 inputs: sample n - j at ((head - j) mod 55), head = newest
	for (int j = 0; j < NOTCH_HIST; j++) { line[2 * (NOTCH_HIST - 1 - j)] = hist[2 * j]; line[2 * (NOTCH_HIST - 1 - j) + 1] = hist[2 * j + 1]; }
	int head = NOTCH_HIST - 1;
	float pin = 0.0f, pout = 0.0f;
	float ur[NOTCH_L], ui[NOTCH_L], pr[NOTCH_L], pi[NOTCH_L], pp[NOTCH_L];
	for (int64_t i = 0; i < n; i++) {
		const float xr = x[2 * i], xi = x[2 * i + 1];
		for (int k = 0; k < NOTCH_L; k++) {
			// x[n - D - k]: the newest kept input is x[n - 1]
			int at = head - (NOTCH_D - 1) - k;
			if (at < 0) at += NOTCH_HIST;
			ur[k] = line[2 * at]; ui[k] = line[2 * at + 1];
			notch_products(w[2 * k], w[2 * k + 1], ur[k], ui[k], pr[k], pi[k]);
			pp[k] = notch_power_of(ur[k], ui[k]);
		}
		const float sr = notch_tree32(pr), si = notch_tree32(pi), P = notch_tree32(pp);
		const float yr = xr - sr, yi = xi - si;
		if (notch_ok(P, yr, yi)) {
			const float g = mu / P, tr = g * yr, ti = g * yi;
			for (int k = 0; k < NOTCH_L; k++) notch_update(w[2 * k], w[2 * k + 1], tr, ti, ur[k], ui[k]);
		}
		y[2 * i] = yr; y[2 * i + 1] = yi;
		pin = pin + notch_power_of(xr, xi);
		pout = pout + notch_power_of(yr, yi);
		head = head + 1 == NOTCH_HIST ? 0 : head + 1;
		line[2 * head] = xr; line[2 * head + 1] = xi;
	}
	for (int j = 0; j < NOTCH_HIST; j++) {
		int at = head - j;
		if (at < 0) at += NOTCH_HIST;
		hist[2 * j] = line[2 * at]; hist[2 * j + 1] = line[2 * at + 1];
	}
	for (int k = 0; k < NOTCH_L; k++) pp[k] = notch_power_of(w[2 * k], w[2 * k + 1]);
	const float E = notch_tree32(pp);
	rec.blocks++;
	rec.in_power = pin; rec.out_power = pout; rec.tap_energy = E;
	if (!(E <= NOTCH_RESET)) {
		for (int k = 0; k < 2 * NOTCH_L; k++) w[k] = 0.0f;
		rec.resets++;
	}
}

#if defined(__HIPCC__)
// A run of `nblk` consecutive blocks: the rows in [nblk][nch][outs], the rows' lengths cnt [nblk][nch] (null: every row holds `outs`),
// out of the same shape.  Only the selected channels' rows are written: sel [nsel] (null: channels 0 .. nsel - 1).  state [nch]
// [NOTCH_STATE_FLOATS] and rec [nch] are indexed by channel.
struct NotchJob {
	const float2 *in = nullptr;
	float2 *out = nullptr;
	const int *cnt = nullptr;
	const int32_t *sel = nullptr;
	float *state = nullptr;
	NotchRecord *rec = nullptr;
	int32_t nch = 0, outs = 0, nblk = 0, nsel = 0;
	float mu = 0.f;
};

// one launch on `st`, one wave per two selected channels; `done` (optional) rides on the dispatch: no barrier packet
void launch_notch(const NotchJob &job, hipStream_t st, hipEvent_t done = nullptr);
#endif

}  // namespace hfdl
