// quality.h -- frame quality records (hfdl_gpu_frontend_quality_enable, include/hfdl_gpu.h): what the constellation the burst decoder
// sliced looked like, per frame and per data segment.  The per-frame arithmetic below is written once, for the device and for the host
// (HFDL_FN, as demod_logic.h: tests/hostsim compiles it with g++ behind the same shims); quality_kernels.hip runs it one wave per
// frame, quality_frame_host() runs the same operations in the same order over an emulated wave.
//
// Definitions, per frame of nsym = segments * 30 stored data symbols x[i], fp32:
//   p[i]   the nearest point of the mode's constellation: psk_slice()'s decision, read from psk_pts (BPSK: +1 if x.x > 0, else -1)
//   e[i]   x[i] - p[i]
//   seg_err_power[s] = (sum over the 30 symbols of segment s of |e|^2) / 30 for s < segments, +0.0 above
//   err_power = (sum over s < segments of seg_err_power[s]) / segments;  err_max = max |e[i]|^2
//   sym_power = (sum |x[i]|^2) / nsym;  gain_re + j gain_im = (sum x[i] conj(p[i])) / nsym
// The symbols are taken AS STORED, in front of the descrambler: descrambler and bitmask_lsb multiply a symbol by +-1, every HFDL
// constellation maps onto itself under that, p follows x, and |e|^2, |x|^2 and x conj(p) are unchanged (to the rounding of psk_pts, whose
// opposite points are opposite to within an ulp; exactly for BPSK).
//
// Order of the sums (fixed: results are bit-identical from run to run and do not depend on how the caller pushes or polls):
//   per symbol   ex = x.x - p.x, ey = x.y - p.y;  |e|^2 = fma(ey, ey, ex * ex);  |x|^2 = fma(x.y, x.y, x.x * x.x);
//                Re = fma(x.y, p.y, x.x * p.x);  Im = fma(x.y, p.x, -(x.x * p.y))        -- three roundings at most per term
//   per segment  the 30 terms are added one after the other, i = 0 .. 29, onto +0.0                 -- 30 roundings
//   per lane     lane k of 64 holds segments k, k + 64, k + 128 (a segment the frame lacks counts +0.0):
//                L[k] = ((0 + S[k]) + S[k + 128]) + S[k + 64]; for err_power the S are the seg_err_power values   -- 2 roundings
//   over lanes   six butterfly steps, stride 32, 16, 8, 4, 2, 1: L[k] = L[k] + L[k ^ stride]        -- 6 roundings
//   the means    one division by 30 (seg_err_power), by segments (err_power) or by nsym              -- 1 (err_power: 2) roundings
// Every multiply-add is an explicit fmaf or two separate operations; the kernel object is built without contraction as well.
#pragma once
#include "demod_logic.h"
#include "../../include/hfdl_gpu.h"

namespace hfdl {

constexpr int Q_LANES = 64, Q_LANE_SEGS = 3;
static_assert(Q_LANES * Q_LANE_SEGS >= HFDL_GPU_QUALITY_SEGMENTS_MAX && HFDL_GPU_QUALITY_SEGMENTS_MAX * DATA_FRAME_LEN == MAX_DATA_SYMBOLS
		&& HFDL_GPU_QUALITY_SYMBOLS_MAX == MAX_DATA_SYMBOLS, "a wave holds every segment of the longest frame");
static_assert(sizeof(hfdl_gpu_frame_quality) == 744, "include/hfdl_gpu.h: hfdl_gpu_frame_quality");

struct QualitySums { float err, pow, gre, gim, emax; };      // sums of |e|^2, |x|^2, Re / Im x conj(p); max |e|^2

// one symbol onto its segment's sums
template <class Pts>
HFDL_FN void quality_symbol(QualitySums &s, int arity, cf x, const Pts &pts)
{
	const cf p = pts(psk_entry(arity, gray_dec(psk_slice(arity, x, nullptr, pts))));
	const float ex = x.x - p.x, ey = x.y - p.y;
	const float e2 = fmaf(ey, ey, ex * ex);
	s.err = s.err + e2;
	s.emax = e2 > s.emax ? e2 : s.emax;
	s.pow = s.pow + fmaf(x.y, x.y, x.x * x.x);
	s.gre = s.gre + fmaf(x.y, p.y, x.x * p.x);
	s.gim = s.gim + fmaf(x.y, p.x, -(x.x * p.y));
}

// What lane `lane` brings to the frame's sums: its segments' sums added onto zeros in the order k, k + 128, k + 64, err holding
// seg_err_power values.  sym(i): stored data symbol i of the frame; store(seg, v): seg_err_power[seg] = v, called for every
// seg < HFDL_GPU_QUALITY_SEGMENTS_MAX this lane holds (+0.0 for a segment the frame lacks).
template <class Pts, class Sym, class Store>
HFDL_FN QualitySums quality_lane(int lane, int arity, int segments, const Sym &sym, const Pts &pts, const Store &store)
{
	QualitySums L;
	L.err = L.pow = L.gre = L.gim = L.emax = 0.f;
	for (int jj = 0; jj < Q_LANE_SEGS; jj++) {
		const int seg = lane + Q_LANES * (jj == 0 ? 0 : Q_LANE_SEGS - jj);      // k, k + 128, k + 64
		QualitySums s;
		s.err = s.pow = s.gre = s.gim = s.emax = 0.f;
		if (seg < segments) {
			for (int i = 0; i < DATA_FRAME_LEN; i++) quality_symbol(s, arity, sym(seg * DATA_FRAME_LEN + i), pts);
			s.err = s.err / (float)DATA_FRAME_LEN;
		}
		if (seg < HFDL_GPU_QUALITY_SEGMENTS_MAX) store(seg, s.err);
		L.err = L.err + s.err; L.pow = L.pow + s.pow; L.gre = L.gre + s.gre; L.gim = L.gim + s.gim;
		L.emax = s.emax > L.emax ? s.emax : L.emax;
	}
	return L;
}

// the frame's figures from the sums over all lanes
HFDL_FN void quality_means(const QualitySums &T, int segments, hfdl_gpu_frame_quality &out)
{
	const float nsym = (float)(segments * DATA_FRAME_LEN);
	out.sym_power = T.pow / nsym;
	out.err_power = T.err / (float)segments;
	out.err_max = T.emax;
	out.gain_re = T.gre / nsym;
	out.gain_im = T.gim / nsym;
}

// what a record takes over from the frame's FrameRec, in the burst decoder's own expressions (its PDU carries the same bits)
HFDL_FN void quality_header(const FrameRec &fr, int32_t freq, hfdl_gpu_frame_quality &out)
{
	const ModeParams mp = mode_params(fr.mode);
	out.sample_index = fr.sample_index;
	out.channel = fr.channel; out.freq = freq; out.mode = fr.mode; out.bitmask_lsb = fr.bitmask_lsb;
	out.nsym = mp.segments * DATA_FRAME_LEN; out.segments = mp.segments;
	out.train_bits_bad = fr.train_bad; out.train_bits_total = fr.train_total;
	out.freq_err_hz = fr.freq_err_hz;
	out.rssi_db = 20.0f * log10f(fr.signal_level);
	out.noise_floor_db = 20.0f * log10f(fr.noise_floor);
}

#ifndef __HIPCC__
// The whole frame on the host (the g++ build of tests/hostsim, where HFDL_FN is plain inline): the wave's lanes one after the other, the
// butterfly over an array.  x: the frame's segments * 30 symbols;
// pts: psk_pts of demod_tables.h.  Fills the five figures and seg_err_power, nothing else.
inline void quality_frame_host(int mode, const cf *x, const float *pts, hfdl_gpu_frame_quality &out)
{
	const ModeParams mp = mode_params(mode);
	QualitySums L[Q_LANES];
	auto sym = [x](int i) { return x[i]; };
	auto store = [&out](int seg, float v) { out.seg_err_power[seg] = v; };
	for (int lane = 0; lane < Q_LANES; lane++) L[lane] = quality_lane(lane, mp.arity, mp.segments, sym, PskTable{pts}, store);
	for (int stride = Q_LANES / 2; stride >= 1; stride >>= 1) {
		QualitySums N[Q_LANES];
		for (int k = 0; k < Q_LANES; k++) {
			const QualitySums &a = L[k], &b = L[k ^ stride];
			N[k].err = a.err + b.err; N[k].pow = a.pow + b.pow; N[k].gre = a.gre + b.gre; N[k].gim = a.gim + b.gim;
			N[k].emax = a.emax > b.emax ? a.emax : b.emax;
		}
		for (int k = 0; k < Q_LANES; k++) L[k] = N[k];
	}
	quality_means(L[0], mp.segments, out);
}
#endif

// ---- launcher (quality_kernels.hip): one wave per entry of the frame queue, the grid of the burst decoder of the same launch.
// counts: the ring's [1] records produced, [2] frames dropped, [3] records the host has taken; null: no ring -- frame f writes recs[f]
// (the stage entry).  syms: [ring][MAX_DATA_SYMBOLS] or null.
#ifdef __HIPCC__
void launch_frame_quality(const FrameRec *frames, const int *nframes, int frame_cap, const cf *data, int data_slots, const float *psk_pts,
		const int32_t *freqs, int *counts, hfdl_gpu_frame_quality *recs, cf *syms, int ring, hipStream_t st);
#endif

}  // namespace hfdl
