// fft_kernels.hip -- wideband forward FFT for the overlap-and-scrap channelizer (gfx950).
//
// Replaces fft_thread's overlap assembly + csdr_fft_execute(fwd) + fft_swap_sides
// (reference src/fft.c:49-59, src/fft_fftw.c:39-41, src/fastddc.c:102-112).
//
// N = R1*R2*R3 (each <= 256).  Three launches, each workgroup holds a tile of 16 columns x R points in
// LDS, runs an in-place radix-4 DIF (result bit-reversed, undone on the way out) and applies the
// inter-pass twiddle while storing.  Global accesses are 128-byte runs (16 adjacent columns of cf32);
// the overlap history and the fftshift are index remaps on the first load / last store, never a pass.
// Where the front end folds in the mixed domain (fold_domain.h) a block's transform ends with pass 2, which then stores the fold's operand
// (fft_rpass2, mix_out); pass 3 runs on demand alone: for the spectrum monitor and for the stage taps that read a spectrum or a filter.
#include <hip/hip_ext.h>
#include "kernels.h"
#include "retune_launch.h"
#include "fft_core.h"
#include "fft_regs.h"

namespace hfdl {

// raw sample -> float complex with the reference's scaling: convert_cf32 / convert_cs16 / convert_cu8
// (src/input-helpers.c:10-78; full scale 1.0 / 32767.5 / 127, cu8 offset = full_scale / 2 as written there)
template <int FMT>
__device__ __forceinline__ float2 load_sample(const void *__restrict__ raw, int i)
{
	if (FMT == SFMT_CS16) {
		const short2 v = ((const short2 *)raw)[i];
		return make_float2((float)v.x / 32767.5f, (float)v.y / 32767.5f);
	} else if (FMT == SFMT_CU8) {
		const uchar2 v = ((const uchar2 *)raw)[i];
		return make_float2(((float)v.x - 63.5f) / 127.0f, ((float)v.y - 63.5f) / 127.0f);
	}
	return ((const float2 *)raw)[i];
}

// last-pass store: plain index, or (the transform is a channel's filter) straight into the matrix-operand tap layout
__device__ __forceinline__ void store_out(float2 *out, const FftOutLayout &lay, unsigned i, size_t at, float2 v)
{
	if (lay.kind == TAPL_PLAIN) { out[at] = v; return; }
	float *o = (float *)out + tap_index_f(lay.kind, 1 << lay.row_log, (size_t)(2 * lay.row_stride), lay.chan, (int)(i >> lay.row_log), (int)(i & ((1u << lay.row_log) - 1u)), 0);
	o[0] = v.x;
	o[4] = v.y;              // Im sits one lane on: four floats
}

// pass 1: columns c = n2*R3+n3 (stride R2*R3 between the R1 samples of a column).  Input is the
// virtual concatenation [hist(split) , fresh(n-split)] -- the overlap assembly of src/fft.c:49-54.
// The last `split` samples of the block are the next block's history: they are written to `hist_next` (a second buffer,
// never the one being read) as they pass through, so no separate copy runs.
template <int FMT>
__global__ __launch_bounds__(FFT_THREADS) void fft_pass1(const float2 *__restrict__ hist, FftInputs in,
		int split, float2 *__restrict__ hist_next, float2 *__restrict__ out, FftPlan p, NcoJob job, int riders)
{
	// rider workgroups come FIRST in the grid: dispatched at once, they run beside the whole pass (at the end of the grid they would start when the pass is nearly over)
	if ((int)blockIdx.x < riders) { if (blockIdx.y == 0) nco_table_segment(job, (int)blockIdx.x * FFT_THREADS + (int)threadIdx.x); return; }
	const int bid = (int)blockIdx.x - riders;
	const int rx = (int)blockIdx.y;                // receiver (kernels.h FftInputs)
	const void *__restrict__ fresh = in.fresh[rx];
	if (hist != nullptr) hist += rx * in.hist_stride;
	if (hist_next != nullptr) hist_next += rx * in.hist_stride;
	out += (size_t)rx * (size_t)p.n;
	extern __shared__ float2 sm[];
	const int cs = p.n >> p.l1;            // R2*R3 columns
	const int c0 = bid * FFT_TILE;
	const int total = p.r1 * FFT_TILE;
	for (int e = threadIdx.x; e < total; e += FFT_THREADS) {
		const int r = e >> FFT_TILE_LOG, col = e & (FFT_TILE - 1);
		const int c = c0 + col;
		float2 v = make_float2(0.f, 0.f);
		if (c < cs) {
			const int idx = r * cs + c;
			v = idx < split ? hist[idx] : load_sample<FMT>(fresh, idx - split);
			if (hist_next != nullptr && idx >= p.n - split) hist_next[idx - (p.n - split)] = v;
		}
		sm[e] = v;
	}
	float2 *ltw = sm + total;                  // the radix's twiddle table next to the tile: no global load inside the stages
	for (int t = threadIdx.x; t < p.r1; t += FFT_THREADS) ltw[t] = p.tw1[t];
	__syncthreads();
	lds_fft_columns<-1>(sm, p.r1, p.l1, FFT_TILE, FFT_TILE_LOG, ltw);
	for (int e = threadIdx.x; e < total; e += FFT_THREADS) {
		const int k1 = e >> FFT_TILE_LOG, col = e & (FFT_TILE - 1);
		const int c = c0 + col;
		if (c >= cs) continue;
		float2 v = sm[bitrev(k1, p.l1) * FFT_TILE + col];
		const unsigned ex = ((unsigned)k1 * (unsigned)c) & (unsigned)(p.n - 1);
		out[(size_t)k1 * cs + c] = cmul(v, unit_twiddle(ex, p.logn));
	}
}

// pass 2: for each (k1, n3): R2-point FFT over n2 (stride R3), twiddle W_{R2 R3}^{k2 n3}.  In place.
__global__ __launch_bounds__(FFT_THREADS) void fft_pass2(float2 *__restrict__ buf, FftPlan p, NcoJob job, int riders)
{
	// rider workgroups come FIRST in the grid: dispatched at once, they run beside the whole pass (at the end of the grid they would start when the pass is nearly over)
	if ((int)blockIdx.x < riders) { if (blockIdx.y == 0) nco_table_segment(job, (int)blockIdx.x * FFT_THREADS + (int)threadIdx.x); return; }
	const int bid = (int)blockIdx.x - riders;
	buf += (size_t)blockIdx.y * (size_t)p.n;       // receiver
	extern __shared__ float2 sm[];
	const int r23 = p.n >> p.l1, ncol = p.r1 * p.r3;
	const int cc0 = bid * FFT_TILE;
	const int total = p.r2 * FFT_TILE;
	for (int e = threadIdx.x; e < total; e += FFT_THREADS) {
		const int r = e >> FFT_TILE_LOG, col = e & (FFT_TILE - 1);
		const int cc = cc0 + col;
		float2 v = make_float2(0.f, 0.f);
		if (cc < ncol) {
			const int k1 = cc >> p.l3, n3 = cc & (p.r3 - 1);
			v = buf[(size_t)k1 * r23 + (size_t)r * p.r3 + n3];
		}
		sm[e] = v;
	}
	float2 *ltw = sm + total;
	for (int t = threadIdx.x; t < p.r2; t += FFT_THREADS) ltw[t] = p.tw2[t];
	__syncthreads();
	lds_fft_columns<-1>(sm, p.r2, p.l2, FFT_TILE, FFT_TILE_LOG, ltw);
	for (int e = threadIdx.x; e < total; e += FFT_THREADS) {
		const int k2 = e >> FFT_TILE_LOG, col = e & (FFT_TILE - 1);
		const int cc = cc0 + col;
		if (cc >= ncol) continue;
		const int k1 = cc >> p.l3, n3 = cc & (p.r3 - 1);
		float2 v = sm[bitrev(k2, p.l2) * FFT_TILE + col];
		const unsigned ex = ((unsigned)k2 * (unsigned)n3) & (unsigned)(r23 - 1);
		buf[(size_t)k1 * r23 + (size_t)k2 * p.r3 + n3] = cmul(v, unit_twiddle(ex, p.l2 + p.l3));
	}
}

// pass 3: for each (k1,k2): contiguous R3-point FFT; X[k1 + R1 k2 + R1 R2 k3] stored at (k + n/2) mod n
// when `shifted` (fft_swap_sides as an index remap).  A tile is 16 adjacent k1 so stores stay 128-byte runs.
__global__ __launch_bounds__(FFT_THREADS) void fft_pass3(const float2 *__restrict__ in, float2 *__restrict__ out, FftPlan p, int shifted,
		FftOutLayout lay, NcoJob job, int riders, int64_t out_rx_stride)
{
	// rider workgroups come FIRST in the grid: dispatched at once, they run beside the whole pass (at the end of the grid they would start when the pass is nearly over)
	if ((int)blockIdx.x < riders) { if (blockIdx.y == 0) nco_table_segment(job, (int)blockIdx.x * FFT_THREADS + (int)threadIdx.x); return; }
	const int bid = (int)blockIdx.x - riders;
	in += (size_t)blockIdx.y * (size_t)p.n;        // receiver
	out += blockIdx.y * out_rx_stride;
	extern __shared__ float2 sm[];
	const int r23 = p.n >> p.l1, ncol = p.r1 * p.r2;
	const int cc0 = bid * FFT_TILE;
	const int total = p.r3 * FFT_TILE;
	for (int e = threadIdx.x; e < total; e += FFT_THREADS) {
		const int col = e >> p.l3, n3 = e & (p.r3 - 1);     // fast index walks a contiguous row
		const int cc = cc0 + col;
		float2 v = make_float2(0.f, 0.f);
		if (cc < ncol) {
			const int k2 = cc >> p.l1, k1 = cc & (p.r1 - 1);
			v = in[(size_t)k1 * r23 + (size_t)k2 * p.r3 + n3];
		}
		sm[n3 * FFT_TILE + ((col + n3) & (FFT_TILE - 1))] = v;      // row-skewed tile (fft_core.h): this transposing fill is conflict-free
	}
	float2 *ltw = sm + total;
	for (int t = threadIdx.x; t < p.r3; t += FFT_THREADS) ltw[t] = p.tw3[t];
	__syncthreads();
	lds_fft_columns<-1, true>(sm, p.r3, p.l3, FFT_TILE, FFT_TILE_LOG, ltw);
	const unsigned half = shifted ? (unsigned)(p.n >> 1) : 0u;
	for (int e = threadIdx.x; e < total; e += FFT_THREADS) {
		const int k3 = e >> FFT_TILE_LOG, col = e & (FFT_TILE - 1);
		const int cc = cc0 + col;
		if (cc >= ncol) continue;
		const int k2 = cc >> p.l1, k1 = cc & (p.r1 - 1);
		const unsigned k = (unsigned)k1 + ((unsigned)k2 << p.l1) + ((unsigned)k3 << (p.l1 + p.l2));
		const unsigned i = (k + half) & (unsigned)(p.n - 1);
		const size_t at = lay.row_log ? (size_t)(i >> lay.row_log) * (size_t)lay.row_stride + (i & ((1u << lay.row_log) - 1u)) : (size_t)i;
		const int r = bitrev(k3, p.l3);
		store_out(out, lay, i, at, sm[r * FFT_TILE + ((col + r) & (FFT_TILE - 1))]);
	}
}

// ---- the register-resident passes (fft_regs.h): R = 16 B points x 16 columns per workgroup of 16 B threads ----

// pass 1, fast form: same indexing as fft_pass1
// Every pass: a workgroup takes `tpw` consecutive tiles and asks for the NEXT tile's sixteen points per thread (registers) before it
// transforms the current one: beside a resident demodulator workgroup (118 KiB of a CU's LDS) only one or two of these workgroups fit
// a CU, and without the look-ahead their load -> transform -> store phases ran one after the other (pass 3: 97 us in the pipeline
// against 35 us alone, profiles/r05_experiments.md).
template <int B, int FMT, bool AHEAD>
__global__ __launch_bounds__(16 * B) void fft_rpass1(const float2 *__restrict__ hist, FftInputs in,
		int split, float2 *__restrict__ hist_next, float2 *__restrict__ out, FftPlan p, NcoJob job, int riders, int tpw)
{
	constexpr int NT = 16 * B;
	if ((int)blockIdx.x < riders) { if (blockIdx.y == 0) nco_table_segment(job, (int)blockIdx.x * NT + (int)threadIdx.x); return; }
	const int rx = (int)blockIdx.y;                // receiver (kernels.h FftInputs)
	const void *__restrict__ fresh = in.fresh[rx];
	if (hist != nullptr) hist += rx * in.hist_stride;
	if (hist_next != nullptr) hist_next += rx * in.hist_stride;
	out += (size_t)rx * (size_t)p.n;
	__shared__ float2 ex[B * FR_PITCH];
	__shared__ float2 ltw[16 * B];
	const int bid = ((int)blockIdx.x - riders) * tpw, tid = (int)threadIdx.x;
	const int cs = p.n >> p.l1;            // R2*R3 columns
	const int col = tid & 15, n2 = tid >> 4;
	float2 x[16], xn[16];
	auto load = [&](float2 (&v)[16], int tile) {
		const int c = tile * 16 + col;
#pragma unroll
		for (int n1 = 0; n1 < 16; n1++) {
			const int idx = (n2 + B * n1) * cs + c;
			v[n1] = idx < split ? hist[idx] : load_sample<FMT>(fresh, idx - split);
		}
	};
	load(x, bid);
	ltw[tid] = p.tw1[tid];
	for (int t = 0; t < (AHEAD ? tpw : 1); t++) {
		const int tile = bid + t;
		if (AHEAD && t + 1 < tpw) load(xn, tile + 1);
		if (hist_next != nullptr) {
			const int c = tile * 16 + col;
#pragma unroll
			for (int n1 = 0; n1 < 16; n1++) {
				const int idx = (n2 + B * n1) * cs + c;
				if (idx >= p.n - split) hist_next[idx - (p.n - split)] = x[n1];
			}
		}
		__syncthreads();                               // the twiddle table (first tile); the exchange buffer free again (later ones)
		stage_a(x, ex, ltw, n2, col);
		__syncthreads();
#pragma unroll
		for (int i = 0; i < 256 / NT; i++) {
			const int tt = tid + i * NT, tcol = tt & 15, k1 = tt >> 4, tc = tile * 16 + tcol;
			float2 z[B], w[B];
			stage_b<B>(z, ex, k1, tcol);
			twiddle_run<B>(w, (unsigned)k1 * (unsigned)tc, 16u * (unsigned)tc, p.logn);
#pragma unroll
			for (int k2 = 0; k2 < B; k2++) out[(size_t)(k1 + 16 * k2) * cs + tc] = cmul(z[slot_small<B>(k2)], w[k2]);
		}
		if (AHEAD) {
#pragma unroll
			for (int n1 = 0; n1 < 16; n1++) x[n1] = xn[n1];
		}
	}
}

// pass 2, fast form: in place on buf; for each (k1, n3): R2-point FFT over n2 (stride R3), twiddle W_{R2 R3}^{k2 n3}.
// mix_out (a runtime argument: no second instantiation): the fold's operand instead (fold_domain.h) -- element (k1, k2, n3) goes to
// [g][rho][k2 & 15] of the block's slot.  A workgroup holds one k1, 16 adjacent n3 and every k2: per k2 >> 4 it writes 16 rows x 16 bins
// = 2 KiB contiguous.  The last stage's lanes then run over k2 & 15 first (a wave's store: 512 contiguous bytes) and the exchange planes
// are laid out [col][k1] for it (fft_regs.h stage_a).  keep: the in-place store as well (pass 3 follows for the spectrum monitor).
template <int B, bool AHEAD>
__global__ __launch_bounds__(16 * B) void fft_rpass2(float2 *__restrict__ buf, FftPlan p, NcoJob job, int riders, int tpw,
		float2 *__restrict__ mix_out, int mix_q, int keep, int64_t mix_rx_stride)
{
	constexpr int NT = 16 * B;
	if ((int)blockIdx.x < riders) { if (blockIdx.y == 0) nco_table_segment(job, (int)blockIdx.x * NT + (int)threadIdx.x); return; }
	buf += (size_t)blockIdx.y * (size_t)p.n;       // receiver
	const bool mix = mix_out != nullptr;
	if (mix) mix_out += blockIdx.y * mix_rx_stride;
	__shared__ float2 ex[B * FR_PITCH];
	__shared__ float2 ltw[16 * B];
	const int bid = ((int)blockIdx.x - riders) * tpw, tid = (int)threadIdx.x;
	const int r23 = p.n >> p.l1;
	const int col = tid & 15, n2 = tid >> 4;
	const int kp = mix ? 1 : 16, cp = mix ? FR_TPITCH : 1;
	auto base_of = [&](int tile) {                            // 16 adjacent n3 of one k1 (R3 is a multiple of 16)
		const int cc0 = tile * 16;
		return buf + (size_t)(cc0 >> p.l3) * r23 + (cc0 & (p.r3 - 1));
	};
	float2 x[16], xn[16];
	auto load = [&](float2 (&v)[16], int tile) {
		const float2 *base = base_of(tile);
#pragma unroll
		for (int n1 = 0; n1 < 16; n1++) v[n1] = base[(size_t)(n2 + B * n1) * p.r3 + col];
	};
	load(x, bid);
	ltw[tid] = p.tw2[tid];
	for (int t = 0; t < (AHEAD ? tpw : 1); t++) {
		const int tile = bid + t;
		if (AHEAD && t + 1 < tpw) load(xn, tile + 1);
		float2 *base = base_of(tile);
		const int n30 = (tile * 16) & (p.r3 - 1);
		__syncthreads();
		stage_a(x, ex, ltw, n2, col, kp, cp);
		__syncthreads();
#pragma unroll
		for (int i = 0; i < 256 / NT; i++) {
			const int tt = tid + i * NT, tlo = tt & 15, thi = tt >> 4;
			const int tcol = mix ? thi : tlo, k1 = mix ? tlo : thi, n3 = n30 + tcol;      // k1: here the low four bits of k2
			float2 z[B], w[B];
			stage_b<B>(z, ex, k1, tcol, kp, cp);
			twiddle_run<B>(w, (unsigned)k1 * (unsigned)n3, 16u * (unsigned)n3, p.l2 + p.l3);
			// One store loop for both forms, offsets in 32 bits (below N <= 2^24 elements).  k2 = k1 + 16 kb goes, in place, to row k2 of R3
			// points; mixed, to bin k1 of group g = K1 + R1 (kb mod 2^(q - 4)), row rho = (kb >> (q - 4)) R3 + n3, a group being
			// pre = 2^(l2 - q + l3) rows of 16 bins.  Both are (kb & lo) * s_lo + (kb >> hs) * s_hi from a base
			const int K1 = (tile * 16) >> p.l3, qh = mix_q - 4, rows_log = p.l2 - mix_q + p.l3;
			const unsigned lo = mix ? (1u << qh) - 1u : ~0u, hs = mix ? (unsigned)qh : 31u;
			const unsigned s_lo = mix ? 1u << (p.l1 + rows_log + 4) : 16u << p.l3, s_hi = mix ? 1u << (p.l3 + 4) : 0u;
			float2 *here = base + (size_t)k1 * p.r3 + tcol;
			float2 *dst = mix ? mix_out + ((size_t)K1 << (rows_log + 4)) + (size_t)n3 * 16 + k1 : here;
#pragma unroll
			for (int kb = 0; kb < B; kb++) {
				w[kb] = cmul(z[slot_small<B>(kb)], w[kb]);
				dst[((unsigned)kb & lo) * s_lo + ((unsigned)kb >> hs) * s_hi] = w[kb];
			}
			if (keep) {                                       // (one branch, not one per store)
#pragma unroll
				for (int kb = 0; kb < B; kb++) here[(unsigned)kb * (16u << p.l3)] = w[kb];
			}
		}
		if (AHEAD) {
#pragma unroll
			for (int n1 = 0; n1 < 16; n1++) x[n1] = xn[n1];
		}
	}
}

// pass 3, fast form: contiguous R3-point FFTs of 16 adjacent k1; the tile is filled row-skewed from 1 KiB runs (fft_pass3), the
// sixteen points of a thread come out of LDS, and X[k1 + R1 k2 + R1 R2 k3] goes to (k + n/2) mod n when `shifted`
template <int B>
__global__ __launch_bounds__(16 * B) void fft_rpass3(const float2 *__restrict__ in, float2 *__restrict__ out, FftPlan p, int shifted,
		FftOutLayout lay, NcoJob job, int riders, int tpw, int64_t out_rx_stride)
{
	constexpr int NT = 16 * B, R = 16 * B;
	if ((int)blockIdx.x < riders) { if (blockIdx.y == 0) nco_table_segment(job, (int)blockIdx.x * NT + (int)threadIdx.x); return; }
	in += (size_t)blockIdx.y * (size_t)p.n;        // receiver
	out += blockIdx.y * out_rx_stride;
	__shared__ float2 ex[B * FR_PITCH];                      // first the skewed input tile (R x 16 <= B x 272), then the exchange buffer
	__shared__ float2 ltw[16 * B];
	const int bid = ((int)blockIdx.x - riders) * tpw, tid = (int)threadIdx.x;
	const int r23 = p.n >> p.l1;
	const int col = tid & 15, n2 = tid >> 4;
	float2 pre[16], pn[16];                                  // the tile as it comes out of HBM: element tid + i NT of 16 rows x R points
	auto load = [&](float2 (&v)[16], int tile) {
		const int cc0 = tile * 16;                            // 16 adjacent k1 of one k2 (R1 is a multiple of 16)
		const float2 *src = in + (size_t)(cc0 >> p.l1) * R + (size_t)(cc0 & (p.r1 - 1)) * r23;
#pragma unroll
		for (int i = 0; i < 16; i++) {
			const int e = tid + i * NT;                       // fast index walks a contiguous row (16 R elements, NT = R threads)
			v[i] = src[(size_t)(e / R) * r23 + (e % R)];
		}
	};
	load(pre, bid);
	ltw[tid] = p.tw3[tid];
	const unsigned half = shifted ? (unsigned)(p.n >> 1) : 0u;
	for (int t = 0; t < tpw; t++) {
		const int tile = bid + t;
		const int k2g = (tile * 16) >> p.l1, k10 = (tile * 16) & (p.r1 - 1);
		__syncthreads();                               // the exchange buffer of the tile before has been read
#pragma unroll
		for (int i = 0; i < 16; i++) {
			const int e = tid + i * NT, tcol = e / R, n3 = e % R;
			ex[n3 * 16 + ((tcol + n3) & 15)] = pre[i];
		}
		if (t + 1 < tpw) load(pn, tile + 1);
		__syncthreads();
		float2 x[16];
#pragma unroll
		for (int n1 = 0; n1 < 16; n1++) {
			const int r = n2 + B * n1;
			x[n1] = ex[r * 16 + ((col + r) & 15)];
		}
		__syncthreads();
		stage_a(x, ex, ltw, n2, col);
		__syncthreads();
#pragma unroll
		for (int i = 0; i < 256 / NT; i++) {
			const int tt = tid + i * NT, tcol = tt & 15, ka = tt >> 4;
			float2 z[B];
			stage_b<B>(z, ex, ka, tcol);
			const unsigned kbase = (unsigned)(k10 + tcol) + ((unsigned)k2g << p.l1);
#pragma unroll
			for (int kb = 0; kb < B; kb++) {
				const unsigned k = kbase + ((unsigned)(ka + 16 * kb) << (p.l1 + p.l2));
				const unsigned i2 = (k + half) & (unsigned)(p.n - 1);
				const size_t at = lay.row_log ? (size_t)(i2 >> lay.row_log) * (size_t)lay.row_stride + (i2 & ((1u << lay.row_log) - 1u)) : (size_t)i2;
				store_out(out, lay, i2, at, z[slot_small<B>(kb)]);
			}
		}
#pragma unroll
		for (int i = 0; i < 16; i++) pre[i] = pn[i];
	}
}

// One launch call for every register-resident pass (the kernel by address, its arguments by pointer): a templated launch per
// instantiation costs the library a kilobyte of host code each, and its size is pinned (tests/test_host_logic_cpu.py)
static void launch_rpass(const void *kernel, dim3 grid, int logr, hipStream_t st, hipEvent_t start, hipEvent_t stop, void **args)
{
	(void)hipExtLaunchKernel(kernel, grid, dim3(1u << logr), args, 0, st, start, stop, 0);       // (a failure is found by the caller's hipGetLastError, as with the launch macros)
}
template <int B> static const void *rpass1_of(int fmt)
{
	return fmt == SFMT_CS16 ? (const void *)fft_rpass1<B, SFMT_CS16, false> : fmt == SFMT_CU8 ? (const void *)fft_rpass1<B, SFMT_CU8, false> : (const void *)fft_rpass1<B, SFMT_CF32, false>;
}

// Retune (hfdl_gpu_frontend_retune_channel): channel c becomes a freshly created channel as far as the riders' arrays go -- its
// channelizer constants are the new frequency's, its carried NCO state and segment hand-over what create left there (zero).  One lane,
// three plain stores; stream order places it behind every rider and inverse FFT that read the old values.
__global__ void retune_channelizer_kernel(ChanConst *cc, NcoState *chain, float2 *cont, int c, ChanConst k)
{
	if (blockIdx.x != 0 || threadIdx.x != 0) return;
	cc[c] = k;
	chain[c] = NcoState{ 0, 0.f, 0, 0 };
	cont[c] = make_float2(0.f, 0.f);
}

void launch_retune_channelizer(ChanConst *cc, NcoState *chain, float2 *cont, int c, const ChanConst &k, hipStream_t st, hipEvent_t done)
{
	hipExtLaunchKernelGGL(retune_channelizer_kernel, dim3(1), dim3(64), 0, st, nullptr, done, 0, cc, chain, cont, c, k);
}

// the register-resident passes take radices 64 / 128 / 256 (N = 2^18 .. 2^24); smaller transforms keep the LDS radix-4 passes
static bool fast_plan(const FftPlan &p) { return p.l1 >= 6 && p.l1 <= 8 && p.l2 >= 6 && p.l2 <= 8 && p.l3 >= 6 && p.l3 <= 8; }

// ---- the mixed domain's copies (kernels.h): one thread per element, lanes over k2 & 15, then n3 ----
// dir 0: taps[slot](rho of -n3, j') = R3 plain[k1][k2][n3];  1: plain = taps / R3 (exact: a power of two);  2: plain = block[g][rho][k2 & 15]
__global__ __launch_bounds__(256) void mixed_copy_kernel(float2 *__restrict__ plain, float *__restrict__ taps, const float2 *__restrict__ block,
		int dir, int l1, int l2, int l3, int q, int m, size_t rs_f, int slot)
{
	const size_t n = (size_t)1 << (l1 + l2 + l3);
	for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
		const int ka = (int)(e & 15), n3 = (int)(e >> 4) & ((1 << l3) - 1), kb = (int)(e >> (4 + l3)) & ((1 << (l2 - 4)) - 1), k1 = (int)(e >> (l2 + l3));
		const int k2 = ka + 16 * kb, jp = mixed_bin(natural_bin_of(k1, k2, q, l1), l1);
		float2 *pl = plain + ((size_t)k1 << (l2 + l3)) + ((size_t)k2 << l3) + n3;
		if (dir == 2) {
			*pl = block[((size_t)(jp >> 4) << (l2 - q + l3 + 4)) + (size_t)mixed_row(k2, n3, q, l3) * 16 + (jp & 15)];
			continue;
		}
		float *t = taps + tap_index_f(TAPL_OCTET, m, rs_f, slot, mixed_tap_row(k2, n3, q, l3), jp, 0);
		const float r3 = (float)(1 << l3), ir3 = 1.0f / r3;       // powers of two: both products are exact
		if (dir == 0) { const float2 v = *pl; t[0] = v.x * r3; t[4] = v.y * r3; }
		else *pl = make_float2(t[0] * ir3, t[4] * ir3);
	}
}

static void launch_mixed_copy(const FftPlan &p, const Geometry &g, float2 *plain, float *taps, const float2 *block, int dir, int slot, hipStream_t st)
{
	hipLaunchKernelGGL(mixed_copy_kernel, dim3(2048), dim3(256), 0, st, plain, taps, block, dir, p.l1, p.l2, p.l3, g.mix_q, g.m, (size_t)g.tap_row_stride * 2, slot);
}
void launch_mixed_tap_pack(const FftPlan &p, const Geometry &g, const float2 *plain, float2 *taps, int slot, hipStream_t st) { launch_mixed_copy(p, g, (float2 *)plain, (float *)taps, nullptr, 0, slot, st); }
void launch_mixed_tap_unpack(const FftPlan &p, const Geometry &g, const float2 *taps, int slot, float2 *plain, hipStream_t st) { launch_mixed_copy(p, g, plain, (float *)taps, nullptr, 1, slot, st); }
void launch_mixed_block_unpack(const FftPlan &p, const Geometry &g, const float2 *slot, float2 *plain, hipStream_t st) { launch_mixed_copy(p, g, plain, nullptr, slot, 2, 0, st); }

// one three-pass sequence for all in.nrx receivers: grid dimension y = receiver (work holds nrx transforms, n apart)
void launch_fft_forward(const FftPlan &p, const float2 *hist, const FftInputs &in, int fmt, int split, float2 *hist_next,
		float2 *work, float2 *out, bool shifted, hipStream_t st, FftOutLayout lay, hipEvent_t done, NcoJob nco, hipEvent_t input_read, hipEvent_t start, FftVariant var)
{
	const unsigned nrx = (unsigned)in.nrx;
	const int64_t ors = in.out_stride;
	const int c1 = (p.n >> p.l1), c2 = p.r1 * p.r3, c3 = p.r1 * p.r2;
	const int g1 = (c1 + FFT_TILE - 1) / FFT_TILE, g2 = (c2 + FFT_TILE - 1) / FFT_TILE, g3 = (c3 + FFT_TILE - 1) / FFT_TILE;
	nco.nseg = 3;
	if (fast_plan(p)) {
		// the fold's operand comes out of pass 2: the riders' two segments, the done event and the timed stop ride on passes 1 and 2
		const bool mix = var.mix_out != nullptr, run1 = var.passes & 1, run2 = var.passes & 2, run3 = var.passes & 4;
		if (mix) nco.nseg = 2;
		// one rider workgroup per 16 B channels in front of each pass (a third of the NCO phasor table each)
		auto riders_of = [&](int l) { const int nt = 1 << l; return nco.cc ? (nco.nch + nt - 1) / nt : 0; };
		const int rd1 = riders_of(p.l1), rd2 = riders_of(p.l2), rd3 = mix ? 0 : riders_of(p.l3);
		// tiles per workgroup: 4 where that still leaves four workgroups per CU to hand out, else 2, else 1
		auto tpw_of = [](int tiles) { return tiles % 4 == 0 && tiles >= 4096 ? 4 : tiles % 2 == 0 && tiles >= 1024 ? 2 : 1; };
		// (passes 1 and 2 keep one tile per workgroup: their sixteen loads per thread go straight into the transform's registers, a second
		// set costs 90 - 140 VGPRs with the index arithmetic of the overlap assembly, and they lose little beside the demodulators)
		const int t3 = tpw_of(g3);
		FftPlan plan = p;
		FftInputs inputs = in;
		int tpw = 1, shift = shifted ? 1 : 0, keep = mix && run3 ? 1 : 0;
		int64_t out_stride = ors;
		nco.seg = 0;
		if (run1) {
			void *args[] = { &hist, &inputs, &split, &hist_next, &work, &plan, &nco, (void *)&rd1, &tpw };
			launch_rpass(p.l1 == 6 ? rpass1_of<4>(fmt) : p.l1 == 7 ? rpass1_of<8>(fmt) : rpass1_of<16>(fmt), dim3(g1 + rd1, nrx), p.l1, st, start, input_read, args);
		}
		nco.seg = 1;
		if (run2) {
			void *args[] = { &work, &plan, &nco, (void *)&rd2, &tpw, &var.mix_out, &var.mix_q, &keep, &var.mix_rx_stride };
			launch_rpass(p.l2 == 6 ? (const void *)fft_rpass2<4, false> : p.l2 == 7 ? (const void *)fft_rpass2<8, false> : (const void *)fft_rpass2<16, false>,
					dim3(g2 + rd2, nrx), p.l2, st, nullptr, mix || !run3 ? done : nullptr, args);
		}
		nco.seg = 2;
		if (run3) {
			void *args[] = { &work, &out, &plan, &shift, &lay, &nco, (void *)&rd3, (void *)&t3, &out_stride };
			launch_rpass(p.l3 == 6 ? (const void *)fft_rpass3<4> : p.l3 == 7 ? (const void *)fft_rpass3<8> : (const void *)fft_rpass3<16>,
					dim3(g3 / t3 + rd3, nrx), p.l3, st, nullptr, mix ? nullptr : done, args);
		}
		return;
	}
	const int riders = nco.cc ? (nco.nch + FFT_THREADS - 1) / FFT_THREADS : 0;       // workgroups that run a third of the NCO phasor table each pass
	const dim3 blk(FFT_THREADS);
	// tile + the radix's twiddle table
	const size_t l1 = (size_t)p.r1 * (FFT_TILE + 1) * sizeof(float2), l2 = (size_t)p.r2 * (FFT_TILE + 1) * sizeof(float2);
	nco.seg = 0;
	if (fmt == SFMT_CS16) hipExtLaunchKernelGGL(fft_pass1<SFMT_CS16>, dim3(g1 + riders, nrx), blk, l1, st, start, input_read, 0, hist, in, split, hist_next, work, p, nco, riders);
	else if (fmt == SFMT_CU8) hipExtLaunchKernelGGL(fft_pass1<SFMT_CU8>, dim3(g1 + riders, nrx), blk, l1, st, start, input_read, 0, hist, in, split, hist_next, work, p, nco, riders);
	else hipExtLaunchKernelGGL(fft_pass1<SFMT_CF32>, dim3(g1 + riders, nrx), blk, l1, st, start, input_read, 0, hist, in, split, hist_next, work, p, nco, riders);
	nco.seg = 1;
	hipLaunchKernelGGL(fft_pass2, dim3(g2 + riders, nrx), blk, l2, st, work, p, nco, riders);
	nco.seg = 2;
	hipExtLaunchKernelGGL(fft_pass3, dim3(g3 + riders, nrx), blk, (size_t)p.r3 * (FFT_TILE + 1) * sizeof(float2), st, nullptr, done, 0,
			(const float2 *)work, out, p, shifted ? 1 : 0, lay, nco, riders, ors);
}

}  // namespace hfdl
