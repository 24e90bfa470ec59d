// spectrum_kernels.hip -- the spectrum monitor: band powers of the spectra the forward FFT leaves in HBM (gfx950); and, at the end of
// the file, the channel export's packing kernel.
//
// HBM-bound: a step reads nrx * N * 8 bytes once, in 16-byte loads (two bins per thread), and touches nrx * bins * 8 .. 12 bytes of
// accumulators.  Compiled without FMA contraction (build.sh), so the arithmetic below is what tests/spectrum_f64.py emulates in fp32.
//
// Summation order (a function of N and bins alone -- never of the launch history, so results are bit-identical run to run):
//   1. a thread's term is the power of its two adjacent bins, |Xw[s]|^2 + |Xw[s + 1]|^2 with |z|^2 = re re + im im, s even;
//   2. G = N / bins <= 512: a workgroup takes 512 consecutive bins = 512 / G whole bands; the G / 2 terms of a band are added up
//      as a binary tree over adjacent threads (xor butterfly inside the wave, then the waves' sums pairwise through LDS);
//   3. G > 512: a workgroup OWNS a band and walks it in G / 512 steps of 512 bins; a thread adds its terms (512 bins apart) up
//      compensated (Kahan), then the 256 thread sums go through the same tree.  No floating-point atomics anywhere;
//   4. the band's sum times 1 / (N^2 wpow) is the block's band power; the thread that holds it adds it to the accumulator with a
//      Kahan step (two floats per band), so the error of the mean does not grow with the number of blocks;
//   5. with an interval row open (SpecmonJob::row_acc), the same thread repeats step 4 from the same p on the row's slot: a row holds
//      the very words a read-with-reset over the same blocks would, at 8 .. 12 more bytes per band and block and no launch of its own.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include "spectrum.h"

namespace hfdl {

template <bool HANN>
__global__ __launch_bounds__(SPECMON_THREADS) void spectrum_bands(SpecmonJob j)
{
	__shared__ float wsum[SPECMON_THREADS / 64];
	const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const int rx = blockIdx.y;
	const int n = j.n, g = n / j.bins;
	const float2 *__restrict__ x = j.spec + (int64_t)rx * j.rx_stride;
	const bool owner = g > SPECMON_TILE;                          // one band per workgroup, walked in steps; else one tile of whole bands
	const int steps = owner ? g / SPECMON_TILE : 1;
	const int first = owner ? blockIdx.x * g : blockIdx.x * SPECMON_TILE;
	float s = 0.f, c = 0.f;
	for (int it = 0; it < steps; it++) {
		const int s0 = first + it * SPECMON_TILE + 2 * t;         // this thread's bins s0, s0 + 1 (s0 + 1 < n: n is a multiple of the tile)
		const float4 v = *reinterpret_cast<const float4 *>(x + s0);
		float2 a = make_float2(v.x, v.y), b = make_float2(v.z, v.w);
		if (HANN) {
			// Xw[s] = 0.5 X[s] - 0.25 (X[s - 1] + X[s + 1]), indices mod N: the neighbours outside the thread's own pair come from the
			// adjacent lanes; the first and the last lane of a wave fetch theirs from memory (the halo, circular at s = 0 / N - 1)
			float2 l = make_float2(__shfl_up(b.x, 1), __shfl_up(b.y, 1));
			float2 r = make_float2(__shfl_down(a.x, 1), __shfl_down(a.y, 1));
			if (lane == 0) l = x[(s0 + n - 1) & (n - 1)];
			if (lane == 63) r = x[(s0 + 2) & (n - 1)];
			const float2 wa = make_float2(0.5f * a.x - 0.25f * (l.x + b.x), 0.5f * a.y - 0.25f * (l.y + b.y));
			const float2 wb = make_float2(0.5f * b.x - 0.25f * (a.x + r.x), 0.5f * b.y - 0.25f * (a.y + r.y));
			a = wa; b = wb;
		}
		const float term = (a.x * a.x + a.y * a.y) + (b.x * b.x + b.y * b.y);
		const float y = term - c;                                 // Kahan; a single step leaves s = term, c = 0 exactly
		const float u = s + y;
		c = (u - s) - y;
		s = u;
	}
	// binary tree over the threads of a band: lanes_per_band = min(G / 2, 256) adjacent threads
	const int per_band = owner ? SPECMON_THREADS : g / 2;
	const int in_wave = per_band < 64 ? per_band : 64;
	for (int o = 1; o < in_wave; o <<= 1) s += __shfl_xor(s, o);
	if (per_band > 64) {                                          // uniform over the workgroup
		if (lane == 0) wsum[wave] = s;
		__syncthreads();
		if (per_band == 128) s = wsum[wave & ~1] + wsum[wave | 1];
		else s = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
	}
	if (t % per_band != 0) return;                                // the first thread of each band holds its sum and owns its accumulator
	const int band = owner ? (int)blockIdx.x : (int)blockIdx.x * (SPECMON_TILE / g) + t / per_band;
	const size_t idx = (size_t)rx * (size_t)j.bins + (size_t)band;
	const float p = s * j.scale;
	const bool fresh = (j.fresh >> rx) & 1;
	float2 acc = make_float2(p, 0.f);
	if (!fresh) {
		acc = j.acc[idx];
		const float y = p - acc.y;
		const float u = acc.x + y;
		acc.y = (u - acc.x) - y;
		acc.x = u;
	}
	j.acc[idx] = acc;
	if (j.flags & SPECMON_MAXHOLD) j.peak[idx] = fresh ? p : fmaxf(j.peak[idx], p);
	if (j.row_acc == nullptr) return;                             // uniform over the launch: the history is off
	float2 row = make_float2(p, 0.f);
	if (!j.row_fresh) {
		row = j.row_acc[idx];
		const float y = p - row.y;
		const float u = row.x + y;
		row.y = (u - row.x) - y;
		row.x = u;
	}
	j.row_acc[idx] = row;
	if (j.flags & SPECMON_MAXHOLD) j.row_peak[idx] = j.row_fresh ? p : fmaxf(j.row_peak[idx], p);
}

void launch_spectrum_monitor(const SpecmonJob &job, hipStream_t st, hipEvent_t done)
{
	const int g = job.n / job.bins;
	const dim3 grid(g > SPECMON_TILE ? job.bins : job.n / SPECMON_TILE, job.nrx);
	if (job.flags & SPECMON_HANN) hipExtLaunchKernelGGL(spectrum_bands<true>, grid, dim3(SPECMON_THREADS), 0, st, nullptr, done, 0, job);
	else hipExtLaunchKernelGGL(spectrum_bands<false>, grid, dim3(SPECMON_THREADS), 0, st, nullptr, done, 0, job);
}

// ---------------------------------------------------------------- channel baseband export
//
// 256 threads per (selected channel, block).  Copy / convert P samples, and the row's mean power in a fixed order:
//   1. a term is (re re) + (im im);
//   2. thread t adds its terms i = t, t + 256, ... < n one after the other, starting from 0.0f;
//   3. the xor butterfly over the 64 lanes (masks 1, 2, .. 32): a binary tree over adjacent lanes;
//   4. the four wave sums pairwise through LDS, (w0 + w1) + (w2 + w3);
//   5. one division by (float)n.
// No floating-point atomics; plain vector stores only.

// one component as int16: one fp32 multiply, round half to even, clamp to +-32767; NaN is tested for itself and stores 0
static __device__ __forceinline__ short export_cs16(float v, float scale, uint32_t &clip)
{
	if (v != v) { clip++; return 0; }
	const float r = rintf(v * scale);
	if (r > 32767.f) { clip++; return 32767; }
	if (r < -32767.f) { clip++; return -32767; }
	return (short)(int)r;
}

template <bool CS16>
__global__ __launch_bounds__(EXPORT_THREADS) void export_pack_kernel(ExportJob j)
{
	__shared__ float wsum[EXPORT_THREADS / 64];
	__shared__ uint32_t wclip[EXPORT_THREADS / 64];
	const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const int s = blockIdx.x, b = blockIdx.y;
	const int c = j.channels[s];
	const size_t in_row = (size_t)b * (size_t)j.nch + (size_t)c;
	const int P = j.P;
	const int n = min(max(j.cnt[in_row], 0), P);
	const float2 *__restrict__ x = j.chan + in_row * (size_t)j.outs;
	const size_t row = (size_t)((j.slot0 + (uint32_t)b) % j.R) * (size_t)j.nsel + (size_t)s;
	float acc = 0.0f;
	uint32_t clip = 0;
	for (int i = t; i < P; i += EXPORT_THREADS) {
		float2 v = make_float2(0.0f, 0.0f);
		if (i < n) {
			v = x[i];
			acc = acc + ((v.x * v.x) + (v.y * v.y));
		}
		if (CS16) {
			short2 q;
			q.x = export_cs16(v.x, j.scale, clip);
			q.y = export_cs16(v.y, j.scale, clip);
			static_cast<short2 *>(j.samples)[row * (size_t)P + (size_t)i] = q;
		} else {
			static_cast<float2 *>(j.samples)[row * (size_t)P + (size_t)i] = v;
		}
	}
	for (int o = 1; o < 64; o <<= 1) {
		acc += __shfl_xor(acc, o);
		if (CS16) clip += __shfl_xor(clip, o);
	}
	if (lane == 0) { wsum[wave] = acc; wclip[wave] = clip; }
	__syncthreads();
	if (t != 0) return;
	const float p = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
	j.counts[row] = n;
	j.power[row] = n ? p / (float)n : 0.0f;
	j.clipped[row] = CS16 ? (wclip[0] + wclip[1]) + (wclip[2] + wclip[3]) : 0u;
}

void launch_export_pack(const ExportJob &job, hipStream_t st, hipEvent_t done)
{
	const dim3 grid(job.nsel, job.nblk);
	if (job.format == EXPORT_CS16) hipExtLaunchKernelGGL(export_pack_kernel<true>, grid, dim3(EXPORT_THREADS), 0, st, nullptr, done, 0, job);
	else hipExtLaunchKernelGGL(export_pack_kernel<false>, grid, dim3(EXPORT_THREADS), 0, st, nullptr, done, 0, job);
}

}  // namespace hfdl
