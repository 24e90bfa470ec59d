// blanker_kernels.hip -- the wideband impulse-noise blanker in front of the forward FFT (gfx950).  blanker.h has the rule and the order
// of the sum; this file is that order on the device.
//
// Two launches per block, grid (chunk of 4096 samples, receiver), both HBM-bound:
//   the sums     reads the block in its sample format (cf32: one 16-byte load per thread and step, 1 KiB contiguous per wave) and leaves
//                one partial sum per chunk: steps 1 - 4 of blanker.h;
//   the zeroing  every workgroup adds the receiver's partial sums up in the same fixed order (step 5: a few KiB out of L2 per 32 KiB of
//                samples -- no ticket, no third launch, and P has the same bits in all of them), forms T = k2 P, reads its chunk again and
//                writes it as cf32 with every sample above T zeroed.  The forward FFT's first pass then reads that buffer through its
//                cf32 instantiation, which is the kernel it is without the blanker: the library's size is pinned
//                (tests/test_host_logic_cpu.py), and blanking instantiations of the twelve first passes would be 140 KB of code.
// The zeroed samples are counted with integer adds alone -- lane counts through the wave butterfly, one 64-bit atomicAdd per workgroup
// that has any -- so the count is exact and order-free.  No floating-point atomics.  Rides in spectrum_kernels' code object
// (objects.sh), compiled without FMA contraction like the rest of it.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include "blanker.h"
#include "kernels.h"

namespace hfdl {

// The two components of sample i as the format stores them, as floats (exact: int16 / uint8 values, or the cf32 words themselves).
// A run-time switch, uniform over the launch, in loops that are not unrolled: the library's size is pinned, and with eight workgroups
// of 256 threads on a CU one load per thread in flight already covers the latency of HBM.
__device__ __forceinline__ float2 raw_sample(const void *__restrict__ raw, int fmt, int i)
{
	if (fmt == SFMT_CS16) { const short2 v = ((const short2 *)raw)[i]; return make_float2((float)v.x, (float)v.y); }
	if (fmt == SFMT_CU8) { const uchar2 v = ((const uchar2 *)raw)[i]; return make_float2((float)v.x, (float)v.y); }
	return ((const float2 *)raw)[i];
}

// Samples a and a + 1 of a block of n, converted; past the end: (0, 0), whose power is the +0.0 the sum is padded with.
// The conversion is load_sample's (fft_kernels.hip: the reference's convert_cf32 / convert_cs16 / convert_cu8) as ONE expression for the
// integer formats, (v - off) / full with off = 0 / 63.5 and full = 32767.5 / 127: v - 0 is exact, so cs16 is load_sample's v / 32767.5,
// and cu8 is its expression itself.  cf32 samples are passed on as the words they are.
// wide: cf32 and the block starts on a 16-byte boundary (a is even), so the pair is one load
__device__ __forceinline__ void load_pair(const void *__restrict__ raw, int fmt, bool wide, int a, int n, float2 &u, float2 &v)
{
	const float off = fmt == SFMT_CU8 ? 63.5f : 0.0f, full = fmt == SFMT_CS16 ? 32767.5f : fmt == SFMT_CU8 ? 127.0f : 1.0f;
	float4 q = make_float4(off, off, off, off);
	if (wide && a + 1 < n) {
		q = *reinterpret_cast<const float4 *>((const float2 *)raw + a);
	} else {
		if (a < n) { const float2 r = raw_sample(raw, fmt, a); q.x = r.x; q.y = r.y; }
		if (a + 1 < n) { const float2 r = raw_sample(raw, fmt, a + 1); q.z = r.x; q.w = r.y; }
	}
	u = make_float2((q.x - off) / full, (q.y - off) / full);
	v = make_float2((q.z - off) / full, (q.w - off) / full);
	if (fmt == SFMT_CF32) {                       // the words themselves, whatever they are (a NaN's payload, a denormal)
		u = make_float2(q.x, q.y);
		v = make_float2(q.z, q.w);
	}
}

// steps 3 and 4: the 256 thread values -> the workgroup's sum, in every thread
__device__ __forceinline__ float blank_tree(float s, float *wsum, int lane, int wave)
{
	for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o);
	if (lane == 0) wsum[wave] = s;
	__syncthreads();
	return (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// ONE kernel for both launches (BlankJob::apply, uniform over the launch): they share the load, and a second kernel's code and
// descriptor are bytes the library does not have.
__global__ __launch_bounds__(BLANK_THREADS) void blank_kernel(BlankJob j)
{
	__shared__ float wsum[BLANK_THREADS / 64];
	__shared__ unsigned wcnt[BLANK_THREADS / 64];
	const int t = threadIdx.x, lane = t & 63, wave = t >> 6, rx = blockIdx.y, w = blockIdx.x, G = gridDim.x;
	float *__restrict__ part = j.partial + (size_t)rx * G;
	float P = 0.0f, T = 0.0f;
	if (j.apply) {
		float fin = 0.0f;
		for (int i = t; i < G; i += BLANK_THREADS) fin = fin + part[i];
		P = blank_tree(fin, wsum, lane, wave) / (float)j.n;
		T = j.k2 * P;                                 // NaN or Inf: no sample compares greater
	}
	const void *__restrict__ raw = j.fresh[rx];
	float2 *__restrict__ out = j.out + (size_t)rx * (size_t)j.out_stride;
	const bool wide = j.fmt == SFMT_CF32 && ((uintptr_t)raw & 15) == 0, wide_out = ((uintptr_t)out & 15) == 0;
	float acc = 0.0f;
	unsigned cnt = 0;
#pragma unroll 1
	for (int s = 0; s < BLANK_STEPS; s++) {
		const int a = w * BLANK_CHUNK + 2 * BLANK_THREADS * s + 2 * t;
		float2 u, v;
		load_pair(raw, j.fmt, wide, a, j.n, u, v);
		const float pu = blank_power_of(u.x, u.y), pv = blank_power_of(v.x, v.y);
		if (!j.apply) { acc = acc + (pu + pv); continue; }
		if (a < j.n && pu > T) { u = make_float2(0.f, 0.f); cnt++; }
		if (a + 1 < j.n && pv > T) { v = make_float2(0.f, 0.f); cnt++; }
		if (a + 1 < j.n) {
			if (wide_out) *reinterpret_cast<float4 *>(out + a) = make_float4(u.x, u.y, v.x, v.y);
			else { out[a] = u; out[a + 1] = v; }
		} else if (a < j.n) {
			out[a] = u;
		}
	}
	if (!j.apply) {
		const float sum = blank_tree(acc, wsum, lane, wave);
		if (t == 0) part[w] = sum;
		return;
	}
	for (int o = 1; o < 64; o <<= 1) cnt += __shfl_xor(cnt, o);
	if (lane == 0) wcnt[wave] = cnt;
	__syncthreads();
	if (t != 0) return;
	const unsigned total = (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
	if (total) atomicAdd(&j.rec[rx].blanked, (unsigned long long)total);
	if (w == 0) { j.rec[rx].power = P; j.rec[rx].threshold = T; }
}

void launch_blanker(BlankJob job, hipStream_t st, hipEvent_t done)
{
	const dim3 grid(blank_chunks(job.n), job.nrx), blk(BLANK_THREADS);
	job.apply = 0;
	hipLaunchKernelGGL(blank_kernel, grid, blk, 0, st, job);
	job.apply = 1;
	hipExtLaunchKernelGGL(blank_kernel, grid, blk, 0, st, nullptr, done, 0, job);
}

}  // namespace hfdl
