// real_kernels.hip -- real-sampled input (gfx950): the pass behind the forward FFT that makes a real block's spectrum out of the transform
// of its sample pairs, and the combine that makes a channel's filter out of the transforms of its even and odd taps.  real_input.h has the
// rule and the order of the operations; this file is that order on the device.  Both kernels are pure streaming, 16 bytes per lane and
// access.  Rides in fft_kernels' code object (objects.sh) and switches FMA contraction off inside its own functions, so the arithmetic is
// what the shared header spells and the rest of the object is compiled as it was.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include "real_input.h"
#include "kernels.h"

namespace hfdl {

__device__ __forceinline__ RealCf real_cf(float x, float y) { RealCf v; v.x = x; v.y = y; return v; }

// ONE launch per step, grid (real_groups(n), receiver), HBM-bound: 8 bytes read and 8 written per bin.  A workgroup stages its two runs
// of C + 1 words in LDS -- both ascending in HBM, whole 128-byte segments -- and reads the mirrored members there, descending.
__global__ __launch_bounds__(REAL_THREADS) void real_untangle_kernel(RealUntangleJob j)
{
	__shared__ float2 lo[REAL_CHUNK + 2], hi[REAL_CHUNK + 2];
	const int n = j.n, C = real_chunk(n), w = (int)blockIdx.x, t = (int)threadIdx.x;
	const float2 *__restrict__ in = j.in + blockIdx.y * j.in_stride;
	float2 *__restrict__ out = j.out + blockIdx.y * j.out_stride;
	const int lo0 = real_lo0(n, w), hi0 = real_hi0(n, w);
	for (int e = 2 * t; e < C; e += 2 * REAL_THREADS) {
		const float4 a = *reinterpret_cast<const float4 *>(in + lo0 + e), b = *reinterpret_cast<const float4 *>(in + hi0 + e);
		lo[e] = make_float2(a.x, a.y); lo[e + 1] = make_float2(a.z, a.w);
		hi[e] = make_float2(b.x, b.y); hi[e + 1] = make_float2(b.z, b.w);
	}
	if (t == 0) {
		lo[C] = in[lo0 + C];                       // at most N'/2
		hi[C] = in[real_mirror(n, lo0)];           // hi0 + C, which is Z[0] for the first workgroup
	}
	__syncthreads();
	for (int e = 2 * t; e < C; e += 2 * REAL_THREADS) {
		RealCf x[4];
		for (int s = 0; s < 2; s++) {
			const float2 a = lo[e + s], am = hi[C - e - s], b = hi[e + s], bm = lo[C - e - s];
			x[s] = real_untangle(real_cf(a.x, a.y), real_cf(am.x, am.y), real_twiddle(lo0 + e + s, j.logn));
			x[2 + s] = real_untangle(real_cf(b.x, b.y), real_cf(bm.x, bm.y), real_twiddle(hi0 + e + s, j.logn));
		}
		*reinterpret_cast<float4 *>(out + lo0 + e) = make_float4(x[0].x, x[0].y, x[1].x, x[1].y);
		*reinterpret_cast<float4 *>(out + hi0 + e) = make_float4(x[2].x, x[2].y, x[3].x, x[3].y);
	}
}

void launch_real_untangle(const RealUntangleJob &job, hipStream_t st, hipEvent_t done)
{
	hipExtLaunchKernelGGL(real_untangle_kernel, dim3(real_groups(job.n), job.nrx), dim3(REAL_THREADS), 0, st, nullptr, done, 0, job);
}

// One thread per four bins: 32 bytes of each transform in, 32 bytes of the tap buffer out -- the four bins' Re and Im quads of the octet
// layout lie side by side (kernels.h tap_index_f), four plain cf32 do anyway.  A row holds at least sixteen bins, so a quad never leaves it.
__global__ __launch_bounds__(REAL_THREADS) void real_tap_combine_kernel(RealTapJob j)
{
	const int k = 4 * ((int)blockIdx.x * REAL_THREADS + (int)threadIdx.x);
	if (k >= j.n) return;
	const float4 e0 = *reinterpret_cast<const float4 *>(j.e + k), e1 = *reinterpret_cast<const float4 *>(j.e + k + 2);
	const float4 o0 = *reinterpret_cast<const float4 *>(j.o + k), o1 = *reinterpret_cast<const float4 *>(j.o + k + 2);
	RealCf h[4];
	h[0] = real_tap_combine(real_cf(e0.x, e0.y), real_cf(o0.x, o0.y), real_twiddle(k, j.logn));
	h[1] = real_tap_combine(real_cf(e0.z, e0.w), real_cf(o0.z, o0.w), real_twiddle(k + 1, j.logn));
	h[2] = real_tap_combine(real_cf(e1.x, e1.y), real_cf(o1.x, o1.y), real_twiddle(k + 2, j.logn));
	h[3] = real_tap_combine(real_cf(e1.z, e1.w), real_cf(o1.z, o1.w), real_twiddle(k + 3, j.logn));
	const int m = 1 << j.m_log;
	float *d = j.taps + tap_index_f(j.kind, m, j.rs_f, j.slot, k >> j.m_log, k & (m - 1), 0);
	if (j.kind == TAPL_OCTET) {
		*reinterpret_cast<float4 *>(d) = make_float4(h[0].x, h[1].x, h[2].x, h[3].x);
		*reinterpret_cast<float4 *>(d + 4) = make_float4(h[0].y, h[1].y, h[2].y, h[3].y);
	} else {
		*reinterpret_cast<float4 *>(d) = make_float4(h[0].x, h[0].y, h[1].x, h[1].y);
		*reinterpret_cast<float4 *>(d + 4) = make_float4(h[2].x, h[2].y, h[3].x, h[3].y);
	}
}

void launch_real_tap_combine(const RealTapJob &job, hipStream_t st)
{
	hipLaunchKernelGGL(real_tap_combine_kernel, dim3((job.n / 4 + REAL_THREADS - 1) / REAL_THREADS), dim3(REAL_THREADS), 0, st, job);
}

}  // namespace hfdl
