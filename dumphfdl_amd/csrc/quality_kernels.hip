// quality_kernels.hip -- frame_quality_kernel: the frame quality records of include/hfdl_gpu.h (hfdl_gpu_frontend_quality_enable), one
// wavefront per finished frame, beside burst_decode_kernel on the decoder's stream.  The arithmetic and the order of its sums are
// quality.h's; this file brings the symbols to it, claims the ring slot and stores the record.  Compiled into spectrum_kernels' object,
// beside the other opt-in features' kernels, without FMA contraction (objects.sh): the host build of quality.h rounds the same way.
#include <hip/hip_runtime.h>
#include "quality.h"

namespace hfdl {

// float4 = two symbols; a frame's symbols start on a multiple of 40 320 bytes
static_assert(sizeof(cf) == 8 && (MAX_DATA_SYMBOLS * sizeof(cf)) % 16 == 0 && MAX_DATA_SYMBOLS % 2 == 0, "frames are read as float4");
constexpr int Q_QUADS = MAX_DATA_SYMBOLS / 2;      // float4 of the longest frame

struct LdsSymbols {
	const cf *x;
	__device__ cf operator()(int i) const { return x[i]; }
};
struct SegmentStore {
	float *seg_err_power;
	__device__ void operator()(int seg, float v) const { seg_err_power[seg] = v; }
};

__device__ __forceinline__ float quality_wave_sum(float v)
{
#pragma unroll
	for (int stride = Q_LANES / 2; stride >= 1; stride >>= 1) v = v + __shfl_xor(v, stride);
	return v;
}

__device__ __forceinline__ float quality_wave_max(float v)
{
#pragma unroll
	for (int stride = Q_LANES / 2; stride >= 1; stride >>= 1) { const float o = __shfl_xor(v, stride); v = v > o ? v : o; }
	return v;
}

__global__ __launch_bounds__(64) void frame_quality_kernel(const FrameRec *__restrict__ frames, const int *nframes_ptr, int frame_cap,
		const cf *__restrict__ data_all, int data_slots, const float *__restrict__ psk_pts, const int32_t *__restrict__ freqs,
		int *counts, hfdl_gpu_frame_quality *__restrict__ recs, cf *__restrict__ syms, int ring)
{
	const int f = blockIdx.x, lane = threadIdx.x;
	int nframes = *nframes_ptr;
	if (nframes > frame_cap) nframes = frame_cap;
	if (f >= nframes) return;
	// claim a slot of the record ring as the burst decoder claims its PDU slot: counts[1] = records ever produced, counts[3] = records
	// the host has taken (both mod 2^32); a full ring drops the frame (counts[2]) before anything of it is written: no hole
	int slot = f;
	if (counts) {
		slot = -1;
		if (lane == 0) {
			unsigned *produced = (unsigned *)&counts[1];
			const unsigned taken = *(volatile unsigned *)&counts[3];
			unsigned t = *(volatile unsigned *)produced;
			for (;;) {
				if (t - taken >= (unsigned)ring) { atomicAdd(&counts[2], 1); break; }
				const unsigned seen = atomicCAS(produced, t, t + 1u);
				if (seen == t) { slot = (int)(t % (unsigned)ring); break; }
				t = seen;
			}
		}
		slot = __shfl(slot, 0);
		if (slot < 0) return;
	}
	const FrameRec fr = frames[f];
	const ModeParams mp = mode_params(fr.mode);
	const int nsym = mp.segments * DATA_FRAME_LEN;
	const cf *x = data_all + ((size_t)fr.channel * data_slots + fr.slot) * MAX_DATA_SYMBOLS;
	hfdl_gpu_frame_quality *out = recs + slot;

	// The frame's symbols, once, coalesced: global -> LDS (and -> the symbol ring, zeros behind the frame's own), four 16-byte loads per
	// lane in flight (this kernel runs beside the fold, where a dependent global load costs microseconds).  Every lane then walks its
	// segments in LDS.
	__shared__ float4 l_x[Q_QUADS];
	const float4 *src = (const float4 *)x;
	float4 *dst = syms ? (float4 *)(syms + (size_t)slot * MAX_DATA_SYMBOLS) : nullptr;
	const int have = nsym / 2;
	for (int base = 0; base < Q_QUADS; base += 4 * Q_LANES) {
		float4 v[4];
#pragma unroll
		for (int u = 0; u < 4; u++) { const int i = base + u * Q_LANES + lane; v[u] = i < have ? src[i] : float4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
		for (int u = 0; u < 4; u++) {
			const int i = base + u * Q_LANES + lane;
			if (i < Q_QUADS) { l_x[i] = v[u]; if (dst) dst[i] = v[u]; }
		}
	}
	__syncthreads();
	const QualitySums L = quality_lane(lane, mp.arity, mp.segments, LdsSymbols{(const cf *)l_x}, PskTable{psk_pts}, SegmentStore{out->seg_err_power});
	QualitySums T;
	T.err = quality_wave_sum(L.err); T.pow = quality_wave_sum(L.pow); T.gre = quality_wave_sum(L.gre); T.gim = quality_wave_sum(L.gim);
	T.emax = quality_wave_max(L.emax);
	if (lane == 0) {
		quality_header(fr, freqs ? freqs[fr.channel] : 0, *out);
		quality_means(T, mp.segments, *out);
	}
}

void launch_frame_quality(const FrameRec *frames, const int *nframes, int frame_cap, const cf *data, int data_slots, const float *psk_pts,
		const int32_t *freqs, int *counts, hfdl_gpu_frame_quality *recs, cf *syms, int ring, hipStream_t st)
{
	hipLaunchKernelGGL(frame_quality_kernel, dim3((unsigned)frame_cap), dim3(Q_LANES), 0, st, frames, nframes, frame_cap, data, data_slots, psk_pts,
			freqs, counts, recs, syms, ring);
}

}  // namespace hfdl
