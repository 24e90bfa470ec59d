// notch_kernels.hip -- the per-channel adaptive carrier canceller between the channelizer and the demodulator (gfx950).  notch.h has the
// rule and the order of its sums; this file is that order on the device.
//
// Lanes are taps: 32 lanes per channel, two channels per wave, one wave per workgroup, which walks its channels' rows of the run in block
// order.  A sample's dependent chain is the tap products, the five-level tree (two DPP quad permutes, the two DPP mirrors -- after two
// levels the lanes of a quad, after three the lanes of an eight, hold the same value, so the mirrored lane stands for the xor'ed one --
// and one 32-lane swizzle), y, and the tap update.  What depends on the input alone -- the delay line (an LDS ring read at a lane's own
// offset), P and mu / P -- is computed one sample ahead, beside the chain.  Rows are fetched 64 samples (512 B per channel) at a time,
// coalesced, and y leaves the same way.  Rides in spectrum_kernels' code object (objects.sh), compiled without FMA contraction.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include "notch.h"

namespace hfdl {

constexpr int NOTCH_RING = 128;         // a power of two >= 55 + NOTCH_CHUNK
constexpr int NOTCH_CHUNK = 64;
static_assert(NOTCH_HIST + NOTCH_CHUNK <= NOTCH_RING && NOTCH_L == 32, "the ring holds the history and a chunk; a channel is half a wave");

template <int CTRL> __device__ __forceinline__ float notch_dpp(float v)
{
	return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}

// notch.h's tree: every lane of a 32-lane half ends up with the half's sum
__device__ __forceinline__ float notch_tree(float v)
{
	v = v + notch_dpp<0xB1>(v);                 // quad_perm [1, 0, 3, 2]: lane xor 1
	v = v + notch_dpp<0x4E>(v);                 // quad_perm [2, 3, 0, 1]: lane xor 2
	v = v + notch_dpp<0x141>(v);                // row_half_mirror: the other quad of the eight
	v = v + notch_dpp<0x140>(v);                // row_mirror: the other eight of the row
	return v + __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x401F));     // bit mode, xor 16: the other row of the half
}

__global__ __launch_bounds__(64) void notch_kernel(NotchJob j)
{
	__shared__ float2 ring[2][NOTCH_RING];
	__shared__ float2 yout[2][NOTCH_CHUNK];
	const int lane = threadIdx.x, h = lane >> 5, k = lane & 31;
	const int si = 2 * (int)blockIdx.x + h;
	const bool have = si < j.nsel;              // (the last wave's second half may be empty: it runs on zeros and writes nothing)
	const int ch = have ? (j.sel ? j.sel[si] : si) : 0;
	float *__restrict__ st = j.state + (size_t)ch * NOTCH_STATE_FLOATS;
	float wr = 0.0f, wi = 0.0f;
	for (int q = k; q < NOTCH_HIST; q += 32) ring[h][NOTCH_HIST - 1 - q] = have ? reinterpret_cast<const float2 *>(st + 2 * NOTCH_L)[q] : make_float2(0.0f, 0.0f);
	if (have) { wr = st[2 * k]; wi = st[2 * k + 1]; }
	unsigned long long resets = 0;
	float pin = 0.0f, pout = 0.0f, E = 0.0f;
	unsigned pos = NOTCH_HIST;                  // where the next sample goes in the ring
	__syncthreads();
	// the delay line, P and mu / P of the sample to come
	float2 u = ring[h][(pos - NOTCH_D - k) & (NOTCH_RING - 1)];
	float P = notch_tree(notch_power_of(u.x, u.y));
	float g = j.mu / P;
	for (int b = 0; b < j.nblk; b++) {
		const size_t row = ((size_t)b * (size_t)j.nch + (size_t)ch) * (size_t)j.outs;
		int cnt = 0;
		if (have) cnt = j.cnt ? min(max(j.cnt[(size_t)b * (size_t)j.nch + (size_t)ch], 0), j.outs) : j.outs;
		const int nmax = max(cnt, __shfl_xor(cnt, 32));
		pin = 0.0f; pout = 0.0f;
		for (int base = 0; base < nmax; base += NOTCH_CHUNK) {
			const int i0 = base + k, i1 = base + k + 32;
			ring[h][(pos + k) & (NOTCH_RING - 1)] = i0 < cnt ? j.in[row + i0] : make_float2(0.0f, 0.0f);
			ring[h][(pos + k + 32) & (NOTCH_RING - 1)] = i1 < cnt ? j.in[row + i1] : make_float2(0.0f, 0.0f);
			__syncthreads();
			const int m = min(NOTCH_CHUNK, nmax - base);
			for (int i = 0; i < m; i++) {
				const bool act = base + i < cnt;            // uniform over a half
				const float2 x = ring[h][pos & (NOTCH_RING - 1)];
				// one sample ahead: x[n + 1 - D - k] is in the ring already, D >= 1
				const float2 un = ring[h][(pos + 1 - NOTCH_D - k) & (NOTCH_RING - 1)];
				const float Pn = notch_tree(notch_power_of(un.x, un.y));
				const float gn = j.mu / Pn;
				// the chain
				float pr, pi;
				notch_products(wr, wi, u.x, u.y, pr, pi);
				const float sr = notch_tree(pr), sim = notch_tree(pi);
				const float yr = x.x - sr, yi = x.y - sim;
				float nr = wr, ni = wi;
				notch_update(nr, ni, g * yr, g * yi, u.x, u.y);
				const bool ok = notch_ok(P, yr, yi);
				if (act) {
					if (ok) { wr = nr; wi = ni; }
					pin = pin + notch_power_of(x.x, x.y);
					pout = pout + notch_power_of(yr, yi);
					if (k == 0) yout[h][i] = make_float2(yr, yi);
					pos++;
					u = un; P = Pn; g = gn;
				}
			}
			__syncthreads();
			if (i0 < cnt) j.out[row + i0] = yout[h][k];
			if (i1 < cnt) j.out[row + i1] = yout[h][k + 32];
			__syncthreads();
		}
		E = notch_tree(notch_power_of(wr, wi));
		if (have && !(E <= NOTCH_RESET)) { wr = 0.0f; wi = 0.0f; resets++; }
	}
	if (!have) return;
	st[2 * k] = wr; st[2 * k + 1] = wi;
	for (int q = k; q < NOTCH_HIST; q += 32) reinterpret_cast<float2 *>(st + 2 * NOTCH_L)[q] = ring[h][(pos - 1 - q) & (NOTCH_RING - 1)];
	if (k == 0 && j.nblk > 0) {
		NotchRecord *r = j.rec + ch;
		r->blocks += (unsigned long long)j.nblk;
		r->resets += resets;
		r->in_power = pin; r->out_power = pout; r->tap_energy = E;
	}
}

void launch_notch(const NotchJob &job, hipStream_t st, hipEvent_t done)
{
	if (job.nsel < 1 || job.nblk < 1) return;
	hipExtLaunchKernelGGL(notch_kernel, dim3((job.nsel + 1) / 2), dim3(64), 0, st, nullptr, done, 0, job);
}

}  // namespace hfdl
