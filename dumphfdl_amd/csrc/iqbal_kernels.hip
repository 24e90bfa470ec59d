// iqbal_kernels.hip -- the wideband I/Q imbalance and DC corrector in front of the forward FFT (gfx950).  iqbal.h has the rule, the order
// of the sums and the state; this file is that order on the device.
//
// ONE launch per step, grid (chunk of 4096 samples, receiver), HBM-bound: 8 bytes read and 8 written per cf32 sample.  Every workgroup
//   - adds the chunk sums the block before left up in the fixed order (five sums of a few KiB out of L2 per 32 KiB of samples: no ticket, no
//     second launch) and advances the receiver's state from the slot that block wrote: identical bits in every workgroup;
//   - forms (kappa, m) from that state and applies them to its chunk, or copies the chunk where there is no estimate;
//   - leaves its chunk's five sums of the UNCORRECTED samples for the next block's launch.
// Workgroup 0 stores the new state, which is the record as well.  State and chunk sums ping-pong between two slots (IqbalJob::slot), so no
// workgroup reads what another writes, and launches of consecutive blocks are ordered like the forward FFTs they sit in front of.  No
// floating-point atomics.  The sample format is a run-time switch and the loops stay rolled, as in blank_kernel, whose loads this kernel
// shares (blanker_kernels.hip is in front of it in the same object: objects.sh); the library's size is pinned.  Rides in spectrum_kernels'
// code object, compiled without FMA contraction like the rest of it.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include "iqbal.h"
#include "kernels.h"

namespace hfdl {

__global__ __launch_bounds__(BLANK_THREADS) void iqbal_kernel(IqbalJob j)
{
	__shared__ float wprev[5][BLANK_THREADS / 64], wcur[5][BLANK_THREADS / 64];
	const int t = threadIdx.x, lane = t & 63, wave = t >> 6, rx = blockIdx.y, w = blockIdx.x, G = gridDim.x;
	const size_t from = (size_t)(j.slot ^ 1) * (size_t)j.nrx + (size_t)rx, to = (size_t)j.slot * (size_t)j.nrx + (size_t)rx;
	const float alpha = j.alpha[rx];
	const bool restart = (j.restart >> rx) & 1;
	IqbalState s = j.state[from];
	float prev[5] = { 0.f, 0.f, 0.f, 0.f, 0.f };
	if (iqbal_reads_sums(s, alpha, restart)) {                // uniform over the workgroup
		const float *__restrict__ part = j.partial + from * 5 * (size_t)G;
#pragma unroll 1
		for (int q = 0; q < 5; q++) {
			float fin = 0.0f;
			for (int i = t; i < G; i += BLANK_THREADS) fin = fin + part[(size_t)q * G + i];
			for (int o = 1; o < 64; o <<= 1) fin += __shfl_xor(fin, o);
			if (lane == 0) wprev[q][wave] = fin;
		}
		__syncthreads();
		for (int q = 0; q < 5; q++) prev[q] = (wprev[q][0] + wprev[q][1]) + (wprev[q][2] + wprev[q][3]);
	}
	float k_re, k_im, m_re, m_im;
	const int mode = iqbal_advance(s, prev, j.n, alpha, restart, j.seed[rx], k_re, k_im, m_re, m_im);

	const void *__restrict__ raw = j.fresh[rx];
	float2 *out = j.out + (size_t)rx * (size_t)j.out_stride;
	const bool wide = j.fmt == SFMT_CF32 && ((uintptr_t)raw & 15) == 0, wide_out = ((uintptr_t)out & 15) == 0;
	float acc[5] = { 0.f, 0.f, 0.f, 0.f, 0.f };
#pragma unroll 1
	for (int st = 0; st < BLANK_STEPS; st++) {
		const int a = w * BLANK_CHUNK + 2 * BLANK_THREADS * st + 2 * t;
		float2 u, v;
		float tu[5], tv[5];
		load_pair(raw, j.fmt, wide, a, j.n, u, v);
		iqbal_terms(u.x, u.y, tu);
		iqbal_terms(v.x, v.y, tv);
		for (int q = 0; q < 5; q++) acc[q] = acc[q] + (tu[q] + tv[q]);
		if (mode == IQBAL_CORRECTED) {
			iqbal_apply(u.x, u.y, k_re, k_im, m_re, m_im, u.x, u.y);
			iqbal_apply(v.x, v.y, k_re, k_im, m_re, m_im, v.x, v.y);
		}
		if (a + 1 < j.n) {
			if (wide_out) *reinterpret_cast<float4 *>(out + a) = make_float4(u.x, u.y, v.x, v.y);
			else { out[a] = u; out[a + 1] = v; }
		} else if (a < j.n) {
			out[a] = u;
		}
	}
	for (int q = 0; q < 5; q++) {
		float sum = acc[q];
		for (int o = 1; o < 64; o <<= 1) sum += __shfl_xor(sum, o);
		if (lane == 0) wcur[q][wave] = sum;
	}
	__syncthreads();
	if (t != 0) return;
	float *__restrict__ mine = j.partial + to * 5 * (size_t)G;
	for (int q = 0; q < 5; q++) mine[(size_t)q * G + w] = (wcur[q][0] + wcur[q][1]) + (wcur[q][2] + wcur[q][3]);
	if (w == 0) j.state[to] = s;
}

void launch_iqbal(const IqbalJob &job, hipStream_t st, hipEvent_t done)
{
	const dim3 grid(blank_chunks(job.n), job.nrx), blk(BLANK_THREADS);
	hipExtLaunchKernelGGL(iqbal_kernel, grid, blk, 0, st, nullptr, done, 0, job);
}

}  // namespace hfdl
