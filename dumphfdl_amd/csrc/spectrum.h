// spectrum.h -- the spectrum monitor's kernel contract (spectrum_kernels.hip, gfx950 only): band powers of the forward FFT's spectra.
// A header of its own: kernels.h, fft_core.h and fold_kernels.hip are what the committed fold counter records are hashed over.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hfdl {

constexpr int SPECMON_THREADS = 256;
constexpr int SPECMON_TILE = 2 * SPECMON_THREADS;       // bins a workgroup takes per iteration: one 16-byte load (two bins) per thread
enum { SPECMON_HANN = 1, SPECMON_MAXHOLD = 2 };           // HFDL_GPU_SPECTRUM_* of include/hfdl_gpu.h

// One step: the fftshifted spectra of `nrx` receivers (receiver r at spec + r * rx_stride, n bins each) add their `bins` band powers
//   p[b] = sum_{s = b G}^{(b + 1) G - 1} |Xw[s]|^2 * scale,   G = n / bins,   scale = 1 / (n^2 wpow)
// into acc[r * bins + b] = { sum, compensation } (Kahan) and, with SPECMON_MAXHOLD, max them into peak[r * bins + b].  Receivers whose
// bit is set in `fresh` start over: their accumulators are overwritten by this block, not added to (no memset is ever queued).
// The summation order is fixed by (n, bins) alone (spectrum_kernels.hip), so a result is bit-identical from run to run.
// Interval rows (optional, row_acc != nullptr): the thread that owns a band repeats the Kahan step and the max on row_acc / row_peak,
// the open row's slot of the history ring, laid out [nrx][bins] like acc / peak, from the same p.  row_fresh is ONE bit for all
// receivers (a row covers the same blocks of every receiver): set, the slot is overwritten -- that is how a row starts and how a slot
// of the ring is taken over from the row that held it before.
struct SpecmonJob {
	const float2 *spec = nullptr;
	int64_t rx_stride = 0;
	int32_t n = 0, bins = 0, nrx = 1;
	uint32_t flags = 0;
	float scale = 0.f;
	uint64_t fresh = 0;
	float2 *acc = nullptr;
	float *peak = nullptr;
	float2 *row_acc = nullptr;
	float *row_peak = nullptr;
	uint32_t row_fresh = 0;
};

// one launch, grid y = receiver; `done` (optional) rides on the dispatch (hipExtLaunchKernelGGL): no barrier packet
void launch_spectrum_monitor(const SpecmonJob &job, hipStream_t st, hipEvent_t done = nullptr);

}  // namespace hfdl
