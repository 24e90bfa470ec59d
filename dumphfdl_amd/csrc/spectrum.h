// spectrum.h -- the spectrum monitor's kernel contract (spectrum_kernels.hip, gfx950 only): band powers of the forward FFT's spectra;
// and the channel export's, which packs selected channels' baseband into a ring (the same translation unit: no FMA contraction).
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

// Channel baseband export: workgroup (s, b) of a launch packs the row of channel channels[s] of the launch's block b -- chan[b][c][0 .. outs),
// of which cnt[b][c] samples (at most P) are valid -- into slot (slot0 + b) % R of the ring:
//   samples[slot][s][0 .. P)   EXPORT_CF32: the valid samples, then +0.0; EXPORT_CS16: per component r = rintf(v * scale), stored as
//                              int16 with |r| > 32767 clamped to +-32767 and NaN stored as 0, both counted in clipped[slot][s]
//   counts[slot][s]            the valid samples n
//   power[slot][s]             (sum_{i<n} (re re + im im)) / n in fp32, 0 for n = 0, in an order that is a function of n alone
//                              (spectrum_kernels.hip), so it is bit-identical from run to run and tests/export_f64.py emulates it
constexpr int EXPORT_THREADS = 256;
enum { EXPORT_CF32 = 0, EXPORT_CS16 = 1 };               // HFDL_GPU_EXPORT_* of include/hfdl_gpu.h
struct ExportJob {
	const float2 *chan = nullptr;       // the launch's first block: [nblk][nch][outs]
	const int32_t *cnt = nullptr;       // [nblk][nch]
	const int32_t *channels = nullptr;  // [nsel], each 0 .. nch - 1
	int32_t nch = 0, outs = 0, P = 0, nsel = 0, nblk = 0, format = EXPORT_CF32;
	float scale = 1.f;
	uint32_t slot0 = 0, R = 1;
	void *samples = nullptr;            // [R][nsel][P] float2 / short2
	int32_t *counts = nullptr;          // [R][nsel]
	float *power = nullptr;
	uint32_t *clipped = nullptr;
};

// one launch, grid (selected channel, block); `done` rides on the dispatch (hipExtLaunchKernelGGL): no barrier packet
void launch_export_pack(const ExportJob &job, hipStream_t st, hipEvent_t done);

}  // namespace hfdl
