// lab.cpp -- the laboratory build (libhfdl_gpu_lab.so, -DHFDL_LAB; include/hfdl_gpu_lab.h): the A/B switches of the measurement scripts,
// the probes (the one reader of the kernels' clock-probe rings among them) and the laboratory's one-shot stage, the burst decoder's
// Viterbi input.  The product build keeps one function of this file: read_lab_config() returning the defaults.
#include "frontend.h"

using namespace hfdl;

#ifndef HFDL_LAB
LabConfig hfdl::read_lab_config() { return LabConfig(); }
#else
#include <algorithm>
#include <cstdio>
#include "../../include/hfdl_gpu_lab.h"
#include "demod_launch.h"

LabConfig hfdl::read_lab_config()
{
	LabConfig c;
	c.fold_tile = (int)env_long("HFDL_GPU_FOLD_TILE", 0, 63, -1);
	c.fold_slices = (int)env_long("HFDL_GPU_FOLD_SLICES", 1, 64, 0);
	c.cu_split = (int)env_long("HFDL_GPU_CU_SPLIT", 2, 8, 0);
	c.cu_partition = env_long("HFDL_GPU_CU_PARTITION", 0, 1, 0) != 0;
	c.fft_stream = (int)env_long("HFDL_GPU_FFT_STREAM", 0, 1, -1);
	c.decode_stream = env_long("HFDL_GPU_DECODE_STREAM", 0, 1, 1) != 0;
	c.fold_bound = (int)env_long("HFDL_GPU_FOLD_BOUND", 0, 1, -1);
	c.fold_ramp = env_long("HFDL_GPU_FOLD_RAMP", 0, 1, 1) != 0;
	return c;
}

static int sync_for_probe(hfdl_gpu_frontend *fe, bool args_ok, const char *what)
{
	if (!fe || !args_ok) return fail(HFDL_GPU_EINVAL, "%s", what);
	return hfdl_gpu_frontend_sync(fe);
}

extern "C" int hfdl_gpu_lab_stream_read_probe(hfdl_gpu_frontend *fe, double *gb_per_s)
{
	if (int rc = sync_for_probe(fe, gb_per_s, "null argument")) return rc;
	// read the resident filter taps themselves (whole multiples of 4 MiB, at most 16 GiB): best launch of every variant
	size_t bytes = sizeof(float2) * (size_t)fe->geo.n * (size_t)fe->geo.nch_pad;
	bytes -= bytes % ((size_t)4 << 20);
	if (bytes > ((size_t)16 << 30)) bytes = (size_t)16 << 30;
	if (bytes == 0) return fail(HFDL_GPU_ERANGE, "front end too small for the probe");
	DevBuf sink;
	HIP_TRY(sink.alloc(sizeof(float)));
	Event e0, e1;
	HIP_TRY(e0.create(EV_TIMING));
	HIP_TRY(e1.create(EV_TIMING));
	double best = 0;
	for (int variant = 0; variant < stream_read_variants(); variant++)
		for (int it = 0; it < 3; it++) {
			HIP_TRY(hipEventRecord(e0, fe->stream));
			launch_stream_read(variant, fe->d_taps, bytes, sink.as<float>(), fe->stream);
			HIP_TRY(hipEventRecord(e1, fe->stream));
			HIP_TRY(hipEventSynchronize(e1));
			float ms = 0;
			HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
			if (getenv("HFDL_GPU_PROBE_VERBOSE")) fprintf(stderr, "stream read variant %d: %.1f GB/s\n", variant, (double)bytes / (ms * 1e-3) / 1e9);
			if (it > 0 && ms > 0) best = std::max(best, (double)bytes / (ms * 1e-3) / 1e9);
		}
	*gb_per_s = best;
	return 0;
}

extern "C" int hfdl_gpu_lab_read_constants(hfdl_gpu_frontend *fe, void *tables, size_t tables_bytes, void *constants, size_t constants_bytes)
{
	if (int rc = sync_for_probe(fe, tables && constants, "null argument")) return rc;
	return fe->demod.read_constants(tables, tables_bytes, constants, constants_bytes);
}

// records made since the last read, oldest first, at most `max`; then the ring's counter starts over.  which = 0: the fold's ring, else
// the demodulator's
extern "C" int hfdl_gpu_lab_clock_probe_read(int which, uint64_t *records, int32_t max, int32_t *n)
{
	if (!records || !n || max < 1) return fail(HFDL_GPU_EINVAL, "bad arguments");
	ClockProbeRing r;
	HIP_TRY(which == 0 ? fold_clock_probe_ring(r) : demod_clock_probe_ring(r));
	unsigned cnt = 0;
	HIP_TRY(hipDeviceSynchronize());
	HIP_TRY(hipMemcpy(&cnt, r.count, sizeof(cnt), hipMemcpyDeviceToHost));
	std::vector<unsigned long long> all(4 * (size_t)r.len);
	HIP_TRY(hipMemcpy(all.data(), r.records, sizeof(unsigned long long) * all.size(), hipMemcpyDeviceToHost));
	const unsigned have = cnt < r.len ? cnt : r.len;
	int k = 0;
	for (unsigned i = 0; i < have && k < max; i++, k++) {
		const unsigned slot = (cnt - have + i) & (r.len - 1);
		for (int j = 0; j < 4; j++) records[4 * k + j] = all[4 * slot + j];
	}
	*n = k;
	cnt = 0;
	HIP_TRY(hipMemcpy(r.count, &cnt, sizeof(cnt), hipMemcpyHostToDevice));
	return 0;
}

extern "C" int hfdl_gpu_lab_burst_soft(int device, const float *symbols, const int32_t *modes, const int32_t *bitmask_lsb, int32_t nframes,
		uint8_t *vin, int32_t *vin_lens)
{
	if (!symbols || !modes || !bitmask_lsb || !vin || !vin_lens || nframes <= 0) return fail(HFDL_GPU_EINVAL, "bad arguments");
	for (int i = 0; i < nframes; i++) if (modes[i] < 0 || modes[i] > 7) return fail(HFDL_GPU_EINVAL, "mode out of range");
	int rc = select_device(device);
	if (rc) return rc;
	StageFrames in;                 // the frames as hfdl_gpu_burst_decode lays them out
	if ((rc = in.upload(symbols, modes, bitmask_lsb, nframes))) return rc;
	const size_t vin_bytes = (size_t)nframes * HFDL_GPU_LAB_VIN_MAX, lens_bytes = sizeof(int32_t) * (size_t)nframes;
	DevBuf d_vin, d_lens;
	HIP_TRY(d_vin.zeroed(vin_bytes));
	HIP_TRY(d_lens.zeroed(lens_bytes));
	launch_burst_soft(in.frames.as<const FrameRec>(), nframes, in.data.as<const cf>(), in.scrambler.as<const uint8_t>(), d_vin.as<uint8_t>(), d_lens.as<int32_t>(), nullptr);
	if ((rc = finish_stage())) return rc;
	HIP_TRY(d_vin.fetch(vin, vin_bytes));
	HIP_TRY(d_lens.fetch(vin_lens, lens_bytes));
	return 0;
}

extern "C" int hfdl_gpu_lab_fold_variant_count(void) { return fold_variant_count(); }

extern "C" int hfdl_gpu_lab_fold_variant_describe(int variant, int32_t desc[6])
{
	int d[6];
	if (!desc || fold_variant_describe(variant, d)) return fail(HFDL_GPU_EINVAL, "no fold variant %d", variant);
	for (int i = 0; i < 6; i++) desc[i] = d[i];
	return 0;
}

// `reps` launches of one compiled tiling (variant -1: the plain-VALU FMA-chain reference kernel) over the front end's own taps and the
// spectra / partial sums of the newest half (whatever the last blocks left there), `nb` blocks per launch, timed by the kernels' own
// events; *checksum = a 64-bit sum over the partial sums' bit patterns, equal across kernels when they are bit-identical.
extern "C" int hfdl_gpu_lab_fold_variant_probe(hfdl_gpu_frontend *fe, int variant, int nb, int reps, double *avg_ms, double *best_ms, uint64_t *checksum)
{
	if (int rc = sync_for_probe(fe, avg_ms && reps >= 1 && nb >= 1, "bad arguments")) return rc;
	if (nb > fe->half_blocks) return fail(HFDL_GPU_ERANGE, "%d blocks asked for, a half holds %d", nb, fe->half_blocks);
	const Geometry &g = fe->geo;
	Event e0, e1;
	HIP_TRY(e0.create(EV_TIMING));
	HIP_TRY(e1.create(EV_TIMING));
	HIP_TRY(hipMemsetAsync(fe->d_partial, 0xff, sizeof(float2) * fe->partial_stride() * (size_t)nb, fe->stream));    // nothing left over from another kernel counts
	double sum = 0, best = 1e30;
	for (int i = 0; i < reps + 1; i++) {
		if (launch_fold_variant(variant, g, fe->d_taps, fe->spec_slot(fe->last_set, 0), fe->spec_stride(), fe->d_partial, fe->partial_stride(), nb, fe->stream, e0, e1) < 0)
			return fail(HFDL_GPU_ERANGE, "fold variant %d does not fit this geometry (M = %d, %d rows per slice) or block count %d", variant, g.m, g.rows_per_slice, nb);
		HIP_TRY(hipEventSynchronize(e1));
		float ms = 0;
		HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
		if (i > 0) { sum += ms; best = std::min(best, (double)ms); }       // first launch: code load
	}
	HIP_TRY(hipGetLastError());
	*avg_ms = sum / reps;
	if (best_ms) *best_ms = best;
	if (checksum) {
		const size_t words = 2 * fe->partial_stride() * (size_t)nb;
		std::vector<uint32_t> h(words);
		HIP_TRY(hipMemcpy(h.data(), fe->d_partial, sizeof(uint32_t) * words, hipMemcpyDeviceToHost));
		uint64_t acc = 0;
		for (size_t i = 0; i < words; i++) acc += (uint64_t)h[i] * (uint64_t)(2 * (i % 65521) + 1);
		*checksum = acc;
	}
	return 0;
}
#endif
