// frontend_quality.cpp -- the frame quality records of include/hfdl_gpu.h as a caller sees them: hfdl_gpu_frontend_quality_enable /
// _quality_read.  Every argument is checked before any device work; the ring, its launch and what orders it are Demod's (demod.h),
// the kernel and its arithmetic quality_kernels.hip's and quality.h's.
#include "frontend.h"
#include "demod_logic.h"

using namespace hfdl;

extern "C" int hfdl_gpu_frontend_quality_enable(hfdl_gpu_frontend *fe, int32_t ring_frames, uint32_t flags)
{
	if (!fe) return fail(HFDL_GPU_EINVAL, "null argument");
	if (flags & ~HFDL_GPU_QUALITY_SYMBOLS) return fail(HFDL_GPU_EINVAL, "unknown quality flags 0x%x", flags);
	if (ring_frames != 0 && (ring_frames < 2 || ring_frames > HFDL_GPU_QUALITY_RING_MAX))
		return fail(HFDL_GPU_EINVAL, "quality ring of %d frames: 2 .. %d (or 0 = off)", ring_frames, HFDL_GPU_QUALITY_RING_MAX);
	const bool symbols = (flags & HFDL_GPU_QUALITY_SYMBOLS) != 0;
	const size_t per_frame = sizeof(hfdl_gpu_frame_quality) + (symbols ? sizeof(float2) * (size_t)MAX_DATA_SYMBOLS : 0);
	if ((size_t)ring_frames * per_frame > ((size_t)1 << 30)) return fail(HFDL_GPU_ERANGE, "quality rings of %d frames x %zu bytes: more than 1 GiB", ring_frames, per_frame);
	HIP_TRY(hipSetDevice(fe->device));
	return fe->demod.quality_enable(ring_frames, symbols);
}

extern "C" int hfdl_gpu_frontend_quality_read(hfdl_gpu_frontend *fe, hfdl_gpu_frame_quality *out, float *symbols, int32_t max_frames, int32_t *n,
		uint32_t *dropped, int wait)
{
	if (!n || max_frames < 0 || (!out && max_frames > 0)) return fail(HFDL_GPU_EINVAL, "quality read: null n, max_frames %d, or a null record buffer", max_frames);
	if (!fe) return fail(HFDL_GPU_EINVAL, "null argument");
	const FrameQuality *q = fe->demod.quality.get();
	if (!q) return fail(HFDL_GPU_EINVAL, "the frame quality records are off: hfdl_gpu_frontend_quality_enable() first");
	if (symbols && !q->d_syms.p) return fail(HFDL_GPU_EINVAL, "symbols asked for, but the records were enabled without HFDL_GPU_QUALITY_SYMBOLS");
	if (wait) { if (int rc = hfdl_gpu_frontend_sync(fe)) return rc; }
	else HIP_TRY(hipSetDevice(fe->device));
	return fe->demod.quality_read(out, symbols, max_frames, n, dropped, fe->stream_d);
}
