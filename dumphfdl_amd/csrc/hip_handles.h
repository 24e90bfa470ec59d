// hip_handles.h -- internal: the error text every translation unit of the shim shares, and move-only owners of HIP events, streams and
// page-locked host memory.  Device memory is owned by DevBuf (kernels.h; DevArray here names its element type).  hipFree is called there,
// hipEventDestroy / hipStreamDestroy / hipHostFree here, and none of them anywhere else (hfdl_gpu_host_free() excepted: that memory is
// the caller's) -- tests/test_host_logic_cpu.py reads the sources for it.
#pragma once
#include <hip/hip_runtime.h>
#include <utility>
#include "../../include/hfdl_gpu.h"
#include "kernels.h"

namespace hfdl {

// the text of hfdl_gpu_last_error() of the calling thread; returns `code`
int fail(int code, const char *fmt, ...);
int fail_hip(hipError_t e, bool alloc, const char *expr, const char *file, int line);

// HFDL_GPU_EHIP; CREATE_TRY, while a front end is created, reports hipErrorOutOfMemory as HFDL_GPU_ENOMEM
#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return hfdl::fail_hip(e_, false, #expr, __FILE__, __LINE__); } while (0)
#define CREATE_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return hfdl::fail_hip(e_, true, #expr, __FILE__, __LINE__); } while (0)

enum EventKind { EV_TIMING, EV_NO_TIMING };

struct Event {
	hipEvent_t e = nullptr;
	Event() = default;
	Event(Event &&o) noexcept : e(std::exchange(o.e, nullptr)) {}
	Event &operator=(Event &&o) noexcept { std::swap(e, o.e); return *this; }
	~Event() { if (e) (void)hipEventDestroy(e); }
	hipError_t create(EventKind k) { return k == EV_TIMING ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableTiming); }     // of an empty owner
	operator hipEvent_t() const { return e; }
};

// a non-blocking stream of its own, or another owner's stream under a second name (alias: neither synchronised nor destroyed here)
struct Stream {
	hipStream_t s = nullptr;
	bool owned = false;
	Stream() = default;
	Stream(const Stream &) = delete;
	Stream &operator=(const Stream &) = delete;
	~Stream() { if (owned && s) (void)hipStreamDestroy(s); }
	hipError_t create() { owned = true; return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
	hipError_t create_on_cus(const uint32_t mask[8]) { owned = true; return hipExtStreamCreateWithCUMask(&s, 8, mask); }
	void alias(const Stream &o) { s = o.s; owned = false; }
	void reset() { if (owned && s) (void)hipStreamDestroy(s); s = nullptr; owned = false; }
	hipError_t sync() const { return owned && s ? hipStreamSynchronize(s) : hipSuccess; }
	operator hipStream_t() const { return s; }
};

template <typename T> struct PinnedBuf {
	T *p = nullptr;
	PinnedBuf() = default;
	PinnedBuf(const PinnedBuf &) = delete;
	PinnedBuf &operator=(const PinnedBuf &) = delete;
	~PinnedBuf() { if (p) (void)hipHostFree(p); }
	hipError_t alloc(size_t count) { return hipHostMalloc((void **)&p, sizeof(T) * count, hipHostMallocDefault); }
};

// device memory of `count` T: DevBuf with the element type in its name
template <typename T> struct DevArray : DevBuf {
	hipError_t alloc(size_t count) { return DevBuf::alloc(sizeof(T) * count); }
	operator T *() const { return as<T>(); }
};

// Brackets the launches of a stage entry point with events on the null stream; stop() = their kernel time in ms, copies excluded (0 if
// the events could not be made).  hfdl_gpu_last_stage_ms() reports it (stages.cpp).
struct StageTimer {
	Event e0, e1;
	StageTimer() { if (e0.create(EV_TIMING) == hipSuccess && e1.create(EV_TIMING) == hipSuccess) (void)hipEventRecord(e0, nullptr); }
	double stop()
	{
		float ms = 0;
		if (e0 && e1) { (void)hipEventRecord(e1, nullptr); (void)hipEventSynchronize(e1); if (hipEventElapsedTime(&ms, e0, e1) != hipSuccess) ms = 0; }
		return ms;
	}
};

}  // namespace hfdl
