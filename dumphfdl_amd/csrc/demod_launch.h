// demod_launch.h -- internal: the contract between the demodulator's kernels (demod_kernels.hip) and the host-side owner of their state
// (demod_host.cpp): the kernels' argument structs, and the launchers, defined next to the kernels.  The test-only strict builds link
// their own demod_kernels object with the product's demod_host object (build_strict.sh): whatever depends on how the kernels were
// compiled -- the LDS sizes -- is asked for through this header, never computed on the host's side of it.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/hfdl_gpu.h"
#include "demod_logic.h"

namespace hfdl {

struct DevTables {            // device image, pointers resolved on the host
	DemodConst c;
	const uint8_t *scrambler;
};

struct DemodBuffers {
	ChanState *states;
	cf *data;
	FrameRec *frames;
	int *counts;
	int *frame_count;           // this launch's frames-queued counter (four, rotating: see Demod::enqueue_demod)
	int frame_cap;
	cf *tap_rs, *tap_mf, *tap_sym;
	float *tap_lvl;
	int *tap_counts;
	int cap;
};

size_t demod_workgroup_lds(int cap);         // LDS bytes of a demodulator workgroup for launches of `cap` samples (the product: the same for every cap)
size_t burst_decode_lds();
int prepare_demod_kernels(size_t demod_lds); // LDS attribute of K4 (both variants) and K5, for sizes above 64 KiB only
// K4: one workgroup per channel, `lds` = demod_workgroup_lds(B.cap); start / stop (optional) ride on the kernel's dispatch
void launch_demod(bool taps, const DevTables &T, const DemodBuffers &B, const cf *chan_out, const int *n_in, int outs_stride, int nblk, int nch,
		size_t lds, hipStream_t st, hipEvent_t start, hipEvent_t stop);
// K5: one wavefront per entry of the frame queue (`frame_cap` of them)
void launch_burst_decode(const FrameRec *frames, int *counts, const int *nframes, int *stale_count, int frame_cap, const cf *data,
		const uint8_t *scrambler, const int32_t *freqs, hfdl_gpu_pdu *pdus, int pdu_cap, hipStream_t st, hipEvent_t start, hipEvent_t stop);
int read_device_constants(void *constants);  // sizeof(HfdlConstants): hfdl_constants() as the device evaluates it

}  // namespace hfdl
