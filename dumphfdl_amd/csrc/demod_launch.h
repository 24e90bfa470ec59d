// demod_launch.h -- internal: the contract between the demodulator's kernels (demod_kernels.hip) and the host code that runs them: the
// owner of a front end's demodulator state (demod_host.cpp), the one-shot stage entry points (stages.cpp) and the laboratory's (lab.cpp).
// It holds the kernels' argument structs and the launchers, defined next to the kernels: device pointers and a stream in, no allocation,
// no copy, no wait.  The test-only strict builds link their own demod_kernels object with the product's host objects (build_strict.sh):
// whatever depends on how the kernels were compiled -- LDS sizes and their limits, the LDS attribute, grid sizes -- stays behind this
// header, never computed on the host's side of it.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/hfdl_gpu.h"
#include "demod_logic.h"
#include "kernels.h"

namespace hfdl {

struct DevTables {            // device image, pointers resolved on the host
	DemodConst c;
	const uint8_t *scrambler;
};

struct DemodBuffers {
	ChanState *states;
	cf *data;                   // [nch][data_slots][MAX_DATA_SYMBOLS]
	int data_slots;
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
int prepare_burst_decode();                  // ... of K5 alone: a process that runs K5 as a stage may never have created a front end
// K4: one workgroup per channel, `lds` = demod_workgroup_lds(B.cap); start / stop (optional) ride on the kernel's dispatch
void launch_demod(bool taps, const DevTables &T, const DemodBuffers &B, const cf *chan_out, const int *n_in, int outs_stride, int nblk, int nch,
		size_t lds, hipStream_t st, hipEvent_t start, hipEvent_t stop);
// K5: one wavefront per entry of the frame queue (`frame_cap` of them); data: [channel][data_slots][MAX_DATA_SYMBOLS]
void launch_burst_decode(const FrameRec *frames, int *counts, const int *nframes, int *stale_count, int frame_cap, const cf *data, int data_slots,
		const uint8_t *scrambler, const int32_t *freqs, hfdl_gpu_pdu *pdus, int pdu_cap, hipStream_t st, hipEvent_t start, hipEvent_t stop);
// retune: states[c] = *image except sample_cnt and data_slot (the demodulators' stream; `done`, optional, rides on the dispatch);
// freqs[c] = freq (the burst decoders' stream)
void launch_retune_demod(ChanState *states, const ChanState *image, int c, hipStream_t st, hipEvent_t done);
void launch_retune_freq(int32_t *freqs, int c, int32_t freq, hipStream_t st);
int read_device_constants(void *constants);  // sizeof(HfdlConstants): hfdl_constants() as the device evaluates it

// The stage kernels: one wavefront per frame (Viterbi), one lane per PDU (triage, LPDU walk), up to 256 wavefronts sharing the symbols
// (slicer).  prepare_viterbi_batch comes first, before anything is allocated: HFDL_GPU_ERANGE for a run whose decisions do not fit the
// LDS, else the kernel's LDS attribute.
int prepare_viterbi_batch(int nbits);
void launch_viterbi_batch(const uint8_t *soft, int nbits, int nframes, uint8_t *out, hipStream_t st);
void launch_crc16(const uint8_t *data, uint32_t len, uint16_t crc_init, uint32_t *out, hipStream_t st);
void launch_pdu_triage(const uint8_t *octets, const int32_t *lens, int npdus, int stride, uint8_t *fcs_status, uint8_t *kind, uint16_t *hdr_len, hipStream_t st);
void launch_lpdu_walk(const uint8_t *octets, const int32_t *lens, int npdus, int stride, uint8_t *counts, hipStream_t st);      // counts: [npdus][5]
void launch_psk_slice(int arity, const cf *x, int n, const float *pts, uint32_t *sym, float *perr, hipStream_t st);
#ifdef HFDL_LAB
// K5's staging and soft half alone, one wavefront per frame: the Viterbi input of frame f to row f of vin ([nframes][HFDL_GPU_LAB_VIN_MAX])
void launch_burst_soft(const FrameRec *frames, int nframes, const cf *data, const uint8_t *scrambler, uint8_t *vin, int32_t *vin_lens, hipStream_t st);
hipError_t demod_clock_probe_ring(ClockProbeRing &r);      // {tag, shader cycles, 100 MHz ticks, start tick} per probed launch (kernels.h)
#endif

}  // namespace hfdl
