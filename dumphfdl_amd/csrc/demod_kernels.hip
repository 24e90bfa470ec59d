// demod_kernels.hip -- K4 (per-channel streaming demodulator) and K5 (batched burst decoder) for gfx950.
//
// K4  demod_kernel        one workgroup of four wavefronts per channel, a software pipeline over chunks of samples;
//                         body in demod_core.h / demod_logic.h (reference src/hfdl.c:676-892)
// K5  burst_decode_kernel one wavefront per finished frame: descramble + soft de-map + 40-row de-interleave
//                         + rate-1/4 combine + K=7 Viterbi + octet bit reversal + PDU metadata
//                         (reference decode_user_data / dispatch_pdu, src/hfdl.c:993-1080;
//                          libfec update_viterbi27_blk / chainback_viterbi27, src/libfec/viterbi27_port.c:105-221).
//     Viterbi mapping: lane = trellis state (64 = one wavefront); the two predecessor metrics arrive by
//     cross-lane shuffle, the 64 decisions of a trellis step are one __ballot word kept in LDS.
//
// Below the kernels: their launchers (demod_launch.h) and nothing else of the host's -- no allocation, no copy, no wait except the
// constants read-back.  The owner of a front end's demodulator state is demod_host.cpp, the one-shot stage entry points are stages.cpp's,
// the laboratory's clock-probe reader is lab.cpp's.
#include <hip/hip_ext.h>
#include <utility>
#include "demod_core.h"
#ifdef HFDL_DM_STRICT
// Hook of the TEST-ONLY strict builds (tests/hostsim/strict_demod_kernels.hip includes this file after defining HFDL_DM_STRICT, the
// fixed-sequence elementary functions and HFDL_DM_SERIAL_LOOP = the header with the one-lane serial loop it wants run instead of the
// four-wave pipeline).  The product build defines none of it and this file names nothing under tests/.
#include HFDL_DM_SERIAL_LOOP
#endif
#include "demod_tables.h"
#include "hip_handles.h"
#include "demod_launch.h"
#ifdef HFDL_LAB
#include "../../include/hfdl_gpu_lab.h"
#endif

namespace hfdl {

static_assert(sizeof(cf) == sizeof(float2), "cf must alias float2");

// global -> LDS copy by NT threads, 8 independent loads per thread issued before the first is used
template <int NT, typename T>
__device__ __forceinline__ void stage_copy(T *__restrict__ dst, const T *__restrict__ src, int n, int tid)
{
	int i = tid;
	for (; i + 7 * NT < n; i += 8 * NT) {
		T v[8];
#pragma unroll
		for (int u = 0; u < 8; u++) v[u] = src[i + u * NT];
#pragma unroll
		for (int u = 0; u < 8; u++) dst[i + u * NT] = v[u];
	}
	for (; i < n; i += NT) dst[i] = src[i];
}

#ifdef HFDL_LAB
// Laboratory build: the shader clock a launch ran at, measured from inside it.  Workgroup 0 notes s_memtime (shader cycles) and
// s_memrealtime (the constant 100 MHz reference) when it starts and when it ends: cycles / reference ticks x 100 MHz = the average clock
// of THIS launch -- what rocm-smi's quarter-second samples cannot resolve (a fold launch lasts 4 - 7 ms, a demodulator launch 1 ms).
// Ring of 4096 records {launch tag, cycles, reference ticks, 0}; hfdl_gpu_lab_clock_probe_read().
__device__ unsigned long long hfdl_clk_probe[4096 * 4];
__device__ unsigned hfdl_clk_probe_n;
#define HFDL_CLK_PROBE_BEGIN(tag) unsigned long long clk_c0 = 0, clk_r0 = 0; unsigned clk_slot = 0; \
	if (blockIdx.x == 0 && threadIdx.x == 0) { clk_slot = atomicAdd(&hfdl_clk_probe_n, 1u) & 4095u; clk_c0 = __builtin_amdgcn_s_memtime(); clk_r0 = __builtin_amdgcn_s_memrealtime(); }
#define HFDL_CLK_PROBE_END(tag) if (blockIdx.x == 0 && threadIdx.x == 0) { hfdl_clk_probe[4 * clk_slot] = (tag); hfdl_clk_probe[4 * clk_slot + 1] = __builtin_amdgcn_s_memtime() - clk_c0; \
	hfdl_clk_probe[4 * clk_slot + 2] = __builtin_amdgcn_s_memrealtime() - clk_r0; hfdl_clk_probe[4 * clk_slot + 3] = clk_r0; }
#else
#define HFDL_CLK_PROBE_BEGIN(tag)
#define HFDL_CLK_PROBE_END(tag)
#endif

// __launch_bounds__(256, 5): at most 96 VGPRs per wave.  The demodulator workgroups (four waves each -- resampler, AGC + matched
// filter, timing recovery, carrier -- one per SIMD of a CU; 37 KiB of LDS whatever the launch's length: the per-sample arrays are rings,
// demod_lds.h) are co-resident with the fold kernel's workgroups (stream A), and the two are budgeted against each other: the fold's tiling leaves a SIMD at least these registers of its 512 (one 372 / 420-register wave per SIMD since round 5; four waves
// of 104 in round 1) -- a fold tiling that does not (two waves of 256) makes the two kernels take turns and costs the pipeline 10 %
// (fold_kernels.hip, profiles/r05/k4_tilings_in_pipeline.txt).  Staying inside the budget also keeps the loops free of scratch spills:
// scratch is memory, and beside a kernel that reads HBM at 4.6 TB/s every spill reload is a multi-microsecond stall.
template <bool TAPS>
__global__ __launch_bounds__(DM_THREADS, 5) void demod_kernel(DevTables T, DemodBuffers B, const cf *__restrict__ chan_out,
		const int *__restrict__ n_in, int outs_stride, int nblk, int nch)
{
	// These workgroups are a handful of wavefronts that run serial recurrences beside thousands of throughput-bound ones (fold, forward
	// FFT): whenever one of them has an instruction ready it goes first (the instruction arbiter otherwise treats all waves of a SIMD alike)
	__builtin_amdgcn_s_setprio(3);
	HFDL_CLK_PROBE_BEGIN(1)
	extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
	const int c = blockIdx.x, tid = threadIdx.x;
	const DemodLds L(B.cap);
	ChanArrays *A = (ChanArrays *)(lds + L.arrays);
	ChanScalars *S = (ChanScalars *)(lds + L.scalars);
	float2 *l_sstab = (float2 *)(lds + L.sstab);
	float *l_mf = (float *)(lds + L.mf), *l_eq = (float *)(lds + L.eq), *l_corr = (float *)(lds + L.corr);
	uint64_t *l_m1 = (uint64_t *)(lds + L.m1);
	float *l_rs_h = (float *)(lds + L.rs_h);
	ChanState *gs = B.states + c;
	// prologue copies with 8 loads of a lane in flight at a time: beside the fold kernel a dependent load costs microseconds
	stage_copy<DM_THREADS>((uint32_t *)A, (const uint32_t *)&gs->a, (int)(sizeof(ChanArrays) / 4), tid);
	stage_copy<DM_THREADS>((uint32_t *)S, (const uint32_t *)&gs->s, (int)(sizeof(ChanScalars) / 4), tid);
	// the launch's blocks ([nblk][nch][outs]; one block unless the host batches) end to end: one stretch of channelizer output
	int *l_blk = (int *)(lds + L.blk);
	if (tid < DM_MAX_BLOCKS) l_blk[tid] = tid < nblk ? n_in[tid * nch + c] : 0;
#ifdef HFDL_DM_STRICT
	// the serial loop reads the launch's channelizer output from LDS (in the space of agc + mf, which are written only after the
	// resampler has consumed it: 16 cap >= 8 n_in because the resampling rate is > 0.5)
	cf *l_in = (cf *)(lds + L.agc);
	int n_block = 0;
	for (int b = 0; b < nblk; b++) {
		const int nb = n_in[b * nch + c];
		stage_copy<DM_THREADS>(l_in + n_block, chan_out + ((size_t)b * nch + c) * outs_stride, nb, tid);
		n_block += nb;
	}
#endif
	// the resampler's filter bank in LDS: all loads of a lane are in flight together, instead of one dependent memory round trip per tap
	stage_copy<DM_THREADS>((float4 *)l_rs_h, (const float4 *)T.c.rs_h, D_RS_NPFB * D_RS_TAPS / 4, tid);
	// symsync taps in the lane order of the timing-recovery wave: entry [bank][lane] = {tap t, tap t + 16} of the lane's row
	for (int e = tid; e < D_SS_NPFB * 64; e += DM_THREADS) {
		const int bank = e >> 6, row = (e >> 4) & 3, t = e & 15;
		const float *src = (row < 2 ? T.c.ss_mf : T.c.ss_dmf) + bank * D_SS_TAPS;
		l_sstab[e] = make_float2(src[t], t + 16 < D_SS_TAPS ? src[t + 16] : 0.f);
	}
	if (tid < D_MF) l_mf[tid] = T.c.mf[tid];
	if (tid < D_EQ) l_eq[tid] = T.c.eq_h0[tid];
	if (tid < 8) { l_m1[tid] = T.c.m1_hi[tid]; l_m1[8 + tid] = T.c.m1_lo[tid]; }
	if (tid < 128) l_corr[tid] = T.c.corr_tab[tid];
	if (tid < (int)(2 * sizeof(PipeMail) / sizeof(int))) ((int *)(lds + L.mbox))[tid] = 0;
	__syncthreads();
	if (tid < DM_MAX_BLOCKS) {           // samples up to and including block tid
		int sum = 0;
		for (int u = 0; u <= tid; u++) sum += l_blk[u];
		l_blk[DM_MAX_BLOCKS + tid] = sum;
	}
	__syncthreads();

	DemodConst K = T.c;
	K.rs_h = l_rs_h; K.ss_mf = nullptr; K.ss_dmf = nullptr; K.mf = l_mf; K.eq_h0 = l_eq; K.m1_hi = l_m1; K.m1_lo = l_m1 + 8; K.corr_tab = l_corr;
	BlockIo io;
	io.rs = (cf *)(lds + L.rs); io.agc = (cf *)(lds + L.agc); io.mf = (cf *)(lds + L.mfo); io.lvl = (float *)(lds + L.lvl); io.cap = B.cap;
	io.data = B.data + (size_t)c * B.data_slots * MAX_DATA_SYMBOLS; io.data_slots = B.data_slots;
	io.frames = B.frames; io.frame_count = B.frame_count; io.frame_cap = B.frame_cap;
	io.channel = c;
	DemodInput in;
	in.chan = chan_out + (size_t)c * outs_stride; in.blk_stride = (size_t)nch * outs_stride;
	in.ends = l_blk + DM_MAX_BLOCKS; in.ring = (cf *)(lds + L.in); in.n_in = l_blk[2 * DM_MAX_BLOCKS - 1];
	if (TAPS) {
		io.tap_resampled = B.tap_rs + (size_t)c * B.cap; io.tap_mf = B.tap_mf + (size_t)c * B.cap;
		io.tap_symbols = B.tap_sym + (size_t)c * B.cap; io.tap_level = B.tap_lvl + (size_t)c * B.cap;
		io.tap_counts = B.tap_counts + 2 * c;
	} else {
		io.tap_resampled = nullptr; io.tap_mf = nullptr; io.tap_symbols = nullptr; io.tap_level = nullptr; io.tap_counts = nullptr;
	}
	DemodShared sh;
	sh.outq = (cf *)(lds + L.outq); sh.outq_cap = 2 * B.cap;
	sh.cum = (uint16_t *)(lds + L.cum);
	sh.sstab = l_sstab;
	sh.S = S;
	sh.mbox = (PipeMail *)(lds + L.mbox);
	sh.sink = (float *)(lds + L.sink);
	sh.stage = (cf *)(lds + L.stage);
#ifdef HFDL_DM_STRICT
	if (tid == 0) {
		DemodConst Ks = K;
		Ks.ss_mf = T.c.ss_mf; Ks.ss_dmf = T.c.ss_dmf;      // the serial loop reads the filter banks where they lie
		demod_block_serial(*S, *A, Ks, io, l_in, n_block);
		(void)in;
	}
#else
	demod_block<TAPS>(*A, K, io, sh, in);
#endif
	__syncthreads();
	{
		uint32_t *dst = (uint32_t *)&gs->a;
		const uint32_t *src = (const uint32_t *)A;
		for (unsigned i = tid; i < sizeof(ChanArrays) / 4; i += DM_THREADS) dst[i] = src[i];
		dst = (uint32_t *)&gs->s;
		src = (const uint32_t *)S;
		for (unsigned i = tid; i < sizeof(ChanScalars) / 4; i += DM_THREADS) dst[i] = src[i];
	}
	HFDL_CLK_PROBE_END(1000ull + (unsigned long long)nblk)           // tag: 1000 + blocks of the launch = a demodulator launch
}

// ---------------------------------------------------------------- K5

__device__ inline int parity_u32(uint32_t x) { return __popc(x) & 1; }

// ---- K=7 r=1/2 Viterbi, one wave per frame, arithmetic of update_viterbi27_blk / chainback_viterbi27
// (src/libfec/viterbi27_port.c:105-135, 147-221).
//
// Both loops are serial chains, so their length in instructions is the decoder's latency (measured with s_memtime: the
// first version spent 136 cycles per step going forward and 290 per step coming back).
//  * State metrics stay IN PLACE with rotating labels: at step t the metric of state s lives in lane rotr6(s, t mod 6).  The
//    predecessors i and i+32 of the states 2i and 2i+1 then sit in the two lanes that differ in bit 5-(t mod 6), and the
//    same two lanes hold 2i and 2i+1 afterwards: ONE exchange with lane ^ (32 >> t mod 6) per step -- a DPP move on the VALU
//    for four of the six residues -- instead of two arbitrary lane gathers.
//  * In a lane the "own" predecessor costs bm and the "other" 510 - bm whatever the parity of the new state, and the libfec
//    tie rule (decision = path via i+32 strictly cheaper) becomes take_other = (own - other + odd) > 0; decision = take ^ odd.
//  * The 64 decisions of a step are the compare's own mask; v_writelane parks it in lane (t mod 60) of a register pair and
//    60 words go to LDS lane-parallel: no exec-masked store in the chain.
//  * The chainback is scalar code: 64 words per trip are fetched lane-parallel and pulled into SGPRs by v_readlane with a
//    loop-constant lane, the state register never leaves the SALU, finished octets are parked with v_writelane and stored
//    64 at a time.
template <int X> __device__ __forceinline__ uint32_t lane_xor(uint32_t v)
{
	if (X == 32) return (uint32_t)__shfl_xor((int)v, 32);
	if (X == 16) return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x401F);                         // bit mode: and 0x1f, xor 0x10
	if (X == 8) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false);      // row_ror:8
	if (X == 4) {
		const int h = __builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, false);                 // row_half_mirror: ^7
		return (uint32_t)__builtin_amdgcn_update_dpp(0, h, 0x1B, 0xf, 0xf, false);                     // quad_perm [3,2,1,0]: ^3
	}
	if (X == 2) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false);       // quad_perm [2,3,0,1]
	return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false);                   // quad_perm [1,0,3,2]
}

// v_writelane_b32 (no clang builtin in this toolchain): lane SLOT of `old` takes the wave-uniform `value`.  On gfx9 a VALU
// instruction reads one SGPR over the constant bus, so the lane select has to be an inline constant.
template <int SLOT> __device__ __forceinline__ uint32_t write_lane(uint32_t old, uint32_t value)
{
	asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(old) : "s"(value), "n"(SLOT));
	return old;
}

struct VitLane {                                  // per-lane constants of the six residues
	uint32_t t0[6], t1[6];                        // branch-table bytes (0 / 255) of the butterfly this lane belongs to
	int odd[6];                                   // 1 if the lane's new state is odd (its own predecessor is i+32)
};

// lanes whose bit 5-R is set: the lanes that hold an odd new state after a residue-R step
template <int R> __device__ __forceinline__ constexpr uint64_t odd_lanes()
{
	return R == 0 ? 0xFFFFFFFF00000000ull : R == 1 ? 0xFFFF0000FFFF0000ull : R == 2 ? 0xFF00FF00FF00FF00ull
		: R == 3 ? 0xF0F0F0F0F0F0F0F0ull : R == 4 ? 0xCCCCCCCCCCCCCCCCull : 0xAAAAAAAAAAAAAAAAull;
}

// one trellis step of residue R; returns the step's 64 decisions (bit = lane)
template <int R> __device__ __forceinline__ uint64_t acs_step(uint32_t &metric, uint32_t sj, const VitLane &c)
{
	const uint32_t s0 = sj & 255u, s1 = sj >> 8;
	const uint32_t bm = (c.t0[R] ^ s0) + (c.t1[R] ^ s1);
	const uint32_t other = lane_xor<(32 >> R)>(metric);
	const uint32_t cown = metric + bm, coth = other + (510u - bm);
	const bool take_other = (int32_t)(cown - coth) + c.odd[R] > 0;
	metric = take_other ? coth : cown;
	return __ballot(take_other) ^ odd_lanes<R>();
}

// step J of a 60-step chunk: decisions parked in lane J of (wlo, whi)
template <int J> __device__ __forceinline__ void chunk_step(uint32_t &metric, uint32_t &wlo, uint32_t &whi, uint32_t pair, const VitLane &c)
{
	const uint64_t word = acs_step<J % 6>(metric, (uint32_t)__builtin_amdgcn_readlane((int)pair, J), c);
	wlo = write_lane<J>(wlo, (uint32_t)word);
	whi = write_lane<J>(whi, (uint32_t)(word >> 32));
}

template <int... J> __device__ __forceinline__ void chunk_steps(uint32_t &metric, uint32_t &wlo, uint32_t &whi, uint32_t pair, const VitLane &c,
		std::integer_sequence<int, J...>)
{
	(chunk_step<J>(metric, wlo, whi, pair, c), ...);
}

// chainback step J of a 48-step trip (wave-uniform values throughout): word of step = lane J of (wlo, whi)
template <int J> __device__ __forceinline__ void chain_step(uint32_t wlo, uint32_t whi, uint32_t &pos, uint32_t &hi, uint32_t &lo)
{
	const uint64_t wj = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)wlo, J) | ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)whi, J) << 32);
	const uint32_t k = (uint32_t)(wj >> pos) & 1u;
	constexpr uint32_t B = 1u << (J % 6);
	pos = k ? (pos | B) : (pos & ~B);
	if (J < 16) hi = (hi << 1) | k; else lo = (lo << 1) | k;
}

template <int... J> __device__ __forceinline__ void chain_steps(uint32_t wlo, uint32_t whi, uint32_t &pos, uint32_t &hi, uint32_t &lo,
		std::integer_sequence<int, J...>)
{
	(chain_step<J>(wlo, whi, pos, hi, lo), ...);
}

__device__ __forceinline__ uint32_t rotl6(uint32_t x, int k) { return k ? ((x << k) | (x >> (6 - k))) & 63u : x; }
__device__ __forceinline__ uint32_t rotr6(uint32_t x, int k) { return k ? ((x >> k) | (x << (6 - k))) & 63u : x; }

__host__ __device__ constexpr size_t viterbi_lds_bytes(int nbits) { return sizeof(uint64_t) * ((size_t)nbits + 8); }

// vin = 2*nbits soft bytes (LDS or global); decw = viterbi_lds_bytes(nbits) of LDS.  out receives ceil(nbits/8) octets:
// MSB-first as libfec leaves them, or bit-reversed (what dumphfdl dispatches).
__device__ __forceinline__ void viterbi27_wave(const uint8_t *vin, int nbits, uint64_t *decw, uint8_t *out, bool reverse_bits)
{
	const int lane = threadIdx.x;
	VitLane c;
#pragma unroll
	for (int r = 0; r < 6; r++) {
		const uint32_t n = rotl6((uint32_t)lane, (r + 1) % 6), i = n >> 1;      // new state held by this lane after a residue-r step
		c.t0[r] = parity_u32((2u * i) & 0x6d) ? 255u : 0u;
		c.t1[r] = parity_u32((2u * i) & 0x4f) ? 255u : 0u;
		c.odd[r] = (lane >> (5 - r)) & 1;
	}
	uint32_t metric = lane == 0 ? 0u : 63u;           // init_viterbi27(vp, 0)
	// 60 trellis steps per trip: every lane fetches the soft pair of one step, the serial loop takes them with v_readlane
	for (int base = 0; base < nbits; base += 60) {
		const int tt = base + lane;
		const uint32_t pair = (lane < 60 && tt < nbits) ? ((uint32_t)vin[2 * tt] | ((uint32_t)vin[2 * tt + 1] << 8)) : 0u;
		const int lim = nbits - base < 60 ? nbits - base : 60;
		uint32_t wlo = 0, whi = 0;
		if (lim == 60) {                                 // every HFDL frame size is a multiple of 60
			chunk_steps(metric, wlo, whi, pair, c, std::make_integer_sequence<int, 60>());
		} else {                                         // ragged end of an arbitrary nbits: same steps, generic slot select
#define HFDL_ACS(R) if (j + R < lim) { const uint64_t wd = acs_step<R>(metric, (uint32_t)__builtin_amdgcn_readlane((int)pair, j + R), c); \
			if (lane == j + R) { wlo = (uint32_t)wd; whi = (uint32_t)(wd >> 32); } }
			for (int j = 0; j < lim; j += 6) { HFDL_ACS(0) HFDL_ACS(1) HFDL_ACS(2) HFDL_ACS(3) HFDL_ACS(4) HFDL_ACS(5) }
#undef HFDL_ACS
		}
		if (lane < lim) decw[base + lane] = ((uint64_t)whi << 32) | wlo;
	}
	__syncthreads();
	// chainback with the "d += 6" offset: bit idx comes from the word of step idx+6 (words past the end read as 0).  The
	// decision of state s at step t sits in bit rotr6(s, (t+1) mod 6); that rotated state register `pos` changes in ONE bit per
	// step (bit (6 - (t+1) mod 6) mod 6 takes the decoded bit), so it is never shifted or rotated.
	const int noct = (nbits + 7) >> 3;
	uint32_t pos = 0;
	int idx = nbits - 1;
	{	// head: single steps until idx = 47 (mod 48); covers a ragged top octet and any nbits
		uint32_t reg = 0;
		for (; idx >= 0 && idx % 48 != 47; idx--) {
			const int tt = idx + 6;
			uint64_t w = 0;
			if (tt < nbits) w = decw[tt];
			const uint32_t wl = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)w), wh = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(w >> 32));
			const uint32_t k = (uint32_t)((((uint64_t)wh << 32) | wl) >> pos) & 1u;
			const int b = (6 - (tt + 1) % 6) % 6;
			pos = (pos & ~(1u << b)) | (k << b);
			reg = (reg >> 1) | (k << 7);
			if ((idx & 7) == 0 && lane == 0) out[idx >> 3] = reverse_bits ? (uint8_t)(__brev(reg) >> 24) : (uint8_t)reg;
		}
	}
	// body: 48 steps per trip (a multiple of 6 and of 8: bit index and octet boundaries are compile-time), scalar code
	for (; idx >= 47; idx -= 48) {
		const int mine = idx - lane + 6;
		const uint64_t w = (lane < 48 && mine < nbits) ? decw[mine] : 0ull;
		uint32_t hi = 0, lo = 0;
		chain_steps((uint32_t)w, (uint32_t)(w >> 32), pos, hi, lo, std::make_integer_sequence<int, 48>());
		// bit n of (hi:lo) = decoded bit idx-47+n: octet L of the trip is byte L, already in dumphfdl's (bit-reversed) order
		if (lane < 6) {
			uint32_t v = (lane < 4 ? lo >> (8 * lane) : hi >> (8 * (lane - 4))) & 255u;
			if (!reverse_bits) v = __brev(v) >> 24;
			const int o = ((idx - 47) >> 3) + lane;
			if (o < noct) out[o] = (uint8_t)v;
		}
	}
}

constexpr int K5_TABLE_BYTES = 15360;      // >= 168*30*3 coded bits, 256-aligned
constexpr int K5_MAX_BITS = 7560;          // Viterbi steps of the longest frame: 168 * 30 * 3 coded bits at rate 1/2

// LDS of a burst decoder's workgroup (one wave, one frame): de-interleaver table, Viterbi input, the decoder's decision words -- the
// laboratory's soft half alone has none -- and the staged scrambler and constellation constants.  Read by the kernels and their launchers.
struct BurstLds {
	size_t table, vin, decw, consts, total;
	__host__ __device__ constexpr explicit BurstLds(bool viterbi)
		: table(0), vin(K5_TABLE_BYTES), decw(2 * (size_t)K5_TABLE_BYTES), consts(decw + (viterbi ? viterbi_lds_bytes(K5_MAX_BITS) : 0)), total(consts + DEC_CONST_BYTES) {}
};

// A frame of the queue as the burst decoder's kernels take it up
struct BurstFrame {
	FrameRec fr;
	ModeParams mp;
	int nsym, ncoded, cols;        // symbols, coded bits and de-interleaver columns of the mode
	const cf *sym;                 // the frame's data symbols
	float mask_flip;
	uint8_t *l_scr;                // LDS: 128 bytes of scrambler, then the constellation table
	float *l_psk;
};

// frame f's parameters, and the scrambler and constellation constants staged at `consts` (DEC_CONST_BYTES of LDS); ends in a barrier
__device__ __forceinline__ BurstFrame burst_frame(const FrameRec *__restrict__ frames, int f, const cf *__restrict__ data_all, int data_slots,
		const uint8_t *__restrict__ scrambler, unsigned char *consts, int lane)
{
	BurstFrame b;
	b.l_scr = consts;
	b.l_psk = (float *)(consts + DEC_PSK_OFFSET);
	b.fr = frames[f];
	b.mp = mode_params(b.fr.mode);
	b.nsym = b.mp.segments * 30; b.ncoded = b.nsym * b.mp.arity; b.cols = b.ncoded / 40;
	b.sym = data_all + ((size_t)b.fr.channel * data_slots + b.fr.slot) * MAX_DATA_SYMBOLS;
	b.mask_flip = b.fr.bitmask_lsb ? -1.0f : 1.0f;
	b.l_scr[lane] = lane < 120 ? scrambler[lane] : 0;
	if (lane + 64 < 120) b.l_scr[lane + 64] = scrambler[lane + 64];
	if (lane < 32) b.l_psk[lane] = ((const float *)(scrambler + DEC_PSK_OFFSET))[lane];
	__syncthreads();
	return b;
}

// The soft half of the burst decoder -- descrambler, soft de-map, de-interleaver push and pop, rate-1/4 combine -- for one frame and
// one wave: fills vin (LDS) with what the Viterbi decoder is fed and returns its length.  l_scr / l_psk: the staged constants;
// table: K5_TABLE_BYTES of LDS; nsym, ncoded, cols: symbols, coded bits and de-interleaver columns of the mode.  The caller synchronises
// before reading vin.
__device__ __forceinline__ int burst_soft_wave(const int mode, const int nsym, const int ncoded, const int cols, const cf *sym, const float mask_flip,
		const uint8_t *l_scr, const float *l_psk, uint8_t *table, uint8_t *vin)
{
	const int lane = threadIdx.x;
	const ModeParams mp = mode_params(mode);
	// descramble + soft de-map + de-interleaver push (src/hfdl.c:1008-1019, 378-392); four symbol loads per lane in flight
	// (this kernel runs beside the fold, where a dependent global load costs microseconds)
	for (int base = 0; base < nsym; base += 256) {
		cf xs[4];
#pragma unroll
		for (int u = 0; u < 4; u++) { const int i = base + u * 64 + lane; xs[u] = i < nsym ? sym[i] : cf{0.f, 0.f}; }
#pragma unroll
		for (int u = 0; u < 4; u++) {
			const int i = base + u * 64 + lane;
			if (i >= nsym) continue;
			const float flip = (l_scr[i % 120] ? -1.0f : 1.0f) * mask_flip;
			cf x = xs[u];
			x.x *= flip; x.y *= flip;
			uint8_t soft[3];
			psk_soft(mp.arity, x, soft, PskTable{l_psk});
			for (int j = 0; j < mp.arity; j++) {
				const int k = i * mp.arity + j;
				const int row = k % 40;
				int col = (k / 40 - mp.col_shift * k) % cols;
				if (col < 0) col += cols;
				table[row * cols + col] = soft[j];
			}
		}
	}
	__syncthreads();
	// de-interleaver pop (+ rate-1/4 chip averaging), src/hfdl.c:394-403, 1022-1038
	const int vin_len = mp.code_rate == 4 ? ncoded / 2 : ncoded;
	for (int j = lane; j < vin_len; j += 64) {
		if (mp.code_rate == 4) {
			const int p0 = 2 * j, p1 = 2 * j + 1;
			const uint8_t a = table[((9 * p0) % 40) * cols + p0 / 40], b = table[((9 * p1) % 40) * cols + p1 / 40];
			vin[j] = (uint8_t)((a & b) + ((a ^ b) >> 1));
		} else {
			vin[j] = table[((9 * j) % 40) * cols + j / 40];
		}
	}
	return vin_len;
}

__global__ __launch_bounds__(64) void burst_decode_kernel(const FrameRec *__restrict__ frames, int *counts, const int *nframes_ptr, int *stale_count, int frame_cap,
		const cf *__restrict__ data_all, int data_slots, const uint8_t *__restrict__ scrambler, const int32_t *__restrict__ freqs,
		hfdl_gpu_pdu *__restrict__ pdus, int pdu_cap)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
	__builtin_amdgcn_s_setprio(2);          // one wavefront per frame beside the fold: first in line when it has something to issue (see demod_kernel)
	const int f = blockIdx.x, lane = threadIdx.x;
	int nframes = *nframes_ptr;
	if (f == 0 && lane == 0 && stale_count) *stale_count = 0;      // the counter of the launch after next: its last users finished before this launch began
	if (nframes > frame_cap) nframes = frame_cap;
	if (f >= nframes) return;
	constexpr BurstLds L(true);
	uint8_t *table = lds + L.table, *vin = lds + L.vin;
	uint64_t *decw = (uint64_t *)(lds + L.decw);
	const BurstFrame b = burst_frame(frames, f, data_all, data_slots, scrambler, lds + L.consts, lane);
	const FrameRec &fr = b.fr;
	const ModeParams &mp = b.mp;
	const int vin_len = burst_soft_wave(fr.mode, b.nsym, b.ncoded, b.cols, b.sym, b.mask_flip, b.l_scr, b.l_psk, table, vin);
	// claim a slot of the PDU ring: counts[1] = PDUs ever produced, counts[3] = PDUs the host has taken (both mod 2^32);
	// a full ring drops the PDU (counts[2]) without leaving a hole
	int slot = -1;
	if (lane == 0) {
		unsigned *produced = (unsigned *)&counts[1];
		const unsigned taken = *(volatile unsigned *)&counts[3];
		unsigned t = *(volatile unsigned *)produced;
		for (;;) {
			if (t - taken >= (unsigned)pdu_cap) { atomicAdd(&counts[2], 1); break; }
			const unsigned seen = atomicCAS(produced, t, t + 1u);
			if (seen == t) { slot = (int)(t % (unsigned)pdu_cap); break; }
			t = seen;
		}
	}
	slot = __shfl(slot, 0);
	__syncthreads();
	if (slot < 0) return;
	const int nbits = vin_len / 2, noct = (nbits + 7) / 8;
	hfdl_gpu_pdu *out = pdus + slot;
	uint8_t *l_oct = table;                    // the de-interleaver table is dead: decoded octets go to LDS first
	viterbi27_wave(vin, nbits, decw, l_oct, true);
	__syncthreads();
	for (int i = lane; i < noct; i += 64) out->octets[i] = l_oct[i];
	if (lane == 0) {
		// dispatch_pdu metadata, src/hfdl.c:1058-1074
		out->channel = fr.channel;
		out->freq = freqs[fr.channel];
		out->mode = fr.mode;
		out->bit_rate = 1800 * mp.arity / mp.code_rate * DATA_FRAME_LEN / (DATA_FRAME_LEN + T_LEN);
		out->len = noct;
		out->freq_err_hz = fr.freq_err_hz;
		out->rssi_db = 20.0f * log10f(fr.signal_level);
		out->noise_floor_db = 20.0f * log10f(fr.noise_floor);
		out->slot = mp.segments == 72 ? 'S' : 'D';
		out->sample_index = fr.sample_index;
		out->train_bits_bad = fr.train_bad;
		out->train_bits_total = fr.train_total;
		int kind = 0;
		uint32_t hdr_len = 0;
		out->fcs_status = (uint8_t)pdu_triage(l_oct, (uint32_t)noct, &kind, &hdr_len);
		out->pdu_kind = (uint8_t)kind;
		out->hdr_len = (uint16_t)hdr_len;
		LpduCounts lc;
		lc.processed = lc.good = lc.bad_fcs = lc.too_short = lc.truncated = 0;
		if (out->fcs_status == 0 && kind != 0) lc = lpdu_walk(l_oct, (uint32_t)noct, kind, hdr_len);
		out->lpdus_processed = lc.processed; out->lpdus_good = lc.good; out->lpdus_bad_fcs = lc.bad_fcs;
		out->lpdus_too_short = lc.too_short; out->lpdus_truncated = lc.truncated;
		out->lpdu_pad[0] = out->lpdu_pad[1] = out->lpdu_pad[2] = 0;
	}
}

#ifdef HFDL_LAB
// laboratory tap on the Viterbi input (hfdl_gpu_lab_burst_soft): burst_decode_kernel's own staging and soft half, one wave per frame,
// vin copied out to row f of vin_out ([nframes][HFDL_GPU_LAB_VIN_MAX])
__global__ __launch_bounds__(64) void burst_soft_kernel(const FrameRec *__restrict__ frames, const cf *__restrict__ data_all, const uint8_t *__restrict__ scrambler,
		uint8_t *__restrict__ vin_out, int32_t *__restrict__ vin_lens)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
	const int f = blockIdx.x, lane = threadIdx.x;
	constexpr BurstLds L(false);
	uint8_t *table = lds + L.table, *vin = lds + L.vin;
	const BurstFrame b = burst_frame(frames, f, data_all, 2, scrambler, lds + L.consts, lane);
	const int vin_len = burst_soft_wave(b.fr.mode, b.nsym, b.ncoded, b.cols, b.sym, b.mask_flip, b.l_scr, b.l_psk, table, vin);
	__syncthreads();
	uint8_t *dst = vin_out + (size_t)f * HFDL_GPU_LAB_VIN_MAX;
	for (int j = lane; j < vin_len && j < HFDL_GPU_LAB_VIN_MAX; j += 64) dst[j] = vin[j];
	if (lane == 0) vin_lens[f] = vin_len;
}
#endif

__global__ __launch_bounds__(64) void viterbi_batch_kernel(const uint8_t *__restrict__ soft, int nbits, uint8_t *__restrict__ out)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
	const int f = blockIdx.x;
	viterbi27_wave(soft + (size_t)f * 2 * nbits, nbits, (uint64_t *)lds, out + (size_t)f * ((nbits + 7) / 8), false);
}

// stage kernels behind hfdl_gpu_crc16_ccitt / hfdl_gpu_pdu_triage: the device functions burst_decode_kernel runs on every PDU
__global__ void crc16_kernel(const uint8_t *__restrict__ data, uint32_t len, uint32_t crc_init, uint32_t *__restrict__ out)
{
	if (threadIdx.x == 0 && blockIdx.x == 0) *out = crc16_ccitt_step(data, len, (uint16_t)crc_init);
}

__global__ void pdu_triage_kernel(const uint8_t *__restrict__ octets, const int32_t *__restrict__ lens, int npdus, int stride,
		uint8_t *__restrict__ fcs_status, uint8_t *__restrict__ kind, uint16_t *__restrict__ hdr_len)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= npdus) return;
	int k = 0;
	uint32_t hl = 0;
	fcs_status[i] = (uint8_t)pdu_triage(octets + (size_t)i * stride, (uint32_t)lens[i], &k, &hl);
	kind[i] = (uint8_t)k;
	hdr_len[i] = (uint16_t)hl;
}

// the carrier wave's slicer (demod_core.h LaneSlicer) on its own: every wave walks its share of the symbols one at a time, the
// way the carrier loop meets them (the symbol is wave-uniform, the constellation sits one point per lane)
__global__ __launch_bounds__(64) void psk_slice_kernel(int arity, const cf *__restrict__ x, int n, const float *__restrict__ pts, uint32_t *__restrict__ sym, float *__restrict__ perr)
{
	const int lane = (int)threadIdx.x;
	const LaneSlicer slice{lane < 16 ? pts[2 * lane] : 0.f, lane < 16 ? pts[2 * lane + 1] : 0.f, lane};
	const int per = (n + (int)gridDim.x - 1) / (int)gridDim.x, i0 = (int)blockIdx.x * per, i1 = i0 + per < n ? i0 + per : n;
	for (int base = i0; base < i1; base += 64) {
		const cf mine = base + lane < i1 ? x[base + lane] : cf{0.f, 0.f};
		uint32_t s_l = 0;
		float e_l = 0.f;
		for (int k = 0; k < 64 && base + k < i1; k++) {
			cf v; v.x = lane_value(mine.x, k); v.y = lane_value(mine.y, k);
			float e;
			const uint32_t sy = slice(arity, v, &e);
			if (lane == k) { s_l = sy; e_l = e; }
		}
		if (base + lane < i1) { sym[base + lane] = s_l; perr[base + lane] = e_l; }
	}
}

__global__ void lpdu_walk_kernel(const uint8_t *__restrict__ octets, const int32_t *__restrict__ lens, int npdus, int stride, uint8_t *__restrict__ counts)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= npdus) return;
	const uint8_t *buf = octets + (size_t)i * stride;
	int k = 0;
	uint32_t hl = 0;
	LpduCounts c;
	c.processed = c.good = c.bad_fcs = c.too_short = c.truncated = 0;
	if (pdu_triage(buf, (uint32_t)lens[i], &k, &hl) == 0 && k != 0) c = lpdu_walk(buf, (uint32_t)lens[i], k, hl);
	uint8_t *o = counts + (size_t)i * 5;
	o[0] = c.processed; o[1] = c.good; o[2] = c.bad_fcs; o[3] = c.too_short; o[4] = c.truncated;
}

// read-back of the named constants and the tables computed from them AS THE DEVICE SEES THEM (laboratory entry point
// hfdl_gpu_lab_read_constants; compared with the reference's text in tests/test_gpu_constants.py)
__global__ void constants_kernel(HfdlConstants *out)
{
	if (threadIdx.x == 0 && blockIdx.x == 0) {
		HfdlConstants k;
		hfdl_constants(k);
		*out = k;
	}
}

// Retune (hfdl_gpu_frontend_retune_channel), the demodulator's side: the state of channel c becomes the image chan_state_init() made at
// create, word by word over the lanes, except two fields that are carried on: sample_cnt (a PDU's sample index stays the stream's
// position) and data_slot (the burst decoder of the last frame before the boundary may still be reading the other slot).
__global__ __launch_bounds__(256) void retune_demod_kernel(ChanState *__restrict__ states, const ChanState *__restrict__ image, int c)
{
	static_assert(sizeof(ChanState) % 4 == 0 && offsetof(ChanState, s.sample_cnt) % 4 == 0 && offsetof(ChanState, s.data_slot) % 4 == 0, "copied as 32-bit words");
	static_assert(sizeof(ChanScalars::sample_cnt) == 8 && sizeof(ChanScalars::data_slot) == 4, "the carried fields are two words and one word");
	constexpr unsigned words = sizeof(ChanState) / 4, cnt0 = offsetof(ChanState, s.sample_cnt) / 4, slot = offsetof(ChanState, s.data_slot) / 4;
	uint32_t *dst = (uint32_t *)(states + c);
	const uint32_t *src = (const uint32_t *)image;
	for (unsigned w = threadIdx.x; w < words; w += blockDim.x)
		if (w != cnt0 && w != cnt0 + 1 && w != slot) dst[w] = src[w];
}

// ... and the burst decoder's: the frequency its PDUs of channel c are labelled with
__global__ void retune_freq_kernel(int32_t *freqs, int c, int32_t freq)
{
	if (blockIdx.x == 0 && threadIdx.x == 0) freqs[c] = freq;
}

// ---------------------------------------------------------------- launchers (demod_launch.h)

size_t demod_workgroup_lds(int cap) { return DemodLds(cap).total; }

size_t burst_decode_lds() { return BurstLds(true).total; }

static int set_big_lds(const void *fn, size_t bytes)
{
	if (bytes > 64 * 1024) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
	return 0;
}

int prepare_burst_decode() { return set_big_lds((const void *)burst_decode_kernel, burst_decode_lds()); }

int prepare_demod_kernels(size_t demod_lds)
{
	int rc;
	if ((rc = set_big_lds((const void *)demod_kernel<true>, demod_lds))) return rc;
	if ((rc = set_big_lds((const void *)demod_kernel<false>, demod_lds))) return rc;
	return prepare_burst_decode();
}

void launch_demod(bool taps, const DevTables &T, const DemodBuffers &B, const cf *chan_out, const int *n_in, int outs_stride, int nblk, int nch,
		size_t lds, hipStream_t st, hipEvent_t start, hipEvent_t stop)
{
	if (taps) hipExtLaunchKernelGGL(demod_kernel<true>, dim3((unsigned)nch), dim3(DM_THREADS), (unsigned)lds, st, start, stop, 0, T, B, chan_out, n_in, outs_stride, nblk, nch);
	else hipExtLaunchKernelGGL(demod_kernel<false>, dim3((unsigned)nch), dim3(DM_THREADS), (unsigned)lds, st, start, stop, 0, T, B, chan_out, n_in, outs_stride, nblk, nch);
}

void launch_burst_decode(const FrameRec *frames, int *counts, const int *nframes, int *stale_count, int frame_cap, const cf *data, int data_slots,
		const uint8_t *scrambler, const int32_t *freqs, hfdl_gpu_pdu *pdus, int pdu_cap, hipStream_t st, hipEvent_t start, hipEvent_t stop)
{
	hipExtLaunchKernelGGL(burst_decode_kernel, dim3((unsigned)frame_cap), dim3(64), (unsigned)burst_decode_lds(), st, start, stop, 0, frames, counts,
			nframes, stale_count, frame_cap, data, data_slots, scrambler, freqs, pdus, pdu_cap);
}

void launch_retune_demod(ChanState *states, const ChanState *image, int c, hipStream_t st, hipEvent_t done)
{
	hipExtLaunchKernelGGL(retune_demod_kernel, dim3(1), dim3(256), 0, st, nullptr, done, 0, states, image, c);
}

void launch_retune_freq(int32_t *freqs, int c, int32_t freq, hipStream_t st)
{
	hipLaunchKernelGGL(retune_freq_kernel, dim3(1), dim3(64), 0, st, freqs, c, freq);
}

// ---- the stage kernels

int prepare_viterbi_batch(int nbits)
{
	const size_t lds = viterbi_lds_bytes(nbits);
	if (lds > 160 * 1024) return fail(HFDL_GPU_ERANGE, "a Viterbi run over %d bits needs %zu bytes of LDS", nbits, lds);
	return set_big_lds((const void *)viterbi_batch_kernel, lds);
}

void launch_viterbi_batch(const uint8_t *soft, int nbits, int nframes, uint8_t *out, hipStream_t st)
{
	hipLaunchKernelGGL(viterbi_batch_kernel, dim3((unsigned)nframes), dim3(64), viterbi_lds_bytes(nbits), st, soft, nbits, out);
}

void launch_crc16(const uint8_t *data, uint32_t len, uint16_t crc_init, uint32_t *out, hipStream_t st)
{
	hipLaunchKernelGGL(crc16_kernel, dim3(1), dim3(64), 0, st, data, len, (uint32_t)crc_init, out);
}

void launch_pdu_triage(const uint8_t *octets, const int32_t *lens, int npdus, int stride, uint8_t *fcs_status, uint8_t *kind, uint16_t *hdr_len, hipStream_t st)
{
	hipLaunchKernelGGL(pdu_triage_kernel, dim3((unsigned)((npdus + 63) / 64)), dim3(64), 0, st, octets, lens, npdus, stride, fcs_status, kind, hdr_len);
}

void launch_lpdu_walk(const uint8_t *octets, const int32_t *lens, int npdus, int stride, uint8_t *counts, hipStream_t st)
{
	hipLaunchKernelGGL(lpdu_walk_kernel, dim3((unsigned)((npdus + 63) / 64)), dim3(64), 0, st, octets, lens, npdus, stride, counts);
}

void launch_psk_slice(int arity, const cf *x, int n, const float *pts, uint32_t *sym, float *perr, hipStream_t st)
{
	const int waves = n < 64 * 256 ? (n + 63) / 64 : 256;
	hipLaunchKernelGGL(psk_slice_kernel, dim3((unsigned)waves), dim3(64), 0, st, arity, x, n, pts, sym, perr);
}

#ifdef HFDL_LAB
void launch_burst_soft(const FrameRec *frames, int nframes, const cf *data, const uint8_t *scrambler, uint8_t *vin, int32_t *vin_lens, hipStream_t st)
{
	hipLaunchKernelGGL(burst_soft_kernel, dim3((unsigned)nframes), dim3(64), BurstLds(false).total, st, frames, data, scrambler, vin, vin_lens);
}

hipError_t demod_clock_probe_ring(ClockProbeRing &r)
{
	r.len = 4096;
	const hipError_t e = hipGetSymbolAddress((void **)&r.records, HIP_SYMBOL(hfdl_clk_probe));
	return e != hipSuccess ? e : hipGetSymbolAddress((void **)&r.count, HIP_SYMBOL(hfdl_clk_probe_n));
}
#endif

int read_device_constants(void *constants)
{
	DevBuf d_k;
	HIP_TRY(d_k.alloc(sizeof(HfdlConstants)));
	HIP_TRY(hipMemset(d_k.p, 0xff, sizeof(HfdlConstants)));
	hipLaunchKernelGGL(constants_kernel, dim3(1), dim3(64), 0, nullptr, d_k.as<HfdlConstants>());
	HIP_TRY(hipDeviceSynchronize());
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpy(constants, d_k.p, sizeof(HfdlConstants), hipMemcpyDeviceToHost));
	return 0;
}

}  // namespace hfdl
