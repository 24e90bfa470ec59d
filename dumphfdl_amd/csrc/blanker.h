// blanker.h -- the wideband impulse-noise blanker's rule, as plain inline functions host code can call (tests/hostsim/blanker_sum_check.cpp
// does), and the contract of its two kernels (blanker_kernels.hip, gfx950 only).
//
// The rule is stateless per block and per receiver.  For the n NEW samples x[i] of a block, after the sample-format conversion
// (sample_load.h), in fp32:
//   power(x) = re re + im im                  two products, one addition, never contracted into an FMA (blank_power_of)
//   P        = (sum_i power(x[i])) / (float)n the sum in the ONE order written down below (blank_block_power)
//   T        = k2 * P                         one fp32 product; k2 = (float)10^(threshold_db / 10), computed in double on the host
//   a sample with power(x) > T enters the transform as (0, 0)
// What follows from it:
//   - every sample is judged exactly once, when it is new: the overlap history of the next block is written by the forward FFT's
//     first pass from what it loaded, which is the blanked block;
//   - Markov's inequality: at most a fraction 1 / k2 of a block can exceed k2 times its mean -- 4 % at 14 dB, 25 % at the 6 dB
//     minimum.  A level jump can never blank a whole block, and there is no state that could get stuck;
//   - a block whose P is NaN or Inf is not blanked: the comparison is false for every sample (so is `anything > Inf`).  Such a block
//     goes through as it would with the blanker off;
//   - the spectrum monitor sees the blanked spectra; retune, channel export and frame quality records are untouched.
//
// The order of the sum, a function of n alone (so P has the same 32 bits from run to run and in every workgroup that computes it):
//   1. the block is cut into chunks of BLANK_CHUNK = 4096 samples, the last one padded with +0.0 terms (every term is >= 0 or NaN, so
//      a +0.0 changes nothing); chunk w belongs to one workgroup of 256 threads;
//   2. thread t starts from 0.0f and adds, for j = 0 .. 7 one after the other, the pair sum power(x[a]) + power(x[a + 1]),
//      a = 4096 w + 512 j + 2 t: one 16-byte load of cf32 per thread and step, 1 KiB contiguous per wave;
//   3. the 64 lanes of a wave: xor butterfly, masks 1, 2, .. 32 -- a binary tree over adjacent lanes;
//   4. the four wave sums pairwise, (w0 + w1) + (w2 + w3): the chunk's partial sum;
//   5. the G = ceil(n / 4096) partial sums: thread t of 256 starts from 0.0f and adds partials t, t + 256, .. one after the other, then
//      steps 3 and 4 again;
//   6. one division by (float)n.
// No floating-point atomics anywhere.  blank_sum_depth(n) = fp32 additions on the longest path of that order.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HFDL_BLANK_HD __host__ __device__
#else
#define HFDL_BLANK_HD
#endif

namespace hfdl {

constexpr int BLANK_THREADS = 256;
constexpr int BLANK_STEPS = 8;                                  // pair sums a thread adds up per chunk
constexpr int BLANK_CHUNK = 2 * BLANK_THREADS * BLANK_STEPS;    // samples per workgroup
constexpr int BLANK_N_MAX = 1 << 24;                            // (float)n is exact up to here
constexpr float BLANK_DB_MIN = 6.f, BLANK_DB_MAX = 60.f;        // include/hfdl_gpu.h

inline float blank_k2(float threshold_db) { return (float)pow(10.0, (double)threshold_db / 10.0); }

// |x|^2 as the sum and the comparison both evaluate it
HFDL_BLANK_HD inline float blank_power_of(float re, float im)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const float a = re * re, b = im * im;
	return a + b;
}

inline int blank_chunks(int n) { return (n + BLANK_CHUNK - 1) / BLANK_CHUNK; }

// steps 2 + 3 + 4 for a chunk: 8 + 1 additions of a thread, 6 + 2 of the tree; step 5: ceil(G / 256) of a thread, 6 + 2 of the tree
inline int blank_sum_depth(int n) { return (BLANK_STEPS + 1) + 8 + (blank_chunks(n) + BLANK_THREADS - 1) / BLANK_THREADS + 8; }

// steps 3 and 4 on the host: v[0 .. 255] -> the workgroup's sum (v is overwritten)
inline float blank_tree256(float *v)
{
	for (int o = 1; o < 64; o <<= 1)
		for (int t = 0; t < BLANK_THREADS; t++)
			if (!(t & o)) { const float s = v[t] + v[t | o]; v[t] = s; v[t | o] = s; }     // both lanes of a butterfly hold a + b (addition commutes bit for bit)
	return (v[0] + v[64]) + (v[128] + v[192]);
}

// the whole order on the host: x = n converted samples (interleaved re, im), 1 <= n <= BLANK_N_MAX
inline float blank_block_power(const float *x, int n)
{
	const int G = blank_chunks(n);
	float fin[BLANK_THREADS], v[BLANK_THREADS];
	for (int t = 0; t < BLANK_THREADS; t++) fin[t] = 0.0f;
	for (int w = 0; w < G; w++) {
		for (int t = 0; t < BLANK_THREADS; t++) {
			float acc = 0.0f;
			for (int j = 0; j < BLANK_STEPS; j++) {
				const int64_t a = (int64_t)w * BLANK_CHUNK + 2 * BLANK_THREADS * j + 2 * t;
				const float p0 = a < n ? blank_power_of(x[2 * a], x[2 * a + 1]) : 0.0f;
				const float p1 = a + 1 < n ? blank_power_of(x[2 * a + 2], x[2 * a + 3]) : 0.0f;
				acc = acc + (p0 + p1);
			}
			v[t] = acc;
		}
		fin[w % BLANK_THREADS] = fin[w % BLANK_THREADS] + blank_tree256(v);
	}
	return blank_tree256(fin) / (float)n;
}

#if defined(__HIPCC__)
// What the kernels leave per receiver.  `blanked` only ever grows: integer adds, so the count is exact whatever the order.
struct BlankRecord {
	float power, threshold;             // P and T of the receiver's newest block
	unsigned long long blanked;         // samples zeroed since the record was cleared
};

// One block of every receiver: receiver r reads n samples of format `fmt` at fresh[r] and leaves them, blanked, as cf32 at
// out + r * out_stride; partial[r * chunks + w] holds the chunk sums in between, rec[r] the record.
struct BlankJob {
	const void *fresh[64] = {};         // (RECEIVERS_MAX of kernels.h)
	float2 *out = nullptr;
	int64_t out_stride = 0;
	float *partial = nullptr;
	BlankRecord *rec = nullptr;
	int32_t n = 0, nrx = 1, fmt = 0;
	int32_t apply = 0;                  // set by launch_blanker: 0 = the chunk sums, 1 = P, T, zeroing and count
	float k2 = 0.f;
};

// two launches on `st`, grid (chunks, receiver): the chunk sums, then P / T / zeroing / count.  `done` (optional) rides on the second
// dispatch (hipExtLaunchKernelGGL): no barrier packet
void launch_blanker(BlankJob job, hipStream_t st, hipEvent_t done = nullptr);
#endif

}  // namespace hfdl
