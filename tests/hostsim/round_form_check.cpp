// round_form_check.cpp -- stand-alone proof that the timing-recovery wave's filter-bank index (demod_core.h symsync_chunk)
//     (int)(bf + copysignf(0x1.fffffep-2f, bf))
// is the same 32-bit integer as the reference form (tests/hostsim/serial_demod.h, liquid's symsync_crcf)
//     (int)roundf(bf)
// for every float bit pattern in a range.  0x1.fffffep-2f is the largest float below one half.
//
// The device's conversion is spelled out, since C leaves an out-of-range float-to-int conversion undefined: v_cvt_i32_f32
// truncates towards zero, saturates at INT32_MIN / INT32_MAX (so do +-inf) and turns a NaN into 0.  The addition is one IEEE
// round-to-nearest-even fp32 add with subnormals kept (the demodulator is built without FMA contraction and with fp32 denormals
// on); a NaN operand gives a NaN, whatever its sign.
//
// usage: round_form_check                  every one of the 2^32 patterns
//        round_form_check LO HI            the patterns LO .. HI inclusive (hexadecimal) in BOTH signs
// prints "ok <patterns compared>" and exits 0, or the first differing patterns and exits 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#include <atomic>

static inline float as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static inline int32_t cvt_i32_f32(float x)       // v_cvt_i32_f32
{
	if (x != x) return 0;
	if (x >= 2147483648.0f) return INT32_MAX;
	if (x <= -2147483648.0f) return INT32_MIN;
	return (int32_t)x;                           // in range: C truncates towards zero, as the instruction does
}

static inline int32_t reference_form(float bf) { return cvt_i32_f32(roundf(bf)); }
static inline int32_t shipped_form(float bf)
{
	volatile float sum = bf + copysignf(0x1.fffffep-2f, bf);      // volatile: one fp32 add, never kept in a wider register
	return cvt_i32_f32(sum);
}

static std::atomic<uint64_t> bad{0};

static void scan(uint64_t lo, uint64_t hi)       // patterns lo .. hi inclusive
{
	for (uint64_t u = lo; u <= hi; u++) {
		const float x = as_float((uint32_t)u);
		const int32_t a = reference_form(x), b = shipped_form(x);
		if (a != b && bad.fetch_add(1) < 16) fprintf(stderr, "pattern %08x (%a): roundf form %d, add form %d\n", (unsigned)u, x, a, b);
	}
}

int main(int argc, char **argv)
{
	std::vector<std::pair<uint64_t, uint64_t>> ranges;
	if (argc == 3) {
		const uint64_t lo = strtoull(argv[1], nullptr, 16), hi = strtoull(argv[2], nullptr, 16);
		if (lo > hi || hi > 0x7fffffffull) { fprintf(stderr, "bad range\n"); return 2; }
		ranges.push_back({lo, hi});
		ranges.push_back({lo | 0x80000000ull, hi | 0x80000000ull});
	} else if (argc == 1) {
		ranges.push_back({0, 0xffffffffull});
	} else {
		fprintf(stderr, "usage: %s [LO HI]\n", argv[0]);
		return 2;
	}
	unsigned nt = std::thread::hardware_concurrency();
	if (nt < 1) nt = 1;
	if (nt > 16) nt = 16;
	uint64_t total = 0;
	std::vector<std::thread> th;
	for (auto &r : ranges) {
		const uint64_t n = r.second - r.first + 1, per = (n + nt - 1) / nt;
		total += n;
		for (unsigned i = 0; i < nt; i++) {
			const uint64_t lo = r.first + i * per;
			if (lo > r.second) break;
			const uint64_t hi = lo + per - 1 < r.second ? lo + per - 1 : r.second;
			th.emplace_back(scan, lo, hi);
		}
	}
	for (auto &t : th) t.join();
	if (bad.load()) { printf("FAILED %llu of %llu patterns differ\n", (unsigned long long)bad.load(), (unsigned long long)total); return 1; }
	printf("ok %llu\n", (unsigned long long)total);
	return 0;
}
