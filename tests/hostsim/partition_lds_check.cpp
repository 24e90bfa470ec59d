// The CU partition of the fold-bound geometries (planner.h plan_cu_partition) and the demodulator's LDS carve-up (demod_lds.h DemodLds) on
// the host.  The device qualifiers demod_logic.h uses are defined here, as in hostsim.cpp.  Prints "ok".
#include <cstdio>
#include <cstdlib>
#define __device__
#define __host__
static const struct { unsigned x; } threadIdx = { 0 };
static inline int atomicAdd(int *p, int v) { int o = *p; *p += v; return o; }
static inline int __popcll(unsigned long long x) { return __builtin_popcountll(x); }
static inline int __popc(unsigned x) { return __builtin_popcount(x); }
#include "demod_lds.h"
#include "planner.h"

using namespace hfdl;

#define CHECK(cond) do { if (!(cond)) { printf("fail line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static bool bit(const uint32_t *m, int i) { return (m[i >> 5] >> (i & 31)) & 1u; }

int main()
{
	// the LDS of a workgroup does not depend on the launch's length and four workgroups fit a CU
	const size_t lds = DemodLds(1000).total;
	CHECK(DemodLds(3000).total == lds && DemodLds(5400).total == lds);
	CHECK(lds <= DM_LDS_BUDGET && 4 * lds <= (size_t)PLAN_CU_LDS);
	printf("demodulator LDS %zu bytes\n", lds);

	for (int nch : { 128, 130, 256, 512 }) {
		const CuPartition p = plan_cu_partition(nch, lds, true);
		CHECK(p.on && p.wg_per_cu == 4);
		int demod = 0, fold = 0, major[8] = {}, inter[8] = {};
		for (int i = 0; i < PLAN_CUS; i++) {
			const bool d = bit(p.mask_demod, i), f = bit(p.mask_fold, i);
			CHECK(d != f);                                   // disjoint, and together every CU
			demod += d; fold += f;
			if (d) { major[i / 32]++; inter[i % 8]++; }
		}
		CHECK(demod + fold == PLAN_CUS && demod == p.demod_cus);
		CHECK(demod * p.wg_per_cu >= nch && (demod - PLAN_XCDS) * p.wg_per_cu < nch);      // enough, and no whole round of XCDs too many
		for (int x = 0; x < 8; x++) CHECK(major[x] == demod / 8 && inter[x] == demod / 8);   // an equal share of every XCD in both numberings
	}
	CHECK(plan_cu_partition(256, lds, true).demod_cus == 64);
	// no partition where the fold does not bound the block, nor where a workgroup's LDS is unknown or too large for a CU
	for (int nch : { 1, 32, 127 }) CHECK(!plan_cu_partition(nch, lds, false).on);
	CHECK(!plan_cu_partition(256, 0, true).on && !plan_cu_partition(256, (size_t)PLAN_CU_LDS + 1, true).on);
	// a larger workgroup: three to a CU, 86 -> 88 CUs for 256 channels; channels that would take more than half the device: none
	CHECK(plan_cu_partition(256, 53 * 1024, true).wg_per_cu == 3 && plan_cu_partition(256, 53 * 1024, true).demod_cus == 88);
	CHECK(!plan_cu_partition(1024, lds, true).on);
	const CuPartition none = plan_cu_partition(64, lds, false);
	for (int w = 0; w < 8; w++) CHECK(none.mask_demod[w] == 0 && none.mask_fold[w] == 0);
	printf("ok\n");
	return 0;
}
