// The padded channel layout of a front end of several receivers (planner.h plan_receiver_slots, fold_group_tables) on the host: channels
// -> slots is injective and order-preserving per receiver, no octet of slots holds two receivers' channels, the padding slots are the
// ones past each receiver's channels, and for every workgroup width every octet is handed to exactly one workgroup, whose octets all
// belong to one receiver and whose channel mapping is that receiver's.  Prints "ok".
#include <cstdio>
#include <set>
#include <vector>
#include "planner.h"

using namespace hfdl;

static int check(const std::vector<int32_t> &nch, int group)
{
	std::vector<RxSpan> rx;
	const int32_t total = plan_receiver_slots(nch.data(), (int32_t)nch.size(), group, rx);
	std::vector<int> owner((size_t)total, -1);               // receiver of each slot's channel, -1: padding
	std::set<int32_t> used;
	int32_t c = 0;
	for (size_t r = 0; r < rx.size(); r++) {
		if (rx[r].slot0 % group || rx[r].slots % group || rx[r].slots < nch[r] || rx[r].slots >= nch[r] + group || rx[r].chan0 != c) return 1;
		for (int32_t i = 0; i < nch[r]; i++, c++) {
			const int32_t s = receiver_slot(rx[r], c);
			if (s < 0 || s >= total || !used.insert(s).second) return 2;
			if (s != rx[r].slot0 + i) return 3;
			owner[(size_t)s] = (int)r;
		}
		for (int32_t s = rx[r].slot0; s < rx[r].slot0 + rx[r].slots; s++)
			if (owner[(size_t)s] != (int)r && owner[(size_t)s] != -1) return 4;
	}
	if ((int32_t)used.size() != c) return 5;
	// no group of slots holds channels of two receivers
	for (int32_t g0 = 0; g0 < total; g0 += group) {
		std::set<int> rs;
		for (int32_t s = g0; s < g0 + group; s++) if (owner[(size_t)s] >= 0) rs.insert(owner[(size_t)s]);
		if (rs.size() > 1) return 6;
	}
	if (group != 8) return 0;
	const int32_t noct = total / 8;
	const int pw_max = 16;
	const std::vector<FoldGroup> t = fold_group_tables(rx, noct, pw_max);
	for (int pw = 1; pw <= pw_max; pw++) {
		int groups = 0, rest = 0;
		for (const RxSpan &r : rx) { groups += r.slots / 8 / pw; rest += r.slots / 8 % pw; }
		std::vector<int> seen((size_t)noct, 0);
		for (int e = 0; e < groups + rest; e++) {
			const FoldGroup &f = t[(size_t)(pw - 1) * noct + e];
			const int width = e < groups ? pw : 1;
			const RxSpan &r = rx[(size_t)f.rx];
			if (f.slot_end != r.slot0 + r.nch || f.to_chan != r.chan0 - r.slot0) return 7;
			for (int o = f.octet; o < f.octet + width; o++) {
				if (o < 0 || o >= noct || seen[(size_t)o]++) return 8;
				if (8 * o < r.slot0 || 8 * o + 8 > r.slot0 + r.slots) return 9;        // the workgroup stays inside its receiver
			}
		}
		for (int o = 0; o < noct; o++) if (seen[(size_t)o] != 1) return 10;
	}
	return 0;
}

int main()
{
	const std::vector<std::vector<int32_t>> cases = {
		{ 1 }, { 8 }, { 256 }, { 1, 3, 9 }, { 70, 5, 66 }, { 6, 6 }, { 32, 32, 32, 32 }, { 2, 2, 2, 2, 2, 2, 2, 2 }, { 7, 9, 15, 17, 1 },
	};
	std::vector<std::vector<int32_t>> all = cases;
	unsigned s = 12345;
	for (int k = 0; k < 200; k++) {
		std::vector<int32_t> v;
		const int nrx = 1 + (int)((s = s * 1103515245u + 12345u) >> 16) % 64;
		for (int r = 0; r < nrx; r++) v.push_back(1 + (int)((s = s * 1103515245u + 12345u) >> 16) % 80);
		all.push_back(v);
	}
	for (const auto &c : all)
		for (int group : { 1, 8 }) {
			const int rc = check(c, group);
			if (rc) { printf("fail %d (group %d, %zu receivers)\n", rc, group, c.size()); return 1; }
		}
	printf("ok\n");
	return 0;
}
