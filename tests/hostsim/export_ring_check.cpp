// export_ring_check.cpp -- the channel export's host bookkeeping (dumphfdl_amd/csrc/export_ring.h) without a device: which blocks the
// ring keeps, which are finished, where a block lives.  tests/test_export_ring_cpu.py builds it with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "export_ring.h"

using hfdl::ExportRing;

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

// a ring and its launch records; `finished` = launches (in launch order) known to have run
struct Sim {
	ExportRing r;
	std::vector<uint64_t> last_of;
	std::vector<char> fin;              // by record index
	uint64_t blocks;                    // the front end's block count
	Sim(uint32_t R, uint64_t first) : last_of(R), fin(R), blocks(first) { r.start(R, first); }
	// a half of nblk blocks is closed; returns the blocks the launch took (0: no launch)
	uint32_t half(uint32_t nblk, bool finished)
	{
		const uint32_t skip = r.skip_of_half(blocks, nblk);
		blocks += nblk;
		if (skip == nblk) return 0;
		const uint32_t at = r.push_launch(last_of.data(), blocks - 1);
		fin[at] = finished;
		return nblk - skip;
	}
	void finish_all() { for (auto &f : fin) f = 1; }
	void read(uint64_t from_block, uint64_t max_blocks, uint64_t &from, uint64_t &to)
	{
		r.settle(last_of.data(), [&](uint32_t at) { return fin[at] != 0; });
		r.range(from_block, max_blocks, from, to);
	}
};

int main()
{
	uint64_t a = 0, b = 0;
	{	// empty ring: nothing to return, next_block = the block count at enable; also with blocks still in an open half
		Sim s(4, 7);
		s.read(0, 100, a, b);      CHECK(a == 7 && b == 7);
		s.read(7, 100, a, b);      CHECK(a == 7 && b == 7);
		s.read(50, 100, a, b);     CHECK(a == 7 && b == 7);
		s.read(0, 0, a, b);        CHECK(a == 7 && b == 7);
		CHECK(s.r.oldest() == 7);
	}
	{	// R = 2, blocks one by one, every launch finished: the newest two are kept
		Sim s(2, 0);
		for (int i = 0; i < 5; i++) CHECK(s.half(1, true) == 1);
		CHECK(s.r.oldest() == 3 && s.r.slot(3) == 1 && s.r.slot(4) == 0);
		s.read(0, 100, a, b);      CHECK(a == 3 && b == 5);
		s.read(4, 100, a, b);      CHECK(a == 4 && b == 5);
		s.read(3, 1, a, b);        CHECK(a == 3 && b == 4);
		// R launches on record and none finished: the record of the oldest is dropped, its block is overwritten anyway
		Sim u(2, 0);
		for (int i = 0; i < 5; i++) u.half(1, false);
		CHECK(u.r.l_tail - u.r.l_head == 2 && u.r.oldest() == 3);
		u.read(0, 100, a, b);      CHECK(a == 3 && b == 3);
		u.finish_all();
		u.read(0, 100, a, b);      CHECK(a == 3 && b == 5);
	}
	{	// a half of 5 blocks into R = 4: the launch leaves the half's oldest block out and keeps blocks 1 .. 4 in slots 1, 2, 3, 0
		Sim s(4, 0);
		CHECK(s.r.skip_of_half(0, 5) == 1);
		CHECK(s.half(5, true) == 4);
		CHECK(s.r.oldest() == 1 && s.r.end == 5);
		s.read(0, 100, a, b);      CHECK(a == 1 && b == 5);
		CHECK(s.r.slot(1) == 1 && s.r.slot(4) == 0);
		// ... and behind three blocks that are kept until it is queued
		Sim t(4, 10);
		CHECK(t.half(3, true) == 3);
		t.read(0, 100, a, b);      CHECK(a == 10 && b == 13);
		CHECK(t.half(5, false) == 4);
		t.read(0, 100, a, b);      CHECK(a == 14 && b == 14);       // queued, not finished: the old blocks are gone, the new ones not there yet
		t.finish_all();
		t.read(0, 100, a, b);      CHECK(a == 14 && b == 18);
	}
	{	// the enable boundary: blocks waiting in the open half when the export was enabled are left out
		Sim s(8, 2);
		s.blocks = 0;                      // the half being filled holds blocks 0, 1 (pushed before the enable) ...
		CHECK(s.r.skip_of_half(0, 4) == 2);
		CHECK(s.half(4, true) == 2);       // ... and 2, 3
		s.read(0, 100, a, b);      CHECK(a == 2 && b == 4);
		Sim t(8, 2);
		t.blocks = 0;
		CHECK(t.half(2, true) == 0);       // only old blocks: no launch
		t.read(0, 100, a, b);      CHECK(a == 2 && b == 2);
	}
	{	// from_block before, inside and after the kept range; R = 4, ten blocks one by one
		Sim s(4, 0);
		for (int i = 0; i < 10; i++) s.half(1, true);
		s.read(0, 100, a, b);      CHECK(a == 6 && b == 10);
		s.read(8, 100, a, b);      CHECK(a == 8 && b == 10);
		s.read(10, 100, a, b);     CHECK(a == 10 && b == 10);
		s.read(1000, 100, a, b);   CHECK(a == 10 && b == 10);
		s.read(7, 2, a, b);        CHECK(a == 7 && b == 9);
		for (uint64_t k = 6; k < 10; k++) CHECK(s.r.slot(k) == k % 4);
	}
	{	// a finished prefix that ends inside a launch's successor: launches of 3, 2 and 4 blocks, the first finished
		Sim s(16, 0);
		s.half(3, true); s.half(2, false); s.half(4, false);
		s.read(0, 100, a, b);      CHECK(a == 0 && b == 3);
		s.read(1, 100, a, b);      CHECK(a == 1 && b == 3);
		s.read(4, 100, a, b);      CHECK(a == 4 && b == 4);         // inside the unfinished launch: nothing yet, and nothing skipped
		s.fin[1] = 1;
		s.read(4, 100, a, b);      CHECK(a == 4 && b == 5);
		s.fin[2] = 1;
		s.read(5, 100, a, b);      CHECK(a == 5 && b == 9);
		// a later launch reported finished before an earlier one is not believed: launches run in order
		Sim t(16, 0);
		t.half(2, false); t.half(2, true);
		t.read(0, 100, a, b);      CHECK(a == 0 && b == 0);
	}
	printf("ok\n");
	return 0;
}
