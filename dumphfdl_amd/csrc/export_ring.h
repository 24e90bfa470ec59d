// export_ring.h -- the channel export's host bookkeeping (frontend.h ChannelExport): which blocks the ring on the device keeps, which of
// them are finished, where a block lives.  Plain C++, no HIP: tests/hostsim/export_ring_check.cpp compiles it alone.
//
// Blocks are numbered as hfdl_gpu_frontend_counters().blocks numbers them.  Block b lives in slot b % R.  A closed half hands its
// blocks to ONE launch; launches run in order on one stream, so the finished launches are a prefix of the launches queued.  The
// host keeps the last block of every launch not yet known to be finished, at most R of them (a launch holds a block at least, so
// the blocks of a launch R launches back have all been overwritten).
#pragma once
#include <stdint.h>

namespace hfdl {

struct ExportRing {
	uint32_t R = 0;
	uint64_t first = 0;                 // the first exported block: the block count when the export was enabled
	uint64_t end = 0;                   // one past the newest block handed to a launch (== first: nothing yet)
	uint64_t done = 0;                  // every block below has been written, or overwritten: its launch is known to have run
	uint64_t l_head = 0, l_tail = 0;    // launches [l_head, l_tail) are not known to be finished; launch l's record sits at l % R

	void start(uint32_t r, uint64_t first_block) { R = r; first = end = done = first_block; l_head = l_tail = 0; }
	uint32_t slot(uint64_t b) const { return (uint32_t)(b % R); }
	uint64_t oldest() const { return end - first > R ? end - R : first; }       // the oldest block kept: a queued launch has taken the slots below

	// A half of blocks [b0, b0 + nblk) is closed.  Returns how many of its OLDEST blocks the launch leaves out: those before `first`
	// (they waited in the open half when the export was enabled) and, of a half larger than the ring, those its own newest blocks
	// would overwrite.  The launch takes the rest (none: no launch) and is recorded by push_launch().
	uint32_t skip_of_half(uint64_t b0, uint32_t nblk) const
	{
		uint64_t skip = first > b0 ? first - b0 : 0;
		if (skip > nblk) skip = nblk;
		if (nblk - skip > R) skip = nblk - R;
		return (uint32_t)skip;
	}
	// a launch whose last block is `last` has been queued: its record goes to last_of[l_tail % R].  With R launches on record the
	// oldest is dropped: its blocks are overwritten anyway.  Returns the record's index.
	uint32_t push_launch(uint64_t *last_of, uint64_t last)
	{
		// (the dropped launch may not have run: `done` passes it only because R launches of a block at least follow it, so after this
		// call done <= oldest() and range(), which starts at oldest(), never returns a block below)
		if (l_tail - l_head == R) { done = last_of[l_head % R] + 1; l_head++; }
		const uint32_t at = (uint32_t)(l_tail % R);
		last_of[at] = last;
		l_tail++;
		end = last + 1;
		return at;
	}
	// finished(record index) -> has that launch run?  Asked oldest first, up to the first that has not.
	template <typename Finished> void settle(const uint64_t *last_of, Finished finished)
	{
		while (l_head < l_tail && finished((uint32_t)(l_head % R))) { done = last_of[l_head % R] + 1; l_head++; }
	}
	// what a read returns: consecutive finished blocks [from, to) from max(from_block, oldest kept) on, at most max_blocks
	void range(uint64_t from_block, uint64_t max_blocks, uint64_t &from, uint64_t &to) const
	{
		from = from_block > oldest() ? from_block : oldest();
		if (from > end) from = end;
		to = done > from ? done : from;
		if (to - from > max_blocks) to = from + max_blocks;
	}
};

}  // namespace hfdl
