// planner.h DemodOrder on the host: a closed half's way through the demodulator (stream B) and the burst decoder (stream D), in the model
// of tests/hostsim/fft_order_check.cpp -- a front end reduced to its launches and waits, every item carrying the set of items ordered
// before it.  The calls are hfdl_gpu.cpp's (push, close_half, flush_pending_demod, channelize_block, push_baseband, retune, sync,
// poll_pdus_ready) and Demod::launch_half / collect_ready, in their order; every index and every wait the demodulator's side needs is
// DemodOrder's answer.  Streams: A (of the channelizer only what matters here: forward FFTs, inverse FFTs, the retune's kernel), B and D;
// in half of the runs D is an alias of B.  Halves of 3 blocks, the first after a drain of 2; 1, 2 or 3 blocks per demodulator launch;
// a demodulator-bound and a fold-bound geometry (the latter holds a half's demodulators back behind the next half's forward FFTs).
// EVERY sequence of up to DEPTH calls out of { H push a host block, S sync, P / p poll_pdus_ready with max_in_flight 1 / 2,
// B push_baseband, x channelize-only block, R retune }.  Asserted, by the resources a kernel touches and not by launch numbers alone:
//   1. a demodulator starts only after every kernel that used its frame queue set or its frame counter before, and the demodulator of
//      launch i after the decoder of launch i - 2 in particular: "done" of a decoder is established no later than the start of the
//      demodulator two launches on, the premise of frame_slots_check.cpp.  A decoder zeroes a counter only after its users before
//   2. the decoder of a launch is ordered after the launch's demodulator
//   3. an inverse FFT into a half is ordered after the last demodulator launch that read the half, and the half is not one whose
//      demodulators are still held back; a half's demodulators follow its inverse FFT
//   4. the snapshot slot a poll reads is never one that a queued, unfinished decoder can still write: every queued decoder that writes
//      it is known to be done by what the poll waited for or found done, or sits behind a decoder the poll has just found unfinished
//      -- for every answer the poll's queries can get
//   -  no wait is ever queued for an event that no launch carried, and a poll asks after a half that has been launched
// Usage: demod_order_check                  the rule as it is: prints "<sequences> sequences" and "ok"
//        demod_order_check drop-b | drop-a | drop-d | drop-ifft     one wait left out (B's for the decoder of launch i - 2, A's for the same,
//                                           D's for the demodulator, the inverse FFT's for the half's last demodulator)
//        demod_order_check wrong-slot       a poll reads the other snapshot slot
//                                           each must print "<sequences> violated" (exit 0); "ok" there is exit 1
#include <bitset>
#include <cstdio>
#include <cstring>
#include <vector>
#include "planner.h"

using namespace hfdl;

#define CHECK(cond) do { if (!(cond)) { if (!mutation) printf("fail line %d: %s  (sequence %s, batch %d, fold_bound %d, own decode stream %d)\n", __LINE__, #cond, seq_text, batch, (int)fold_bound, (int)own_decode); return false; } } while (0)

enum { A, B, D, NSTREAMS };
enum Kind { K_FFT, K_IFFT, K_DEMOD, K_DECODE, K_RETUNE };
enum Mutation { M_NONE, M_DROP_B, M_DROP_A, M_DROP_D, M_DROP_IFFT, M_WRONG_SLOT };
constexpr int MAXI = 256, NEVER = -1, NOTHING = -2;      // an event no launch carries / one recorded on a stream with nothing queued
constexpr int HALF_BLOCKS = 3, HALF_FIRST = 2;
typedef std::bitset<MAXI> Set;
struct Item { int stream, kind; Set before; };

static char seq_text[32];
static int batch;
static bool fold_bound, own_decode;
static Mutation mutation = M_NONE;

struct Sim {
	std::vector<Item> items;
	int last[NSTREAMS] = { NOTHING, NOTHING, NOTHING };
	std::vector<int> waits[NSTREAMS];
	int base = 0;                       // items below: complete (a sync has waited for them)
	// the front end's state (frontend.h) and the demodulator's (demod.h)
	FftOrder forder;
	DemodOrder order;
	int half_target = HALF_FIRST, cur_half = 0, batch_fill = 0;
	int pending_buf = -1, pending_nblk = 0;
	int chan[2] = { NEVER, NEVER }, fft_done = NEVER;
	int dm[2][HALF_BLOCKS], ev_dec[2] = { NEVER, NEVER }, ev_demod[3] = { NEVER, NEVER, NEVER };
	// what the assertions look at
	std::vector<int> dem, dec;          // demodulator / decoder of launch i
	std::vector<int> set_users[2], counter_users[4];      // the kernels that touched a frame queue set / a frame counter last
	std::vector<int> snap_writers[2];   // the decoders that write a snapshot slot
	int last_reader[2] = { NEVER, NEVER };      // the last demodulator launch that read a half
	int handed = 0, launched = 0;       // halves handed to the demodulator / launched

	Sim() { order.own_decode = own_decode; for (auto &h : dm) for (int &e : h) e = NEVER; }
	int sd() const { return own_decode ? D : B; }
	bool wait(int stream, int ev)
	{
		CHECK(ev != NEVER);
		if (ev >= 0) waits[stream].push_back(ev);
		return true;
	}
	int launch(int stream, int kind)
	{
		Item it{ stream, kind, {} };
		auto after = [&](int i) { if (i >= 0) { it.before |= items[(size_t)i].before; it.before.set((size_t)i); } };
		after(last[stream]);
		for (int w : waits[stream]) after(w);
		waits[stream].clear();
		items.push_back(it);
		return last[stream] = (int)items.size() - 1;
	}
	bool ordered(int earlier, int later) const { return earlier < 0 || earlier < base || items[(size_t)later].before.test((size_t)earlier); }
	bool all_ordered(const std::vector<int> &earlier, int later) const
	{
		for (int e : earlier) if (!ordered(e, later)) return false;
		return true;
	}

	// Demod::launch_half
	bool launch_half(int buf, int nblk, int ready)
	{
		CHECK(buf == order.newest && launched == handed - 1);      // launches follow their hand-over: the half is the newest
		if (ready != NOTHING && !wait(B, ready)) return false;      // (push_baseband has no event: the half was filled by a copy the host waited for)
		const int k = (nblk + batch - 1) / batch;
		for (int j0 = 0, l = 0; j0 < nblk; j0 += batch, l++) {
			const size_t i = (size_t)order.launches;
			const DemodLaunch p = order.launch(l, k);
			CHECK(p.set >= 0 && p.set < 2 && p.counter >= 0 && p.counter < 4 && p.zeroed >= 0 && p.zeroed < 4 && p.zeroed != p.counter);
			CHECK(p.done_event >= 0 && p.done_event < HALF_BLOCKS && (p.done_event == 0) == (l == k - 1));
			if (p.wait_decoder && mutation != M_DROP_B && !wait(B, ev_dec[p.set])) return false;
			const int d = dm[buf][p.done_event] = launch(B, K_DEMOD);
			CHECK(ordered(chan[buf], d));                       // 3: the half has been filled
			CHECK(all_ordered(set_users[p.set], d));            // 1
			CHECK(all_ordered(counter_users[p.counter], d));
			if (i >= 2) CHECK(ordered(dec[i - 2], d));
			if (own_decode && mutation != M_DROP_D && !wait(D, d)) return false;
			const int e = launch(sd(), K_DECODE);
			CHECK(ordered(d, e));                               // 2
			CHECK(all_ordered(counter_users[p.zeroed], e));     // 1: the counter it zeroes has no user left
			set_users[p.set] = { d, e };
			counter_users[p.counter] = { d, e };
			counter_users[p.zeroed] = { e };
			snap_writers[buf].push_back(e);
			if (own_decode) ev_dec[p.set] = e;
			dem.push_back(d);
			dec.push_back(e);
			last_reader[buf] = d;
		}
		ev_demod[order.decoded_event(0)] = last[sd()];
		launched++;
		return true;
	}
	bool flush_pending(bool after_fft)
	{
		if (pending_buf < 0) return true;
		const int buf = pending_buf;
		pending_buf = -1;
		return launch_half(buf, pending_nblk, after_fft ? fft_done : chan[buf]);
	}
	bool enqueue_fft()
	{
		const FftPushPlan plan = forder.push(FFT_SERIAL, batch_fill, half_target, pending_buf >= 0);
		const int f = launch(A, K_FFT);
		if (plan.hold_after) fft_done = f;
		if (plan.hold_after && !flush_pending(true)) return false;
		batch_fill++;
		return true;
	}
	bool close_half(bool launch_now, bool with_demod = true)
	{
		const int nblk = batch_fill;
		if (nblk == 0) return true;
		const int half = cur_half;
		const HalfClosePlan plan = forder.close(launch_now);
		if (dm[half][0] != NEVER && mutation != M_DROP_IFFT && !wait(A, dm[half][0])) return false;      // Demod::half_read_event
		if (with_demod && own_decode && !fold_bound) {
			const bool any = order.wait_on_a();                 // Demod::frames_free_event
			if (any && mutation != M_DROP_A && !wait(A, ev_dec[order.next_set()])) return false;
		}
		CHECK(pending_buf != half);                             // 3: not over a half still to be demodulated
		const int f = chan[half] = launch(A, K_IFFT);
		CHECK(ordered(last_reader[half], f));                   // 3
		cur_half ^= 1;
		batch_fill = 0;
		if (!with_demod) return true;
		order.hand_over(half);
		handed++;
		if (!plan.hold_back) return launch_half(half, nblk, chan[half]);
		CHECK(pending_buf < 0);
		pending_buf = half;
		pending_nblk = nblk;
		return true;
	}
	bool push()
	{
		if (!enqueue_fft()) return false;
		if (batch_fill < half_target) return true;
		const bool r = close_half(!fold_bound);
		half_target = HALF_BLOCKS;
		return r;
	}
	bool channelize() { return flush_pending(false) && close_half(true) && enqueue_fft() && close_half(false, false); }
	bool retune()
	{
		if (!flush_pending(false) || !close_half(true)) return false;
		launch(A, K_RETUNE);
		launch(B, K_RETUNE);            // the state reset behind the demodulators
		launch(sd(), K_RETUNE);         // the PDU frequency behind the burst decoders
		forder.retune();
		return true;
	}
	bool sync()
	{
		if (!flush_pending(false) || !close_half(true)) return false;
		half_target = HALF_FIRST;
		base = (int)items.size();
		forder.drained();
		return true;
	}
	bool push_baseband()
	{
		if (!sync()) return false;
		const int half = cur_half;
		cur_half ^= 1;
		order.hand_over(half);
		handed++;
		return launch_half(half, 1, NOTHING);
	}
	// Demod::collect_ready.  `known`: what the poll knows to be complete
	bool poll(int max_in_flight)
	{
		const int half = order.poll_half();
		if (half < 0) return true;
		CHECK(launched >= handed - 1);                          // the half before the newest is never one still held back
		const int ev = dm[half][0], e1 = order.decoded_event(1), e2 = order.decoded_event(2);
		CHECK(e1 >= 0 && e1 != order.decoded_event(0) && e2 != order.decoded_event(0) && e2 != e1);
		const int last_dec = ev_demod[e1], older_dec = e2 >= 0 ? ev_demod[e2] : NOTHING;
		CHECK(ev != NEVER && last_dec != NEVER && older_dec != NEVER);
		(void)max_in_flight;            // 1 waits for `ev`; 2 asks after it and reads nothing unless it is done: from here on the two are one
		Set known;
		auto learn = [&](Set &s, int i) { if (i >= 0) { s |= items[(size_t)i].before; s.set((size_t)i); } };
		auto is_known = [&](int i) { return i < base || known.test((size_t)i); };
		learn(known, ev);
		// what the two queries can answer: the half's last decoder done; not done and the last decoder of the half before it done; neither
		for (int answer = 0; answer < 3; answer++) {
			const bool decoded = answer == 0, older = answer == 1;
			if (!decoded && is_known(last_dec)) continue;       // the query cannot say "not ready"
			if (older && e2 < 0) continue;
			if (answer == 2 && e2 >= 0 && is_known(older_dec)) continue;
			Set done = known;
			if (decoded) learn(done, last_dec);
			if (older) learn(done, older_dec);
			int slot = order.snapshot_slot(decoded, older);
			if (slot < 0) continue;                             // nothing is read
			if (mutation == M_WRONG_SLOT) slot ^= 1;
			for (int w : snap_writers[slot]) {
				if (w < base || done.test((size_t)w)) continue;
				CHECK(!decoded && items[(size_t)w].before.test((size_t)last_dec));     // 4: behind a decoder just found unfinished, it has not started
			}
		}
		return true;
	}
};

int main(int argc, char **argv)
{
	static const char *const names[] = { "", "drop-b", "drop-a", "drop-d", "drop-ifft", "wrong-slot" };
	if (argc > 1) {
		for (int m = 1; m < 6; m++) if (!strcmp(argv[1], names[m])) mutation = (Mutation)m;
		if (mutation == M_NONE) { printf("unknown argument %s\n", argv[1]); return 2; }
	}
	constexpr int DEPTH = 6, NOPS = 7;
	long sequences = 0;
	for (batch = 1; batch <= 3; batch++)
		for (int fb = 0; fb < 2; fb++)
			for (int own = 0; own < 2; own++) {
				fold_bound = fb != 0;
				own_decode = own != 0;
				for (int depth = 1; depth <= DEPTH; depth++) {
					long count = 1;
					for (int i = 0; i < depth; i++) count *= NOPS;
					for (long code = 0; code < count; code++) {
						Sim s;
						long c = code;
						for (int i = 0; i < depth; i++, c /= NOPS) seq_text[i] = "HSPpBxR"[c % NOPS];
						seq_text[depth] = 0;
						bool ok = true;
						for (int i = 0; i < depth && ok; i++)
							switch (seq_text[i]) {
							case 'H': ok = s.push(); break;
							case 'S': ok = s.sync(); break;
							case 'P': ok = s.poll(1); break;
							case 'p': ok = s.poll(2); break;
							case 'B': ok = s.push_baseband(); break;
							case 'x': ok = s.channelize(); break;
							case 'R': ok = s.retune(); break;
							}
						ok = ok && s.poll(2) && s.sync();       // what every run ends with: nothing may be left held back
						sequences++;
						if (!ok && mutation) { printf("%ld violated\n", sequences); return 0; }
						if (!ok) return 1;
						if (s.pending_buf >= 0 || s.launched != s.handed || (int)s.items.size() >= MAXI) { printf("fail: sequence %s left a half behind\n", seq_text); return 1; }
					}
				}
			}
	if (mutation) { printf("%ld ok: survives %s\n", sequences, names[mutation]); return 1; }
	printf("%ld sequences\nok\n", sequences);
	return 0;
}
