// planner.h FftOrder with the retune transition (FftOrder::retune, FftPushPlan::wait_retune), on the host: the model of
// tests/hostsim/fft_order_check.cpp -- a front end reduced to its launches and waits -- with a sixth call, 'R' = a retune
// (hfdl_gpu.cpp hfdl_gpu_frontend_retune_channel: held-back demodulators launched, the half being filled closed with its demodulators
// at once, then the tap FFT and retune_channelizer_kernel on stream A, whose dispatch carries the event `retune_done`), in EVERY
// sequence of up to DEPTH calls, for each rule on both kinds of geometry.  Asserted besides everything the other check asserts:
//   - the retune's kernel is ordered behind every forward FFT queued before it, on whichever stream it ran (its riders read the old
//     channelizer constants and carried NCO state), and behind the inverse FFT of every half closed before it
//   - every forward FFT queued after a retune is ordered behind the retune's kernel, on whichever stream it runs
//   - the wait for `retune_done` is only ever queued when a retune has carried it
// Prints the number of sequences and "ok".
#include <bitset>
#include <cstdio>
#include <vector>
#include "planner.h"

using namespace hfdl;

#define CHECK(cond) do { if (!(cond)) { printf("fail line %d: %s  (sequence %s, rule %d, fold_bound %d)\n", __LINE__, #cond, seq_text, (int)rule, (int)fold_bound); return false; } } while (0)

enum { A, C, B, NSTREAMS };
enum Kind { K_FFT, K_FOLD, K_IFFT, K_DEMOD, K_RETUNE };
constexpr int MAXI = 256, NEVER = -1, NOTHING = -2;      // an event no launch carries / one recorded on a stream with nothing queued
struct Item { int stream, kind, half; std::bitset<MAXI> before; };

static char seq_text[32];
static FftRule rule;
static bool fold_bound;

struct Sim {
	std::vector<Item> items;
	int last[NSTREAMS] = { NOTHING, NOTHING, NOTHING };
	std::vector<int> waits[NSTREAMS];
	int base = 0;                       // items below: complete (a sync has waited for them)
	bool ok = true;
	// the front end's state (frontend.h)
	FftOrder order;
	int half_first = 2, half_blocks = 3, half_target = 2, cur_half = 0, batch_fill = 0, halves = 0;
	int pending_half = -1;              // the closed half whose demodulators are held back (its number), -1: none
	int demod_half = -1;                // the newest half handed to the demodulator
	int chan[2] = { NEVER, NEVER }, spec[2] = { NEVER, NEVER }, fft_done = NEVER, ev_switch = NEVER;
	int last_fft = NEVER, ifft_of_half[64], ifft_of_set[2] = { NEVER, NEVER };
	int retune_done = NEVER, last_retune = NEVER, last_ifft = NEVER;
	std::vector<int> ffts_of_half;

	bool wait(int stream, int ev)
	{
		CHECK(ev != NEVER);
		if (ev >= 0) waits[stream].push_back(ev);
		return true;
	}
	int launch(int stream, int kind, int half)
	{
		Item it{ stream, kind, half, {} };
		auto after = [&](int i) { if (i >= 0) { it.before |= items[(size_t)i].before; it.before.set((size_t)i); } };
		after(last[stream]);
		for (int w : waits[stream]) after(w);
		waits[stream].clear();
		items.push_back(it);
		return last[stream] = (int)items.size() - 1;
	}
	bool ordered(int earlier, int later) const { return earlier < 0 || earlier < base || items[(size_t)later].before.test((size_t)earlier); }

	bool launch_demod(int half_no, int buf, bool after_fft)
	{
		if (after_fft) CHECK(fft_done == last_fft);
		if (!wait(B, after_fft ? fft_done : chan[buf])) return false;
		CHECK(half_no > demod_half);            // the halves are demodulated in their order
		demod_half = half_no;
		const int d = launch(B, K_DEMOD, half_no);
		CHECK(ordered(ifft_of_half[half_no], d));
		if (after_fft) CHECK(ordered(last_fft, d));
		return true;
	}
	bool flush_pending(bool after_fft)
	{
		if (pending_half < 0) return true;
		const int h = pending_half;
		pending_half = -1;
		return launch_demod(h, h & 1, after_fft);
	}
	bool enqueue_fft(bool on_device)
	{
		const int i = batch_fill, set = cur_half;
		const bool held = pending_half >= 0;
		const FftPushPlan plan = order.push(fft_side(rule, on_device), i, half_target, held);
		if (rule == FFT_RULE_SERIAL || (rule == FFT_RULE_INPUT && !on_device && !saw_device)) {
			// what the front end did before it had a choice
			CHECK(plan.side == FFT_SERIAL && !plan.wait_switch && !plan.wait_set_free && !plan.wait_first_fold && !plan.flush_before && !plan.wait_retune);
			CHECK(plan.hold_after == (held && i + 1 == half_target));
		}
		const int st = plan.side == FFT_SERIAL ? A : C;
		if (plan.flush_before && !flush_pending(false)) return false;
		if (plan.wait_switch) { ev_switch = last[st == A ? C : A]; if (!wait(st, ev_switch)) return false; }
		if (plan.wait_set_free && chan[set] != NEVER && !wait(st, chan[set])) return false;
		if (plan.wait_first_fold && !wait(st, chan[set ^ 1])) return false;
		if (plan.wait_retune && !wait(st, retune_done)) return false;
		const int f = launch(st, K_FFT, halves);
		if (plan.side == FFT_BESIDE) spec[set] = f;
		else if (plan.hold_after) fft_done = f;
		CHECK(ordered(last_fft, f));
		CHECK(ordered(last_retune, f));         // the riders of this FFT read what the retune wrote
		if (i == 0) CHECK(ordered(ifft_of_set[set], f));
		if (i == 0 && order.halves == 1) CHECK(ordered(ifft_of_set[set ^ 1], f));      // the first fold after a drain runs alone
		last_fft = f;
		ffts_of_half.push_back(f);
		if (plan.hold_after && !flush_pending(true)) return false;
		CHECK(!plan.hold_after || pending_half < 0);
		batch_fill++;
		return true;
	}
	bool close_half(bool launch_now, bool with_demod = true)
	{
		if (batch_fill == 0) return true;
		const int half = cur_half;
		const HalfClosePlan plan = order.close(launch_now);
		if (rule == FFT_RULE_SERIAL || (rule == FFT_RULE_INPUT && !saw_device)) CHECK(!plan.wait_input && plan.hold_back == !launch_now);
		if (plan.wait_input && !wait(A, spec[half])) return false;
		const int fold = launch(A, K_FOLD, halves);
		for (int f : ffts_of_half) CHECK(ordered(f, fold));
		ffts_of_half.clear();
		chan[half] = ifft_of_set[half] = ifft_of_half[halves] = last_ifft = launch(A, K_IFFT, halves);
		const int h = halves++;
		cur_half ^= 1;
		batch_fill = 0;
		if (!with_demod) return true;
		if (!plan.hold_back) return launch_demod(h, half, false);
		CHECK(pending_half < 0);                // one half is held back at a time
		pending_half = h;
		return true;
	}
	bool saw_device = false;
	bool push(bool on_device)
	{
		saw_device = saw_device || on_device;
		if (!enqueue_fft(on_device)) return false;
		if (batch_fill < half_target) return true;
		const bool r = close_half(!fold_bound);
		half_target = half_blocks;
		return r;
	}
	bool channelize(bool on_device)
	{
		saw_device = saw_device || on_device;
		return flush_pending(false) && close_half(true) && enqueue_fft(on_device) && close_half(false, false);
	}
	bool retune()
	{
		if (!flush_pending(false) || !close_half(true)) return false;
		const int r = launch(A, K_RETUNE, halves);      // (the tap FFT in front of it is on stream A too)
		retune_done = last_retune = r;
		CHECK(ordered(last_fft, r));
		CHECK(ordered(last_ifft, r));
		CHECK(batch_fill == 0 && pending_half < 0);
		order.retune();
		return true;
	}
	bool sync()
	{
		if (!flush_pending(false) || !close_half(true)) return false;
		half_target = half_first;
		base = (int)items.size();
		retune_done = NEVER;                    // nothing may wait for it any more: FftOrder::drained() forgets the retune
		order.drained();
		return true;
	}
};

int main()
{
	constexpr int DEPTH = 7, NOPS = 6;
	long sequences = 0;
	for (int r = 0; r < 3; r++)
		for (int fb = 0; fb < 2; fb++) {
			rule = (FftRule)r;
			fold_bound = fb != 0;
			for (int depth = 1; depth <= DEPTH; depth++) {
				long count = 1;
				for (int i = 0; i < depth; i++) count *= NOPS;
				for (long code = 0; code < count; code++) {
					Sim s;
					long c = code;
					for (int i = 0; i < depth; i++, c /= NOPS) seq_text[i] = "HDSxdR"[c % NOPS];
					seq_text[depth] = 0;
					bool ok = true;
					for (int i = 0; i < depth && ok; i++)
						switch (seq_text[i]) {
						case 'H': ok = s.push(false); break;
						case 'D': ok = s.push(true); break;
						case 'S': ok = s.sync(); break;
						case 'x': ok = s.channelize(false); break;
						case 'd': ok = s.channelize(true); break;
						case 'R': ok = s.retune(); break;
						}
					ok = ok && s.sync();            // what every run ends with: nothing may be left held back
					if (!ok) return 1;
					if (s.pending_half >= 0 || (int)s.items.size() >= MAXI) { printf("fail: sequence %s left a half behind\n", seq_text); return 1; }
					sequences++;
				}
			}
		}
	printf("%ld sequences\nok\n", sequences);
	return 0;
}
