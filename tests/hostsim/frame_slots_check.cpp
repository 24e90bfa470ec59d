// planner.h plan_frame_slots on the host: the frame records per channel and set (F) and the data slots per channel (S) that a launch's
// signal time asks for, stepped under adversarial schedules.
//
// The model is the front end's, reduced to what the rule depends on.  Signal time runs on; a channel's frames END at least T_F apart; the
// data symbols of a frame are written into the channel's current slot from right after the frame before ended (the earliest a framer could
// start on them) until the frame's own end, when its record is queued in the set of the launch at hand (launch i: set i & 1) and the
// channel moves on to the next slot of its ring.  Launches cut the signal anywhere, each covering at most T_L, one-block launches included.
// The burst decoder of launch i reads the records of its set and their slots; it is done at some moment that is only known to lie before
// the demodulator of launch i + 2 starts (planner.h DemodOrder, hazard 1: the wait goes there), so until then neither its set nor the slots of its
// frames may be written.
//
// Checked in every step: no write touches a slot whose frame has not been read yet; no set holds more than F records of one channel.
// Usage: frame_slots_check            the rule as planner.h states it: prints "<steps> ok"
//        frame_slots_check S-1 | F-1  one slot / one record fewer: must print "<steps> violated" (exit 0); "ok" there is exit 1
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "planner.h"

using namespace hfdl;

struct Channel {
	double prev_end, next_end;       // the end of the frame before (its successor's symbols are written from then on) and of the frame at hand
	int slot = 0;
	std::vector<long> free_from;     // per slot: the launch from which it may be written again
};

enum Decoder { DEC_RANDOM, DEC_LATEST };

// One schedule: `nlaunch` launches over `nch` channels.  gap(): distance from a frame's end to the next one's (>= T_F); cut(): a launch's length
// (0 < .. <= T_L).  Returns the number of violations; *steps counts the events looked at.
template <class Gap, class Cut>
static long run(int F, int S, int nch, int nlaunch, double first_end, Gap gap, Cut cut, Decoder dec, std::mt19937_64 &rng, long *steps)
{
	std::vector<Channel> ch((size_t)nch);
	for (int c = 0; c < nch; c++) {
		ch[(size_t)c].prev_end = -1e9;
		ch[(size_t)c].next_end = first_end + (c ? gap() - PLAN_MIN_FRAME_S : 0.0);
		ch[(size_t)c].free_from.assign((size_t)S, 0);
	}
	long bad = 0;
	double t0 = 0;
	std::uniform_real_distribution<double> u01(0.0, 1.0);
	for (long i = 0; i < nlaunch; i++) {
		const double t1 = t0 + cut();
		// when the decoder of launch i - 1 is done, as a moment of launch i's signal time: anywhere in it, or at its very end
		const double prev_decoder_done = dec == DEC_LATEST ? t1 : t0 + (t1 - t0) * u01(rng);
		for (Channel &k : ch) {
			int in_set = 0;
			// the frame at hand is written over (max(prev_end, t0), min(next_end, t1)): its slot must be free for this launch
			for (;;) {
				const double w0 = k.prev_end > t0 ? k.prev_end : t0, w1 = k.next_end < t1 ? k.next_end : t1;
				(*steps)++;
				if (w0 < w1) {
					const long ff = k.free_from[(size_t)k.slot];
					// held by a frame of launch i or later: its decoder has not even started.  Held by one of launch i - 1: written before that decoder is done?
					if (ff > i + 1 || (ff == i + 1 && w0 < prev_decoder_done)) bad++;
				}
				if (k.next_end >= t1) break;
				// the frame ends in this launch: its record goes to this launch's set, its slot to this launch's decoder
				if (++in_set > F) bad++;
				k.free_from[(size_t)k.slot] = i + 2;
				k.slot = k.slot + 1 < S ? k.slot + 1 : 0;
				k.prev_end = k.next_end;
				k.next_end += gap();
			}
		}
		t0 = t1;
	}
	return bad;
}

static long campaign(double t_launch, int dS, int dF, long *steps)
{
	const FrameSlots fs = plan_frame_slots(t_launch);
	const int F = fs.per_channel + dF, S = fs.data_slots + dS;
	if (F < 1 || S < 1) return 1;
	const double TF = PLAN_MIN_FRAME_S;
	std::mt19937_64 rng(1234567u + (unsigned)(t_launch * 1000));
	std::uniform_real_distribution<double> u01(0.0, 1.0);
	long bad = 0;
	// 1. the tightest schedule: frames back to back, full launches, the first frame ending right behind a launch's start, every decoder
	//    done as late as it may be
	for (int k = 0; k < 64; k++) {
		const double first = t_launch * 3 + 1e-6 + k * (t_launch / 64.0);
		bad += run(F, S, 1, 400, first, [&] { return TF; }, [&] { return t_launch; }, DEC_LATEST, rng, steps);
	}
	// 2. random schedules: gaps of T_F plus a little or a lot, launches of any length up to T_L with runs of one-block launches (T_L / 32),
	//    decoders done anywhere
	for (int trial = 0; trial < 300; trial++) {
		const double slack = trial % 3 == 0 ? 0.0 : (trial % 3 == 1 ? 0.05 : 3.0);
		const int mode = trial % 5;
		auto gap = [&] { return TF + slack * u01(rng) * u01(rng); };
		auto cut = [&] {
			if (mode == 0) return t_launch;
			if (mode == 1) return u01(rng) < 0.5 ? t_launch : t_launch / 32.0;
			if (mode == 2) return t_launch * (1.0 - 0.02 * u01(rng));
			return t_launch * (u01(rng) < 0.3 ? 1.0 : (0.001 + 0.999 * u01(rng)));
		};
		bad += run(F, S, 6, 600, t_launch * u01(rng), gap, cut, trial & 1 ? DEC_LATEST : DEC_RANDOM, rng, steps);
	}
	return bad;
}

int main(int argc, char **argv)
{
	const int dS = argc > 1 && !strcmp(argv[1], "S-1") ? -1 : 0, dF = argc > 1 && !strcmp(argv[1], "F-1") ? -1 : 0;
	// the figures the documents state
	const FrameSlots one_s = plan_frame_slots(0.999), cfg3 = plan_frame_slots(31734.0 / 5400.0);
	if (one_s.per_channel != 1 || one_s.data_slots != 2 || cfg3.per_channel != 3 || cfg3.data_slots != 7) { printf("fail: figures\n"); return 1; }
	// launches of a second, of the test geometry's half (3.67 s), of cfg3's (5.87 s), the longest the output counts allow (6.07 s) and a few between
	const double launches[] = { 0.999, 1.84, 2.5, 3.67, 4.7, 31734.0 / 5400.0, 32767.0 / 5400.0 };
	long steps = 0;
	for (double tl : launches) {
		const long bad = campaign(tl, dS, dF, &steps);
		if (dS == 0 && dF == 0 && bad) { printf("fail: T_L %.3f: %ld violations with F = %d, S = %d\n", tl, bad, plan_frame_slots(tl).per_channel, plan_frame_slots(tl).data_slots); return 1; }
		if ((dS || dF) && !bad) { printf("%ld ok: T_L %.3f survives %s\n", steps, tl, argv[1]); return 1; }
	}
	printf("%ld %s\n", steps, dS || dF ? "violated" : "ok");
	return 0;
}
