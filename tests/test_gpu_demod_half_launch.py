"""A half that closes full is ONE demodulator launch: several frames of a channel can end inside it, and a channel's data symbols live in a
ring of slots (planner.h plan_frame_slots, demod_logic.h on_symbol, the burst decoder's frame queue).

250 ksps, three channels: blocks of 28 672 samples (0.1147 s).  With HFDL_GPU_FOLD_BATCH=32 a half holds 32 blocks and its demodulator launch
spans 3.67 s -- more than a single-slot frame (2.344 s), so two frames of a channel can END in one launch (two records per channel and set)
and a channel has five data slots.  Every case compares every field of every PDU and every channel statistic with a launch per block
(HFDL_GPU_DEMOD_BATCH=1: at most one frame per launch, as ever) of the same calls."""
import numpy as np
import pytest

import hfdl_synth as synth

pytestmark = pytest.mark.gpu

FS, CF = 250000, 10_000_000
FREQS = [9_958_000, 10_021_000, 10_061_000]
BLOCK = 28672                                   # input samples per block at 250 ksps
HALF = 32
T_FRAME = synth.burst_symbols_len(0) / synth.SYMBOL_RATE        # 4219 symbols: 2.344 s, every single-slot mode
GAP = 0.05
MARGIN = 0.05                                   # a frame's end as the demodulator sees it lags the burst's by the filters' delays: milliseconds
SLOTS = 5                                       # plan_frame_slots(32 blocks of 0.1147 s): floor(2 x 3.676 / 2.095) + 2


def burst_plan(freqs, starts, count, seed):
    """Back-to-back single-slot bursts on every channel, modes cycling."""
    rng = np.random.default_rng(seed)
    bursts = []
    for ci, (f, t) in enumerate(zip(freqs, starts)):
        for k in range(count[ci]):
            mode = (ci + k) % 4
            bursts.append(dict(freq=f, mode=mode, octets=synth.make_pdu(rng, mode), t0=t, amp=0.08 + 0.01 * ci, cfo=3.0 * (ci - 1)))
            t += T_FRAME + GAP
    return bursts


def frame_ends(bursts, freq):
    return sorted(b["t0"] + T_FRAME for b in bursts if b["freq"] == freq)


def ends_per_launch(ends, bounds, block_s):
    """Frame ends (s) that lie safely inside each launch [bounds[i], bounds[i + 1]) (in blocks)."""
    return [sum(1 for e in ends if bounds[i] * block_s + MARGIN < e < bounds[i + 1] * block_s - MARGIN) for i in range(len(bounds) - 1)]


def run(gpu, monkeypatch, fs, cf, freqs, x, block, demod_batch, fold_batch=HALF, polls=(), timers=False):
    """Push the blocks of x; a draining poll after every block index in `polls` and at the end."""
    monkeypatch.setenv("HFDL_GPU_FOLD_BATCH", str(fold_batch))
    if demod_batch is None:
        monkeypatch.delenv("HFDL_GPU_DEMOD_BATCH", raising=False)
    else:
        monkeypatch.setenv("HFDL_GPU_DEMOD_BATCH", str(demod_batch))
    fe = gpu.Frontend(fs, cf, freqs)
    try:
        assert fe.input_size == block
        if timers:
            fe.reset_timers(True)
        got = []
        for b in range(len(x) // block):
            fe.push_block(x[b * block:(b + 1) * block])
            if b in polls:
                got += fe.poll_pdus()
        got += fe.poll_pdus()
        return dict(pdus=sorted(got, key=lambda p: (p["freq"], p["sample_index"])), stats=fe.all_channel_stats(),
                    batch=fe.geometry.demod_batch, fold=fe.geometry.fold_batch, launches=fe.demod_time_ms()[1:] if timers else None)
    finally:
        fe.close()


def same(got, ref):
    assert got["pdus"] == ref["pdus"]            # every field of every PDU
    assert got["stats"] == ref["stats"]          # every channel statistic


@pytest.fixture(scope="module")
def traffic():
    """19.6 s: eight frames in a row on channel 0 (more than its five data slots), seven and six on the others.  Channel 1's first frame
    ends 0.1 s into the second launch (blocks 32 .. 63: 3.670 .. 7.340 s), see test_a_third_frame_starts_in_the_launch_that_ended_two."""
    bursts = burst_plan(FREQS, [0.10, 3.770 - T_FRAME, 2.05], [8, 7, 6], seed=41)
    dur = 19.6
    assert max(b["t0"] for b in bursts) + T_FRAME < dur - 0.2
    x = synth.synth_wideband(FS, CF, int(dur * FS), bursts, noise_sigma=0.004, seed=43)
    return bursts, x[:len(x) // BLOCK * BLOCK]


@pytest.fixture(scope="module")
def per_block(gpu, traffic):
    """The reference: a launch per block, the whole stream."""
    mp = pytest.MonkeyPatch()
    try:
        ref = run(gpu, mp, FS, CF, FREQS, traffic[1], BLOCK, 1)
    finally:
        mp.undo()
    assert ref["batch"] == 1 and ref["fold"] == HALF
    assert len(ref["pdus"]) == len(traffic[0]), "every burst of this input decodes with a launch per block"
    return ref


@pytest.fixture(scope="module")
def per_half(gpu, traffic):
    mp = pytest.MonkeyPatch()
    try:
        return run(gpu, mp, FS, CF, FREQS, traffic[1], BLOCK, None, timers=True)
    finally:
        mp.undo()


def test_two_frames_of_a_channel_end_in_one_launch(traffic, per_block, per_half):
    bursts, x = traffic
    nblk = len(x) // BLOCK
    bounds = list(range(0, nblk, HALF)) + [nblk]
    block_s = BLOCK / FS
    # from the burst plan and the launch boundaries alone: on at least one channel two frames end inside one 32-block launch
    per_channel = [ends_per_launch(frame_ends(bursts, f), bounds, block_s) for f in FREQS]
    assert any(max(n) >= 2 for n in per_channel), per_channel
    assert per_half["batch"] == HALF and per_half["fold"] == HALF
    assert per_half["launches"] == (len(bounds) - 1, nblk)         # one launch per half closed full, one for the rest
    same(per_half, per_block)


def test_a_third_frame_starts_in_the_launch_that_ended_two(traffic, per_block, per_half):
    """Channel 1: two frames end in the second launch and the data symbols of a third begin in it, before that launch's burst decoder can
    have read the first: with two data slots they would land on the first frame's symbols.  From the burst plan alone."""
    bursts, _ = traffic
    t0, t1 = HALF * BLOCK / FS, 2 * HALF * BLOCK / FS
    mine = sorted((b for b in bursts if b["freq"] == FREQS[1]), key=lambda b: b["t0"])
    ends = [b["t0"] + T_FRAME for b in mine]
    preamble = (synth.PREKEY_LEN + 2 * 127 + 127 + 15 + 9 * 15) / synth.SYMBOL_RATE        # a frame's first data symbol follows its start by this
    assert t0 + MARGIN < ends[0] < ends[1] < t1 - MARGIN
    assert mine[2]["t0"] + preamble < t1 - 0.4, "0.4 s of the third frame's data symbols, 700 of them, are written in that launch"
    got = [p for p in per_half["pdus"] if p["freq"] == FREQS[1]]
    assert [(p["mode"], p["octets"][:len(b["octets"])]) for p, b in zip(got, mine)] == [(b["mode"], b["octets"]) for b in mine]
    same(per_half, per_block)


def test_the_data_slots_wrap(traffic, per_block, per_half):
    bursts, _ = traffic
    assert len(frame_ends(bursts, FREQS[0])) > SLOTS
    assert per_block["stats"][0]["frames"] > SLOTS and per_half["stats"][0]["frames"] == per_block["stats"][0]["frames"]
    same(per_half, per_block)
    # what came out is what was sent, channel by channel in order
    for f in FREQS:
        sent = [(b["mode"], b["octets"]) for b in sorted((b for b in bursts if b["freq"] == f), key=lambda b: b["t0"])]
        got = [(p["mode"], p["octets"][:len(o)]) for p, (_, o) in zip((p for p in per_half["pdus"] if p["freq"] == f), sent)]
        assert got == sent


@pytest.mark.parametrize("polls", [(), (40,)], ids=["32+32+5", "poll-in-a-half"])
def test_ragged_and_polled_halves(gpu, monkeypatch, traffic, polls):
    """69 blocks: two full halves and five blocks; with a draining poll after block 40 the second half closes at 9 blocks."""
    x = traffic[1][:69 * BLOCK]
    ref = run(gpu, monkeypatch, FS, CF, FREQS, x, BLOCK, 1, polls=polls)
    got = run(gpu, monkeypatch, FS, CF, FREQS, x, BLOCK, None, polls=polls, timers=True)
    assert got["batch"] == HALF and len(ref["pdus"]) >= 6
    want_launches = [32, 32, 5] if not polls else [32, 9, 28]
    assert got["launches"] == (len(want_launches), sum(want_launches))        # one launch per half, closed full or by the poll
    same(got, ref)


def test_a_launch_cut_by_the_output_counts(gpu, monkeypatch):
    """128 ksps: blocks of 0.224 s, 32 of them would make 38 736 samples at 5400 sps and twice that does not fit the 16-bit output counts:
    HFDL_GPU_DEMOD_BATCH=32 is cut to the 27 that fit, the geometry says so, and results are those of a launch per block."""
    fs, cf, freqs = 128000, 10_000_000, [9_979_000, 10_011_000, 10_033_000]
    bursts = burst_plan(freqs, [0.15, 0.9, 1.6], [3, 3, 3], seed=47)
    dur = 9.4
    assert max(b["t0"] for b in bursts) + T_FRAME < dur - 0.2
    x = synth.synth_wideband(fs, cf, int(dur * fs), bursts, noise_sigma=0.004, seed=49)
    x = x[:len(x) // BLOCK * BLOCK]
    nblk = len(x) // BLOCK
    assert nblk > 32
    ref = run(gpu, monkeypatch, fs, cf, freqs, x, BLOCK, 1)
    got = run(gpu, monkeypatch, fs, cf, freqs, x, BLOCK, 32, timers=True)
    assert got["batch"] == 27 and got["fold"] == HALF
    assert got["launches"] == (3, nblk)          # a half of 32: 27 + 5; then the rest
    assert len(ref["pdus"]) == len(bursts)
    same(got, ref)
