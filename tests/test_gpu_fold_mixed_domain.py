"""GPU tests: the fold in the mixed FFT domain (csrc/fold_domain.h) against the fold on spectra.

With HFDL_GPU_FOLD_SPECTRUM=0, where the geometry allows it, the forward FFT stops after its second pass and the fold contracts over
that pass's rows; with 1 (the default) a front end runs all three passes and folds spectra, as every front end did before.  Both are built on the
same blocks here.  The stage taps must read the same words either way (the spectrum and the filter are made on demand, by the pass 3
the pipeline left out; the NCO phasor table by two rider segments instead of three), the channelizer output of both is held to the
float64 direct-form model under the gate of tests/test_gpu_channelizer_f64.py, and everything a launch shape, the spectrum monitor
or a retune could change is compared word for word.

The geometry is the smallest that takes the register-resident passes and meets the predicate: 1.4 Msps, N = 2^18 split 6 / 6 / 6,
M = 2048 -- five bits of k2 inside a bin (the generalised group index), one bit of k2hi in the row -- 128 rows, three channels (one
octet with five padding slots; 2 MiB of taps per channel).  The geometry comes from the planner and the predicate is asserted."""
import numpy as np
import pytest

import ddc_f64 as M
import hfdl_synth as synth
import test_gpu_channelizer_f64 as CH
from dumphfdl_amd import frontend as F

pytestmark = pytest.mark.gpu

FS, CF = 1_400_000, 10_000_000
FREQS = [9_583_000, 10_012_000, 10_655_000]


def make(gpu, monkeypatch, spectrum_domain, fold_batch=None, freqs=FREQS):
    """A front end folding in the mixed domain (HFDL_GPU_FOLD_SPECTRUM=0) or on spectra (1: the default)."""
    monkeypatch.setenv("HFDL_GPU_FOLD_SPECTRUM", "1" if spectrum_domain else "0")
    if fold_batch:
        monkeypatch.setenv("HFDL_GPU_FOLD_BATCH", str(fold_batch))
    else:
        monkeypatch.delenv("HFDL_GPU_FOLD_BATCH", raising=False)
    fe = gpu.Frontend(FS, CF, list(freqs))
    g = fe.geometry
    logn, logm = g.fft_size.bit_length() - 1, g.fft_inv_size.bit_length() - 1
    l1 = (logn + 2) // 3
    l2 = (logn - l1 + 1) // 2
    l3 = logn - l1 - l2
    # the planner's split (frontend_create.cpp HostFftPlan::build) and the predicate (fold_domain.h mixed_fold_fits)
    assert (g.fft_size, g.fft_inv_size, g.pre_decimation) == (1 << 18, 2048, 128) and (l1, l2, l3) == (6, 6, 6)
    assert all(6 <= l <= 8 for l in (l1, l2, l3)) and logm - l1 >= 4 and logm <= l1 + l2
    return fe


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def noise(nsamples, seed, level=0.05):
    rng = np.random.default_rng(seed)
    x = np.empty(nsamples, np.complex64)
    x.real = rng.standard_normal(nsamples, dtype=np.float32)
    x.imag = rng.standard_normal(nsamples, dtype=np.float32)
    return x * np.float32(level)


def run_both(gpu, monkeypatch, x, nblk, fold_batch=32):
    """The same blocks through both front ends, one half closed by a sync: per path the taps of every block."""
    out = {}
    for name, spec in (("mixed", False), ("spectrum", True)):
        fe = make(gpu, monkeypatch, spec, fold_batch)
        n = fe.input_size
        for b in range(nblk):
            fe.push_block(x[b * n:(b + 1) * n])
        fe.sync()
        out[name] = dict(
            spectrum=[fe.read_tap(F.TAP_SPECTRUM, 0, back=nblk - 1 - b) for b in range(nblk)],
            filter=[fe.read_tap(F.TAP_FILTER, c) for c in range(len(FREQS))],
            phasors=[[fe.read_tap(F.TAP_NCO_PHASORS, c, back=nblk - 1 - b) for c in range(len(FREQS))] for b in range(nblk)],
            chan=[[fe.read_tap(F.TAP_CHAN_OUT, c, back=nblk - 1 - b) for c in range(len(FREQS))] for b in range(nblk)])
        fe.close()
    return out


def against_model(tag, oracle, x, got, nblk):
    dev = {b: {c: (got["chan"][b][c], got["phasors"][b][c]) for c in range(len(FREQS))} for b in range(nblk)}
    return CH.compare(tag, oracle, FS, CF, FREQS, x, dev, CH.FLOOR.get(FS, CH.FLOOR_ANY))


def test_taps_equal_and_both_paths_under_the_float64_gate(gpu, oracle, monkeypatch):
    """Five blocks of the channelizer tests' signal (in-band tones, a tone 60 dB up on an alias of every channel centre, wide-band noise
    60 dB up outside the pass bands, a tone on the pass-band edge) in one fold launch.  HFDL_GPU_TAP_SPECTRUM of every block,
    HFDL_GPU_TAP_FILTER of every channel and HFDL_GPU_TAP_NCO_PHASORS of every (block, channel): equal as uint32.  HFDL_GPU_TAP_CHAN_OUT
    of BOTH paths against the float64 direct-form model: e_gpu <= 4 max(e_ora, floor), the gate of tests/test_gpu_channelizer_f64.py
    for a geometry outside its table (FLOOR_ANY); compare() prints both sides' errors."""
    nblk = 5
    dec = oracle.lib().orc_compute_fft_decimation_rate(FS, 5400)
    n = F.plan_geometry(dec, 250 / FS).input_size
    x = M.make_signal(FS, CF, FREQS, FREQS, nblk * n, 77, dec, 128)
    r = run_both(gpu, monkeypatch, x, nblk)
    for b in range(nblk):
        assert (words(r["mixed"]["spectrum"][b]) == words(r["spectrum"]["spectrum"][b])).all(), "spectrum tap, block %d" % b
        for c in range(len(FREQS)):
            assert (words(r["mixed"]["phasors"][b][c]) == words(r["spectrum"]["phasors"][b][c])).all(), "phasor table, block %d channel %d" % (b, c)
    for c in range(len(FREQS)):
        assert (words(r["mixed"]["filter"][c]) == words(r["spectrum"]["filter"][c])).all(), "filter tap, channel %d" % c
        assert np.abs(r["mixed"]["filter"][c]).max() > 0.5            # (a pass band of gain ~1: the tap is not empty)
    against_model("mixed domain, fs %d" % FS, oracle, x, r["mixed"], nblk)
    against_model("spectrum domain, fs %d" % FS, oracle, x, r["spectrum"], nblk)


def test_a_block_scaled_by_2_to_the_minus_100(gpu, oracle, monkeypatch):
    """Block 0 of the same kind of signal times 2^-100 (exact in fp32), blocks 1 and 2 as they are: in the mixed domain the taps carry the
    factor R3 and the block's transform is one pass shorter, so what underflows differs from the spectrum-domain fold's.  Both paths
    against the float64 model, per (block, channel) relative to that block's own level -- the tiny block under the same gate as the
    others: the stop-band products that go subnormal are far below an ulp of its sums.  (Block 1's overlap history is the tiny block's
    tail: the model is fed the same samples.)"""
    nblk = 3
    dec = oracle.lib().orc_compute_fft_decimation_rate(FS, 5400)
    n = F.plan_geometry(dec, 250 / FS).input_size
    x = M.make_signal(FS, CF, FREQS, FREQS, nblk * n, 78, dec, 128)
    x[:n] *= np.float32(2.0 ** -100)
    r = run_both(gpu, monkeypatch, x, nblk)
    assert 0 < np.abs(r["mixed"]["chan"][0][0]).max() < 2.0 ** -90
    against_model("mixed domain, block 0 x 2^-100", oracle, x, r["mixed"], nblk)
    against_model("spectrum domain, block 0 x 2^-100", oracle, x, r["spectrum"], nblk)


def test_block_counts_per_launch_change_nothing(gpu, monkeypatch):
    """The property of test_fold_batching_changes_nothing on the new path: halves of 1, 4, 5, 16, 17 (16 + 1) and 32 blocks of one stream,
    each closed by a sync -- the four-, sixteen- and thirty-two-column forms reading pass 2's output -- give, per block and channel, the
    words of a fold launch per block (HFDL_GPU_FOLD_BATCH=1)."""
    counts = [1, 4, 5, 16, 17, 32]
    total = sum(counts)
    fe = make(gpu, monkeypatch, False, 1)
    n = fe.input_size
    x = noise(total * n, 3)
    ref = []
    for b in range(total):
        fe.push_block(x[b * n:(b + 1) * n])
        fe.sync()
        ref.append([words(fe.read_tap(F.TAP_CHAN_OUT, c)).copy() for c in range(len(FREQS))])
    fe.close()
    fe = make(gpu, monkeypatch, False, 32)
    fe.reset_timers(True)
    b = 0
    for k in counts:
        for j in range(k):
            fe.push_block(x[(b + j) * n:(b + j + 1) * n])
        fe.sync()
        for j in range(k):
            for c in range(len(FREQS)):
                assert (words(fe.read_tap(F.TAP_CHAN_OUT, c, back=k - 1 - j)) == ref[b + j][c]).all(), (k, j, c)
        b += k
    shapes = fe.fold_launch_shapes()
    fe.close()
    assert shapes == {1: 2, 4: 1, 5: 1, 16: 2, 32: 1}, shapes


def test_a_short_burst_scenario_decodes_alike(gpu, monkeypatch):
    """Two bursts in 3.2 s of noise: the (freq, sample_index, mode, octets) lists of both paths are equal, and every PDU sent is there."""
    rng = np.random.default_rng(9)
    bursts = [dict(freq=FREQS[0], mode=1, octets=synth.make_pdu(rng, 1), t0=0.12, amp=0.1, cfo=5.0),
              dict(freq=FREQS[2], mode=3, octets=synth.make_pdu(rng, 3), t0=0.2, amp=0.07, cfo=-8.0)]
    x = synth.synth_wideband(FS, CF, int(3.2 * FS), bursts, noise_sigma=0.004, seed=6)
    got = {}
    for name, spec in (("mixed", False), ("spectrum", True)):
        fe = make(gpu, monkeypatch, spec)
        n = fe.input_size
        for b in range(len(x) // n):
            fe.push_block(x[b * n:(b + 1) * n])
        got[name] = sorted((p["freq"], p["sample_index"], p["mode"], p["octets"]) for p in fe.poll_pdus())
        fe.close()
    assert got["mixed"] == got["spectrum"]
    sent = sorted((b["freq"], b["octets"]) for b in bursts)
    assert sorted((f, o[:len(s[1])]) for (f, _, _, o), s in zip(got["mixed"], sent)) == sent


def test_the_spectrum_monitor_reads_the_same_band_powers(gpu, monkeypatch):
    """Monitor on: pass 2 stores in place as well and pass 3 runs into the monitor's scratch -- mean and peak of 256 bands over six
    blocks equal the spectrum-domain front end's as uint32, and so does the channelizer output beside it."""
    nblk = 6
    res = {}
    for name, spec in (("mixed", False), ("spectrum", True)):
        fe = make(gpu, monkeypatch, spec, 32)
        n = fe.input_size
        x = noise(nblk * n, 4)
        x += (0.2 * np.exp(2j * np.pi * 0.1234 * np.arange(len(x)))).astype(np.complex64)
        fe.spectrum_enable(256, hann=True, maxhold=True)
        for b in range(nblk):
            fe.push_block(x[b * n:(b + 1) * n])
        s = fe.spectrum_read()
        fe.sync()
        res[name] = (s, [words(fe.read_tap(F.TAP_CHAN_OUT, c, back=0)).copy() for c in range(len(FREQS))], words(fe.read_tap(F.TAP_SPECTRUM, 0)).copy())
        fe.close()
    a, b = res["mixed"], res["spectrum"]
    assert a[0]["blocks"] == b[0]["blocks"] == nblk
    assert (words(a[0]["mean"]) == words(b[0]["mean"])).all() and (words(a[0]["peak"]) == words(b[0]["peak"])).all()
    assert a[0]["peak"].max() > 0.01
    assert (a[2] == b[2]).all()
    # the fold's operand is the same with the monitor on or off: the output of the monitored mixed front end equals an unmonitored one's
    fe = make(gpu, monkeypatch, False, 32)
    n = fe.input_size
    for blk in range(nblk):
        fe.push_block(x[blk * n:(blk + 1) * n])
    fe.sync()
    for c in range(len(FREQS)):
        assert (words(fe.read_tap(F.TAP_CHAN_OUT, c)) == a[1][c]).all()
    fe.close()


def test_a_retuned_channels_filter_equals_the_spectrum_domain_one(gpu, monkeypatch):
    """Channel 1 retuned between two blocks: HFDL_GPU_TAP_FILTER of every channel afterwards -- the retuned channel's taps packed by the
    retune, the others untouched -- equals the spectrum-domain front end's as uint32, and differs from what it was."""
    new = 10_250_000
    res = {}
    for name, spec in (("mixed", False), ("spectrum", True)):
        fe = make(gpu, monkeypatch, spec)
        n = fe.input_size
        x = noise(2 * n, 5)
        fe.push_block(x[:n])
        before = words(fe.read_tap(F.TAP_FILTER, 1)).copy()
        fe.retune(1, new)
        fe.push_block(x[n:])
        fe.sync()
        res[name] = [words(fe.read_tap(F.TAP_FILTER, c)).copy() for c in range(len(FREQS))] + [words(fe.read_tap(F.TAP_CHAN_OUT, 1)).copy()]
        assert (res[name][1] != before).any()
        fe.close()
    for c in range(len(FREQS)):
        assert (res["mixed"][c] == res["spectrum"][c]).all(), c
    # and a front end created on the new frequency holds the same taps
    fe = make(gpu, monkeypatch, False, freqs=[FREQS[0], new, FREQS[2]])
    assert (words(fe.read_tap(F.TAP_FILTER, 1)) == res["mixed"][1]).all()
    fe.close()
