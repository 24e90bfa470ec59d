"""GPU tests of the spectrum monitor (hfdl_gpu_frontend_spectrum_enable / _read; dumphfdl_amd/csrc/spectrum_kernels.hip) against the
float64 model of tests/spectrum_f64.py.

Gates (derived, not fitted; u = 2^-24):
  stage check -- the device's own spectra (HFDL_GPU_TAP_SPECTRUM) through the float64 model against spectrum_read:
      |mean - mean64| <= (log2 G + 8) 2^-23 ref   per band,   ref = mean64 (RECT), the widened-band RECT power / 0.375 (HANN),
      peak against max_t of the float64 per-block values under the same gate.  The terms are non-negative: |X|^2 2u, a tree of depth
      log2 G at most log2 G u (bands longer than a 512-bin tile: a compensated per-thread sum, ~2u, and a tree of depth 8 -- no more),
      normalisation u, compensated accumulation ~2u, the read-back's division u.  tests/test_spectrum_cpu.py shows the arithmetic
      alone at 0.12 of this gate at most.  On top of the gate the device must equal the fp32 emulation of its summation order bit for bit
      (the kernel is compiled without FMA contraction, so every operation is an IEEE fp32 operation numpy repeats).
  end to end -- float64 np.fft of the same [history, new] window, RECT, T = 1:
      |sqrt(mean_gpu) - sqrt(mean_f64)| <= 3e-6 sqrt(sum_b mean_f64) + (log2 G + 8) 2^-23 sqrt(mean_f64)
      (the forward FFT's gate of 3e-6 relative RMS; the error inside a band is no larger than the whole).
Input: white noise at -60 dBFS, a 0 dBFS tone at bin 1000.37 above the centre, a -70 dBFS tone 3 * 64 + 5 bins further up, one HFDL
burst (hfdl_synth) on the front end's first channel."""
import numpy as np
import pytest

import hfdl_synth as synth
import spectrum_f64 as S
from dumphfdl_amd import frontend as F
from spectrum_f64 import check_against_model, u32      # (tests/test_gpu_spectrum_history.py takes them from here)

pytestmark = pytest.mark.gpu

T_READS = (1, 5, 32, 40)       # crossing a half and a 16 + 4 cut
NBLK = 40


def stream_for(fe, fs, cf, freq, seed, nblk=NBLK):
    """complex64 stream of nblk blocks for one receiver: the model's test signal + one HFDL burst on `freq`."""
    g = fe.geometry
    ns = nblk * g.input_size
    rng = np.random.default_rng(seed)
    burst = synth.synth_wideband(fs, cf, ns, [dict(freq=freq, mode=2, octets=synth.make_pdu(rng, 2), t0=0.05, amp=0.003, cfo=4.0)], noise_sigma=0.0, seed=seed)
    return S.make_signal(g.fft_size, ns, seed, burst=burst).astype(np.complex64)


def run_geometry(tag, fe, fs, centres, xs, chan_of_rx, push):
    """Stage check, end-to-end check and the operator's checks on one front end.  xs[r] = receiver r's stream of NBLK blocks;
    push(b) pushes block b of every receiver.  Every pass pushes blocks 0 .. NBLK - 1 behind block NBLK - 1, so block t of every pass has
    the same [history, new] window and the same spectrum."""
    g = fe.geometry
    N, n, ov, nrx = g.fft_size, g.input_size, g.overlap_length, len(xs)
    push(NBLK - 1)
    fe.poll_pdus()
    spec = [[None] * NBLK for _ in range(nrx)]
    for b in range(NBLK):
        push(b)
        for r in range(nrx):
            spec[r][b] = fe.read_tap(F.TAP_SPECTRUM, chan_of_rx[r])        # drains: one block per half
    fe.poll_pdus()
    for bins in (16, 256, N // 16):
        for hann in (False, True):
            G = N // bins
            fe.spectrum_enable(bins, hann=hann, maxhold=True)
            r0 = fe.spectrum_read(0)
            assert r0["blocks"] == 0 and r0["mean"] is None and r0["first_block"] == fe.counters()["blocks"]
            first = fe.counters()["blocks"]
            model = []
            for r in range(nrx):
                p64 = np.array([S.band_powers(spec[r][t], bins, hann) for t in range(NBLK)])
                ref = np.array([S.hann_ref(spec[r][t], bins) for t in range(NBLK)]) if hann else p64
                model.append((p64, ref, S.Accumulator()))
            for b in range(NBLK):
                push(b)
                for r in range(nrx):
                    model[r][2].add(S.emulate_block(spec[r][b], bins, hann))
                if b + 1 in T_READS:
                    for r in range(nrx):
                        got = fe.spectrum_read(r)
                        assert got["first_block"] == first
                        check_against_model("%s rx%d bins=%d %s" % (tag, r, bins, "HANN" if hann else "RECT"), got, model[r][0], model[r][1], model[r][2].read(), G, b + 1)
            # the spectra of this pass are those of the reference pass: the newest block's, bit for bit
            for r in range(nrx):
                assert np.array_equal(fe.read_tap(F.TAP_SPECTRUM, chan_of_rx[r]).view(np.uint32), spec[r][NBLK - 1].view(np.uint32))
            fe.poll_pdus()
    # ---- end to end against the samples, T = 1, and what an operator would check (64-bin bands)
    for r in range(nrx):
        x = xs[r].astype(np.complex128)
        w = S.windows(x[:n], N, ov, [0], history=x[(NBLK - 1) * n:])[0]
        for bins in (16, N // 64, N // 16):
            G = N // bins
            fe.spectrum_enable(bins)
            push(0)
            got = fe.spectrum_read(r)
            push(NBLK - 1)
            fe.poll_pdus()
            assert got["blocks"] == 1 and got["peak"] is None
            m64 = S.band_powers_from_samples(w, bins)
            err = np.abs(np.sqrt(got["mean"].astype(np.float64)) - np.sqrt(m64))
            lim = 3e-6 * np.sqrt(m64.sum()) + S.gate(G) * np.sqrt(m64)
            print("%s rx%d end to end bins=%d: worst error / bound %.3f" % (tag, r, bins, (err / lim).max()))
            assert (err <= lim).all(), (tag, r, bins, float((err / lim).max()))
        bins = N // 64
        lo, hi = S.band_edges(centres[r], fs, N, bins)
        f_tone, f_weak = centres[r] + S.TONE_BIN * fs / N, centres[r] + S.WEAK_BIN * fs / N
        res = {}
        # block 1 behind block 0: a window the tones run through without a seam (block 0 behind block NBLK - 1 has one, which splatters)
        w1 = S.windows(x[:2 * n], N, ov, [1])[0]
        for hann in (False, True):
            push(0)
            fe.spectrum_enable(bins, hann=hann)
            push(1)
            got = fe.spectrum_read(r)
            push(NBLK - 1)
            fe.poll_pdus()
            assert got["blocks"] == 1
            assert np.allclose(got["freqs"], (lo + hi) / 2, rtol=0, atol=1e-6)
            for name, p in (("model", S.band_powers_from_samples(w1, bins, hann)), ("device", got["mean"].astype(np.float64))):
                bt = int(np.argmax(p))
                assert lo[bt] <= f_tone < hi[bt], (name, hann, bt)              # orientation: a mirrored or I/Q-swapped axis fails
                near = p[bt - 1:bt + 2].sum() if hann else p.sum()              # HANN: the tone's band and its neighbours hold all of it; RECT: Parseval
                assert abs(near - 1.0) <= 1e-4, (name, hann, near)
                bw = int(np.searchsorted(hi, f_weak, side="right"))
                assert lo[bw] <= f_weak < hi[bw]
                res[name, hann] = 10 * np.log10(p[bw] / max(p[bw - 1], p[bw + 1]))
        print("%s rx%d: -70 dBFS tone above its louder neighbour, model RECT %.1f HANN %.1f dB, device RECT %.1f HANN %.1f dB"
              % (tag, r, res["model", False], res["model", True], res["device", False], res["device", True]))
        for name in ("model", "device"):
            assert res[name, True] >= 10.0 and res[name, False] < 10.0, (name, res)
    fe.spectrum_enable(0)


def case1_freqs(nch, cf=10_000_000):
    return [int(cf + (i - nch // 2) * 15_000 + 4_000) for i in range(nch)]


@pytest.mark.parametrize("fs,nch", [(250_000, 1), (2_400_000, 130)])
def test_band_powers_one_receiver(gpu, fs, nch):
    cf = 10_000_000
    freqs = [10_040_000] if nch == 1 else case1_freqs(nch)
    fe = gpu.Frontend(fs, cf, freqs)
    n = fe.input_size
    x = stream_for(fe, fs, cf, freqs[0], seed=100 + nch)
    run_geometry("%d x %d" % (fs, nch), fe, fs, [cf], [x], [0], lambda b: fe.push_block(x[b * n:(b + 1) * n]))
    fe.close()


def test_band_powers_three_receivers(gpu):
    """Three receivers at 2.048 Msps with different content: every receiver's accumulator against the model of ITS spectra."""
    fs = 2_048_000
    centres, nchs = [10_000_000, 11_300_000, 8_950_000], [1, 3, 2]
    freqs = [[c + 50_000 + 15_000 * i for i in range(k)] for c, k in zip(centres, nchs)]
    fe = gpu.MultiFrontend(fs, list(zip(centres, freqs)))
    n = fe.input_size
    xs = [stream_for(fe, fs, c, fr[0], seed=200 + r) for r, (c, fr) in enumerate(zip(centres, freqs))]
    chan0 = [0, 1, 4]
    run_geometry("3 x 2.048 Msps", fe, fs, centres, xs, chan0, lambda b: fe.push_blocks([x[b * n:(b + 1) * n] for x in xs]))
    fe.close()


def test_band_powers_40_msps(gpu):
    """N = 2^23: bands of 16 bins (524288 of them) and of 2^19 bins (a workgroup walks 1024 tiles), stage check and end to end."""
    fs, cf = 40_000_000, 8_000_000
    fe = gpu.Frontend(fs, cf, [8_927_000])
    g = fe.geometry
    N, n, ov = g.fft_size, g.input_size, g.overlap_length
    assert N == 1 << 23
    x = S.make_signal(N, n, seed=40).astype(np.complex64)
    fe.push_block(x)
    w = S.windows(x.astype(np.complex128), N, ov, [0], history=x)[0]
    for bins, hann in ((N // 16, False), (16, True), (4096, True), (16, False)):
        G = N // bins
        fe.spectrum_enable(bins, hann=hann, maxhold=True)
        fe.push_block(x)
        got = fe.spectrum_read(0)
        X = fe.read_tap(F.TAP_SPECTRUM)
        fe.poll_pdus()
        p64 = S.band_powers(X, bins, hann)[None]
        ref = S.hann_ref(X, bins)[None] if hann else p64
        acc = S.Accumulator()
        acc.add(S.emulate_block(X, bins, hann))
        check_against_model("40 Msps bins=%d %s" % (bins, "HANN" if hann else "RECT"), got, p64, ref, acc.read(), G, 1)
        if not hann:
            m64 = S.band_powers_from_samples(w, bins)
            err = np.abs(np.sqrt(got["mean"].astype(np.float64)) - np.sqrt(m64))
            lim = 3e-6 * np.sqrt(m64.sum()) + S.gate(G) * np.sqrt(m64)
            print("40 Msps end to end bins=%d: worst error / bound %.3f" % (bins, (err / lim).max()))
            assert (err <= lim).all()
            lo, hi = S.band_edges(cf, fs, N, bins)
            bt = int(np.argmax(got["mean"]))
            assert lo[bt] <= cf + S.TONE_BIN * fs / N < hi[bt]
    fe.close()


def traffic(fs, cf, freqs, dur, seed):
    bursts = synth.plan_traffic(freqs, dur, seed=seed, dense=True, gap_s=0.12, amp=(0.02, 0.1))
    return synth.synth_wideband(fs, cf, int(dur * fs), bursts, noise_sigma=0.012, seed=seed)


def pdu_key(p):
    return tuple((k, u32([v]).tobytes() if isinstance(v, float) else v) for k, v in sorted(p.items()))


def test_monitor_moves_nothing_else(gpu):
    """Same seeded traffic with the monitor off and on (HANN | MAXHOLD, a read after every third push): identical PDUs (every field),
    identical channelizer output of every block of the last half as uint32, identical fold launch shapes and counters."""
    fs, cf = 250_000, 10_000_000
    freqs = [9_915_000, 9_972_000, 10_026_000, 10_083_000, 10_101_000]
    x = traffic(fs, cf, freqs, 9.0, 31)

    def run(monitor):
        fe = gpu.Frontend(fs, cf, freqs)
        n, nblk = fe.input_size, len(x) // fe.input_size
        fe.reset_timers(True)
        if monitor:
            fe.spectrum_enable(256, hann=True, maxhold=True)
        reads = []
        for b in range(nblk):
            fe.push_block(x[b * n:(b + 1) * n])
            if monitor and b % 3 == 2:
                reads.append(fe.spectrum_read(0, reset=(b % 2 == 0)))
        shapes = fe.fold_launch_shapes()
        pdus = fe.poll_pdus()
        held = 0
        outs = []
        while True:
            try:
                outs.append([fe.read_tap(F.TAP_CHAN_OUT, c, back=held).view(np.uint32).copy() for c in range(len(freqs))])
            except F.GpuError:
                break
            held += 1
        cnt = fe.counters()
        fe.close()
        return sorted(pdu_key(p) for p in pdus), outs, shapes, cnt, reads

    off, on = run(False), run(True)
    assert len(off[0]) >= 5 and off[0] == on[0]
    assert len(off[1]) >= 1 and len(off[1]) == len(on[1])
    for a, b in zip(off[1], on[1]):
        assert all(np.array_equal(p, q) for p, q in zip(a, b))
    assert off[2] == on[2] and sum(off[2].values()) >= 2
    assert off[3] == on[3]
    assert len(on[4]) >= 5 and all(r["blocks"] >= 1 for r in on[4])


@pytest.mark.parametrize("what", ["poll", "fold_batch", "device", "cs16"])
def test_monitor_result_is_bit_identical_whatever_the_pipeline_does(gpu, monkeypatch, what):
    """mean and peak as uint32 across: a draining poll after every block against one per half, HFDL_GPU_FOLD_BATCH 1 against 32, host
    against device input, cs16 against the same samples as cf32 (x / 32767.5 in fp32, the reference's convert_cs16)."""
    fs, cf = 250_000, 10_000_000
    freqs = [9_915_000, 10_026_000, 10_101_000]
    x = traffic(fs, cf, freqs, 5.0, 17)
    raw = np.clip(np.round(x.view(np.float32) * 20000), -32768, 32767).astype(np.int16)
    xq = (raw.astype(np.float32) / np.float32(32767.5)).view(np.complex64)

    def run(mode):
        if mode in ("fb1", "fb32"):
            monkeypatch.setenv("HFDL_GPU_FOLD_BATCH", mode[2:])
        else:
            monkeypatch.delenv("HFDL_GPU_FOLD_BATCH", raising=False)
        fe = gpu.Frontend(fs, cf, freqs)
        n, nblk = fe.input_size, len(x) // fe.input_size
        fe.spectrum_enable(512, hann=True, maxhold=True)
        dev = None
        if mode == "device":
            import torch
            dev = torch.from_numpy(np.array(xq.view(np.float32))).cuda()
            torch.cuda.synchronize()
        for b in range(nblk):
            if mode == "device":
                fe.push_block(dev.data_ptr() + 8 * b * n)
            elif mode == "cs16":
                fe.push_block_raw(raw[2 * b * n:2 * (b + 1) * n], F.SFMT_CS16)
            else:
                fe.push_block(xq[b * n:(b + 1) * n])
            if mode == "poll_each" or (mode == "poll_half" and b % fe.geometry.fold_batch == fe.geometry.fold_batch - 1):
                fe.poll_pdus()
        got = fe.spectrum_read(0)
        fe.poll_pdus()
        fe.close()
        assert got["blocks"] == nblk and got["first_block"] == 0
        return u32(got["mean"]).copy(), u32(got["peak"]).copy()

    a, b = {"poll": ("poll_each", "poll_half"), "fold_batch": ("fb1", "fb32"), "device": ("host", "device"), "cs16": ("host", "cs16")}[what]
    ra, rb = run(a), run(b)
    assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1])
    r2 = run(a)                                   # and from run to run
    assert np.array_equal(ra[0], r2[0]) and np.array_equal(ra[1], r2[1])


def test_reset_semantics_and_receivers(gpu):
    """blocks / first_block, a per-receiver reset (the other receivers' averages go on; peak starts over too), enable -> disable ->
    enable with other bins, and receiver r of a multi-receiver front end against a front end of its own fed receiver r's samples: as
    uint32 -- the two spectra are themselves bit-identical (asserted here on the newest block, as test_gpu_multi_receiver.py does)."""
    fs = 2_048_000
    centres, nchs = [10_000_000, 11_300_000, 8_950_000], [1, 3, 2]
    freqs = [[c + 50_000 + 15_000 * i for i in range(k)] for c, k in zip(centres, nchs)]
    multi = gpu.MultiFrontend(fs, list(zip(centres, freqs)))
    singles = [gpu.Frontend(fs, c, fr) for c, fr in zip(centres, freqs)]
    n = multi.input_size
    nblk = 12
    xs = [stream_for(multi, fs, c, fr[0], seed=300 + r, nblk=nblk) for r, (c, fr) in enumerate(zip(centres, freqs))]
    # receiver r louder in block 2 than anywhere else: a peak that a reset must forget
    for x in xs:
        x[2 * n:3 * n] *= 3
    with pytest.raises(F.GpuError):
        multi.spectrum_read(0)                                     # off
    for bad in (8, 24, -16):
        with pytest.raises(F.GpuError):
            multi.spectrum_enable(bad)
    with pytest.raises(F.GpuError):
        multi.spectrum_enable(multi.geometry.fft_size // 8)
    multi.spectrum_enable(64)
    with pytest.raises(F.GpuError):
        multi.spectrum_read(3)
    multi.spectrum_enable(0)
    with pytest.raises(F.GpuError):
        multi.spectrum_read(0)
    for fe in [multi] + singles:
        fe.spectrum_enable(1024, hann=True, maxhold=True)
    for b in range(nblk):
        blk = [x[b * n:(b + 1) * n] for x in xs]
        multi.push_blocks(blk)
        for s, xb in zip(singles, blk):
            s.push_block(xb)
        if b == 4:                                                 # receiver 1 starts over after block 4; its single twin too
            for fe, rx in ((multi, 1), (singles[1], 0)):
                got = fe.spectrum_read(rx, reset=True)
                assert got["blocks"] == 5 and got["first_block"] == 0
                again = fe.spectrum_read(rx)
                assert again["blocks"] == 0 and again["first_block"] == 5
    for r, s in enumerate(singles):
        gm, gs = multi.spectrum_read(r), s.spectrum_read(0)
        want = (7, 5) if r == 1 else (12, 0)
        assert (gm["blocks"], gm["first_block"]) == want and (gs["blocks"], gs["first_block"]) == want
        chan = [0, 1, 4][r]
        assert np.array_equal(multi.read_tap(F.TAP_SPECTRUM, chan).view(np.uint32), s.read_tap(F.TAP_SPECTRUM).view(np.uint32))
        assert np.array_equal(u32(gm["mean"]), u32(gs["mean"])) and np.array_equal(u32(gm["peak"]), u32(gs["peak"]))
        assert np.array_equal(gm["freqs"], gs["freqs"])
    # the loud block 2 is in receiver 0's and 2's peak and no longer in receiver 1's
    p0, p1 = multi.spectrum_read(0), multi.spectrum_read(1)
    bt = int(np.argmax(p0["mean"]))
    assert p0["peak"][bt] > 8.0 and p1["peak"][int(np.argmax(p1["mean"]))] < 1.5
    for fe in [multi] + singles:
        fe.poll_pdus()
        fe.close()


def test_what_counts_as_a_block(gpu):
    """channelize_block is a block of the monitor, push_baseband is none: blocks / first_block after each, in the numbering of counters()."""
    fs, cf = 250_000, 10_000_000
    fe = gpu.Frontend(fs, cf, [10_040_000])
    g = fe.geometry
    n = g.input_size
    x = S.make_signal(g.fft_size, 4 * n, seed=9).astype(np.complex64)
    fe.push_block(x[:n])                                        # block 0, before the monitor is on
    fe.spectrum_enable(64, maxhold=True)
    fe.channelize_block(x[n:2 * n])                             # block 1: counted
    got = fe.spectrum_read(0)
    assert (got["blocks"], got["first_block"]) == (1, 1) and fe.counters()["blocks"] == 2
    p64 = S.band_powers(fe.read_tap(F.TAP_SPECTRUM), 64)
    assert np.abs(got["mean"] - p64).max() <= S.gate(g.fft_size // 64) * p64.max() and np.array_equal(u32(got["mean"]), u32(got["peak"]))
    fe.push_baseband([np.zeros(g.max_outputs_per_block, np.complex64)])      # no forward FFT: not a block
    again = fe.spectrum_read(0)
    assert (again["blocks"], again["first_block"]) == (1, 1) and np.array_equal(u32(again["mean"]), u32(got["mean"]))
    fe.push_block(x[2 * n:3 * n])                               # block 2
    got = fe.spectrum_read(0, reset=True)
    assert (got["blocks"], got["first_block"]) == (2, 1)
    fe.channelize_block(x[3 * n:])
    got = fe.spectrum_read(0)
    assert (got["blocks"], got["first_block"]) == (1, 3)
    fe.poll_pdus()
    fe.close()


def test_replay_writes_rtl_power_csv(gpu, tmp_path):
    """hfdl_replay --spectrum-file on a cs16 file: the CSV parses, one line per whole interval of signal, the 0 dBFS tone (here at half
    scale: -6.02 dBFS less the cs16 scaling) in the band the header's formula names at the level the float64 model gives, and the PDUs
    on stdout are those of a run without the flag."""
    import os
    import subprocess
    from test_spectrum_cpu import parse_rtl_power
    fs, cf = 250_000, 10_000_000
    freqs = [9_930_000, 10_037_000, 10_081_500]
    probe = gpu.Frontend(fs, cf, freqs)
    N, n, ov = probe.geometry.fft_size, probe.geometry.input_size, probe.geometry.overlap_length
    probe.close()
    dur, interval, bins = 6.3, 2, N // 64
    ns = int(dur * fs)
    bursts = synth.plan_traffic(freqs, dur, seed=3, dense=True)
    x = synth.synth_wideband(fs, cf, ns, bursts, noise_sigma=0.01, seed=1).astype(np.complex128)
    x += 0.5 * np.exp(2j * np.pi * (S.TONE_BIN / N) * np.arange(ns))
    raw = np.clip(np.round(x.astype(np.complex64).view(np.float32) * 20000), -32768, 32767).astype(np.int16)
    xq = (raw.astype(np.float32) / np.float32(32767.5)).view(np.complex64)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "dumphfdl_amd", "hfdl_replay")
    path = tmp_path / "iq.cs16"
    raw.tofile(path)
    csv = tmp_path / "spectrum.csv"
    base = [exe, "--iq-file", str(path), "--sample-rate", str(fs), "--sample-format", "CS16", "--centerfreq", str(cf / 1e3)]
    chans = ["%.3f" % (f / 1e3) for f in freqs]
    plain = subprocess.run(base + chans, capture_output=True, text=True, timeout=300)
    mon = subprocess.run(base + ["--spectrum-file", str(csv), "--spectrum-bins", str(bins), "--spectrum-interval", str(interval), "--spectrum-hann"] + chans,
                         capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and mon.returncode == 0, mon.stderr

    def pdus(out):        # every field but the wall-clock timestamp
        return sorted(" ".join(t for t in l.split() if not t.startswith("ts=")) for l in out.splitlines() if l.startswith("PDU "))
    assert len(pdus(plain.stdout)) >= len(bursts) - 1 and pdus(plain.stdout) == pdus(mon.stdout)
    lines = [parse_rtl_power(l) for l in open(csv).read().splitlines()]
    assert len(lines) == int(dur // interval) == 3
    lo, hi = S.band_edges(cf, fs, N, bins)
    per = [-(-(k + 1) * interval * fs // n) for k in range(len(lines))]       # blocks pushed when interval k closes
    first = 0
    for k, p in enumerate(lines):
        T = per[k] - first
        assert p["samples"] == T and len(p["db"]) == bins
        assert abs(p["low"] - lo[0]) <= 0.5 and abs(p["high"] - hi[-1]) <= 0.5 and abs(p["step"] - (hi[0] - lo[0])) <= 0.005
        want = np.mean([S.band_powers_from_samples(w, bins, True) for w in S.windows(xq, N, ov, range(first, per[k]))], axis=0)
        bt = int(np.argmax(p["db"]))
        assert lo[bt] <= cf + S.TONE_BIN * fs / N < hi[bt] and bt == int(np.argmax(want))
        # per band: half a unit of the second decimal from the formatter, plus the end-to-end bound of this file's docstring on the
        # amplitude -- the forward FFT's 3e-6 of the whole spectrum's RMS, through the three Hann taps (weights of absolute sum 1) and
        # the division by sqrt(0.375), and the monitor's own gate -- turned into dB
        amp_tol = 3e-6 / np.sqrt(0.375) * np.sqrt(np.mean(np.abs(xq) ** 2)) + S.gate(64) * np.sqrt(want / 0.375)
        db_tol = 0.005 + 1e-9 + 20 * np.log10(1 + amp_tol / np.sqrt(want))
        err = np.abs(p["db"] - 10 * np.log10(want))
        print("interval %d: worst dB error / bound %.3f (worst bound %.4f dB)" % (k, (err / db_tol).max(), db_tol.max()))
        assert (err <= db_tol).all()
        level = (0.5 * 20000 / 32767.5) ** 2                                 # the tone as the cs16 file holds it, -10.31 dBFS
        got3 = (10 ** (p["db"][bt - 1:bt + 2] / 10)).sum()
        assert abs(got3 - level) <= level * (1e-4 + 10 ** 0.0005 - 1), (got3, level)      # 1e-4 as on the C ABI + the CSV's second decimal
        first = per[k]
