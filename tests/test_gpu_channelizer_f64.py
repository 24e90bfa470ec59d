"""GPU tests: the device channelizer against the float64 direct-form model (tests/ddc_f64.py) in every fold form.

One gate everywhere, calibrated by the oracle on the same input so that no tolerance is invented: per (block, channel)
e_gpu = error of the device chan_out against the model, e_ora = error of the oracle's chan_out against the same model, both as
relative RMS and as worst element / RMS of the model output, and

    e_gpu <= 4 * max(e_ora, floor)

with floor = the oracle-against-model figures of oracle/PINNING.md for the geometry.  Device and oracle are two fp32 evaluations of
the same sums with different FFT factorisations and summation orders; a wrong alias row, bin, scrap index or block column is orders
of magnitude outside a factor of 4.  For e_gpu the model runs with the device's own NCO phasor tables (tap 9: the fp32 phasor recurrence's drift is not the
fold's; the tables themselves are bounded against the float64 phase); e_ora, the calibrating side, uses the float64 phase.  The
device is never compared with itself."""
import numpy as np
import pytest

import ddc_f64 as M
from dumphfdl_amd import frontend as F

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-4
# oracle against model as measured on the CPU (oracle/PINNING.md, tests/test_channelizer_f64_cpu.py): (relative RMS, worst / RMS)
FLOOR = {250_000: (6.3e-5, 1.6e-4), 2_400_000: (3.6e-5, 1.3e-4)}
FLOOR_ANY = (6.3e-5, 1.6e-4)          # the worst over the five rates measured: geometries outside that table


def read_blocks(fe, held, first_block, channels, dev):
    """chan_out (tap 3) and NCO phasors (tap 9) of the `held` newest blocks, which are stream blocks first_block .. first_block + held - 1."""
    with pytest.raises(F.GpuError):
        fe.read_tap(F.TAP_CHAN_OUT, channels[0], back=held)                 # exactly `held` blocks are in the newest half
    for j in range(held):
        back = held - 1 - j
        dev[first_block + j] = {c: (fe.read_tap(F.TAP_CHAN_OUT, c, back=back), fe.read_tap(F.TAP_NCO_PHASORS, c, back=back)) for c in channels}


def compare(tag, oracle, fs, cf, freqs, x, dev, floor, gate=True, rms_tol=None):
    """dev: {block: {index into freqs: (chan_out, phasors)}} of one receiver's stream x.  Returns the worst (e_gpu, e_ora, ratio) pairs."""
    plans = [M.channel_plan(oracle, fs, cf, f) for f in freqs]
    st = M.Stream(x, plans[0][0])
    H = [M.taps_spectrum(t, st.L) for _, t in plans]
    ora = oracle.Frontend(fs, cf, freqs)
    n = st.input_size
    bad, worst = [], dict(gpu=[0.0, 0.0], ora=[0.0, 0.0], ratio=[0.0, 0.0], ph=0.0)
    for b in range(max(dev) + 1):
        ora.push_block(x[b * n:(b + 1) * n])
        if b not in dev:
            continue
        for c, (plan, taps) in enumerate(plans):
            got, ph = dev[b][c]
            want_o = ora.channel_view(c)["chan_out"]
            assert len(got) == len(want_o) == len(ph)
            model = M.ddc_reference(st, taps, plan, nco_phasors=[ph], blocks=[b], fast=True, taps_fft=H[c])[0]
            # the table against the float64 phase: fp32 start phase (<= 2 ulp(pi) a block) + a recurrence of len(ph) steps of <= 4 roundings
            K = b * len(ph) + np.arange(len(ph))
            assert plan.post_input_size % plan.post_decimation == 0
            dph = float(np.abs(ph.astype(np.complex128) - np.exp(1j * M.nco_phase(plan, K))).max())
            worst["ph"] = max(worst["ph"], dph)
            assert dph <= (4 * len(ph) + 4 * (b + 1)) * 2.0 ** -23, (tag, b, c, dph)
            # the calibrating side holds nothing from the device: the oracle against the model with the float64 phase (the same
            # convolution; only the phasor factor exchanged)
            model_f64 = model / ph.astype(np.complex128) * np.exp(1j * M.nco_phase(plan, K))
            eg, eo = M.errors(got, model), M.errors(want_o, model_f64)
            for i in range(2):
                lim = rms_tol if (rms_tol is not None and i == 0) else 4 * max(eo[i], floor[i])
                ratio = eg[i] / max(eo[i], floor[i])
                worst["gpu"][i] = max(worst["gpu"][i], eg[i]); worst["ora"][i] = max(worst["ora"][i], eo[i]); worst["ratio"][i] = max(worst["ratio"][i], ratio)
                if (gate or (rms_tol is not None and i == 0)) and not eg[i] <= lim:
                    bad.append((b, c, "rms" if i == 0 else "max", eg[i], eo[i]))
        st.forget(b)
    ora.close()
    print("%s: e_gpu rms %.3g max %.3g | e_ora rms %.3g max %.3g | worst e_gpu / max(e_ora, floor) rms %.2f max %.2f | phasors off the float64 phase by <= %.2g"
          % (tag, worst["gpu"][0], worst["gpu"][1], worst["ora"][0], worst["ora"][1], worst["ratio"][0], worst["ratio"][1], worst["ph"]))
    assert not bad, (tag, len(bad), bad[:8])
    return worst


def spread(nch, k=12):
    """Channels of the first octet, the last octet, the last channel and the middle: <= k of them."""
    pick = [0, 1, 7, 8, nch // 2 - 1, nch // 2, 63 if nch > 64 else nch // 3, 64 if nch > 65 else 2 * nch // 3, nch - 10, nch - 8, nch - 3, nch - 2, nch - 1]
    return sorted(set(c for c in pick if 0 <= c < nch))[:k]


def case1_freqs(fs, nch, cf=10_000_000):
    if nch == 5:
        return [9_915_000, 9_972_000, 10_026_000, 10_083_000, 10_101_000]
    return [int(cf + (i - nch // 2) * 15_000 + 4_000) for i in range(nch)]


@pytest.mark.parametrize("fs,nch", [(250_000, 5), (2_400_000, 130)])
def test_every_fold_form_against_the_float64_model(gpu, oracle, monkeypatch, fs, nch):
    """Halves of 1, 4, 5, 16, 17 (16 + 1), 20 (16 + 4), 21 and 32 blocks of one continuous stream (in-band tones, noise, a tone 60 dB up
    on an alias of the channel centre, wide-band noise 60 dB up in every alias row outside the pass band, a tone on the pass-band edge), pushed
    without polling and closed by a sync: the four-, sixteen- and thirty-two-column forms each against the model, every block of every
    half.  130 channels at 2.4 Msps: full 64-channel workgroups, left-over octets, six padding slots; the first half after a sync
    closes at 16 blocks there, so the halves above 16 are preceded by 16 blocks that are not read.  Both geometries fold on the
    matrix pipe (rows per slice a multiple of 4: asserted), the plain-VALU fall-back is not what is covered here."""
    cf = 10_000_000
    freqs = case1_freqs(fs, nch)
    watch = spread(nch)
    counts = [1, 4, 5, 16, 17, 20, 21, 32]
    monkeypatch.setenv("HFDL_GPU_FOLD_BATCH", "32")
    fe = gpu.Frontend(fs, cf, freqs)
    g = fe.geometry
    assert g.fold_batch == 32
    rows = g.pre_decimation // g.fold_slices
    assert rows >= 4 and rows % 4 == 0, "plain-VALU fold on this geometry: the matrix forms are not covered"
    fold_bound = nch >= 128
    total = sum(counts) + (16 * sum(1 for k in counts if k > 16) if fold_bound else 0)
    dec = oracle.lib().orc_compute_fft_decimation_rate(fs, 5400)
    strong = [freqs[c] for c in watch]
    n = fe.input_size
    x = M.make_signal(fs, cf, freqs, strong, total * n, 100 + nch, dec, g.pre_decimation)
    fe.reset_timers(True)
    dev, b = {}, 0
    for k in counts:
        pre = 16 if (fold_bound and k > 16) else 0
        for j in range(pre + k):
            fe.push_block(x[(b + j) * n:(b + j + 1) * n])
        fe.sync()
        read_blocks(fe, k, b + pre, watch, dev)
        b += pre + k
    shapes = fe.fold_launch_shapes()
    fe.close()
    want = {1: 2, 4: 2, 5: 1, 16: 3 + (4 if fold_bound else 0), 21: 1, 32: 1}
    print("fold launches by block count:", shapes)
    assert shapes == want, (shapes, want)
    dev = {blk: {i: v[c] for i, c in enumerate(watch)} for blk, v in dev.items()}
    compare("fs %d x %d channels, %d blocks" % (fs, nch, len(dev)), oracle, fs, cf, [freqs[c] for c in watch], x, dev, FLOOR[fs])


def test_three_receivers_against_the_float64_model(gpu, oracle, monkeypatch):
    """Receivers of 70, 5 and 66 channels at 2.048 Msps with inputs of their own, 32 blocks in one half (16 that are not read first:
    141 channels bound the block by the fold): every receiver's sampled channels against the model built from ITS centre and stream."""
    fs = 2_048_000
    centres, nchs = [10_000_000, 11_500_000, 8_700_000], [70, 5, 66]
    recv = [(cf, [int(cf + (i - k // 2) * 14_000 + 3_000) for i in range(k)]) for cf, k in zip(centres, nchs)]
    monkeypatch.setenv("HFDL_GPU_FOLD_BATCH", "32")
    fe = gpu.MultiFrontend(fs, recv)
    g = fe.geometry
    assert g.fold_batch == 32 and g.channels == 141
    n = fe.input_size
    dec = oracle.lib().orc_compute_fft_decimation_rate(fs, 5400)
    local = [spread(k, 5) for k in nchs]
    xs = [M.make_signal(fs, cf, fr, [fr[c] for c in loc], 48 * n, 200 + r, dec, g.pre_decimation) for r, ((cf, fr), loc) in enumerate(zip(recv, local))]
    fe.reset_timers(True)
    for b in range(48):
        fe.push_blocks([x[b * n:(b + 1) * n] for x in xs])
    fe.sync()
    base = np.concatenate([[0], np.cumsum(nchs)])
    glob = [int(base[r]) + c for r, loc in enumerate(local) for c in loc]
    dev = {}
    read_blocks(fe, 32, 16, glob, dev)
    shapes = fe.fold_launch_shapes()
    fe.close()
    assert shapes == {16: 1, 32: 1}, shapes
    for r, ((cf, fr), loc) in enumerate(zip(recv, local)):
        d = {blk: {i: v[int(base[r]) + c] for i, c in enumerate(loc)} for blk, v in dev.items()}
        compare("receiver %d (%d channels) of 3, fs %d" % (r, nchs[r], fs), oracle, fs, cf, [fr[c] for c in loc], xs[r], d, FLOOR_ANY)


def test_40_msps_against_the_float64_model(gpu, oracle):
    """N = 2^23, M = 4096, 2048 alias rows, two channels, eight blocks (one half closed by a sync); the float64 convolution of a block
    runs through a 2^24-point numpy transform."""
    fs, cf = 40_000_000, 8_000_000
    freqs = [cf - 1_000_000 - 1440, cf + 17_654_321]
    fe = gpu.Frontend(fs, cf, freqs)
    g = fe.geometry
    assert (g.fft_size, g.fft_inv_size, g.pre_decimation) == (1 << 23, 4096, 2048)
    n = fe.input_size
    dec = oracle.lib().orc_compute_fft_decimation_rate(fs, 5400)
    x = M.make_signal(fs, cf, freqs, freqs, 8 * n, 40, dec, g.pre_decimation, chunk=1 << 21)
    for b in range(8):
        fe.push_block(x[b * n:(b + 1) * n])
    fe.sync()
    dev = {}
    read_blocks(fe, 8, 0, [0, 1], dev)
    fe.close()
    compare("fs 40 Msps x 2 channels", oracle, fs, cf, freqs, x, dev, FLOOR_ANY)


def test_80_msps_against_the_float64_model_and_the_oracle(gpu, oracle):
    """N = 2^24 end to end: two channels, two blocks against the model and the oracle; the filter taps (written by the radix-16 pass
    in matrix-operand order) and the spectrum against the oracle's with the worst-element gate of the forward-FFT tests,
    max |err| <= 10 x (the RMS gate) x rms(want)."""
    fs, cf = 80_000_000, 40_000_000
    freqs = [cf - 21_000_000 - 1440, cf + 33_456_789]
    fe = gpu.Frontend(fs, cf, freqs)
    g = fe.geometry
    assert (g.fft_size, g.fft_inv_size) == (1 << 24, 4096)
    for c, f in enumerate(freqs):
        och = oracle.Channel(fs, cf, f)
        want = och.taps_fft().astype(np.complex128)
        och.close()
        err = np.abs(fe.read_tap(F.TAP_FILTER, c).astype(np.complex128) - want)
        rms = np.sqrt(np.mean(np.abs(want) ** 2))
        print("80 Msps filter %d: rel rms %.3g worst/rms %.3g" % (c, np.sqrt(np.mean(err ** 2)) / rms, err.max() / rms))
        assert np.sqrt(np.mean(err ** 2)) < 1e-5 * rms and err.max() <= 10 * 1e-5 * rms
        del want, err
    n = fe.input_size
    dec = oracle.lib().orc_compute_fft_decimation_rate(fs, 5400)
    x = M.make_signal(fs, cf, freqs, freqs, 2 * n, 80, dec, g.pre_decimation, chunk=1 << 21)
    for b in range(2):
        fe.push_block(x[b * n:(b + 1) * n])
    fe.sync()
    dev = {}
    read_blocks(fe, 2, 0, [0, 1], dev)
    # the spectrum on two further blocks of plain Gaussian noise (history and block): the worst-element gate presumes rounding error
    # spread evenly over the outputs, which a spectrum with full-scale tones in a few bins is not
    rng = np.random.default_rng(81)
    ora = oracle.Frontend(fs, cf, freqs[:1])
    for b in range(2):
        z = (rng.standard_normal(n, dtype=np.float32) + 1j * rng.standard_normal(n, dtype=np.float32)).astype(np.complex64)
        fe.push_block(z)
        ora.push_block(z)
    fe.sync()
    want = ora.spectrum().astype(np.complex128)
    ora.close()
    err = np.abs(fe.read_tap(F.TAP_SPECTRUM).astype(np.complex128) - want)
    rms = np.sqrt(np.mean(np.abs(want) ** 2))
    print("80 Msps spectrum: rel rms %.3g worst/rms %.3g" % (np.sqrt(np.mean(err ** 2)) / rms, err.max() / rms))
    assert np.sqrt(np.mean(err ** 2)) < 5e-6 * rms and err.max() <= 10 * 5e-6 * rms
    del want, err
    fe.close()
    compare("fs 80 Msps x 2 channels", oracle, fs, cf, freqs, x, dev, FLOOR_ANY)


def test_pruned_fold_against_the_float64_model(gpu, oracle, monkeypatch):
    """HFDL_GPU_FOLD_PRUNE=3e-7 (opt-in, documented as not the reference's sum): the same comparison reported, gated only at the
    relative RMS of 1e-4 the channelizer tests use."""
    fs, cf, nch = 2_400_000, 10_000_000, 130
    freqs = case1_freqs(fs, nch)
    watch = spread(nch, 6)
    monkeypatch.setenv("HFDL_GPU_FOLD_PRUNE", "3e-7")
    fe = gpu.Frontend(fs, cf, freqs)
    g = fe.geometry
    assert 0 < g.fold_rows < g.pre_decimation
    n = fe.input_size
    dec = oracle.lib().orc_compute_fft_decimation_rate(fs, 5400)
    x = M.make_signal(fs, cf, freqs, [freqs[c] for c in watch], 8 * n, 300, dec, g.pre_decimation)
    for b in range(8):
        fe.push_block(x[b * n:(b + 1) * n])
    fe.sync()
    dev = {}
    read_blocks(fe, 8, 0, watch, dev)
    fe.close()
    dev = {blk: {i: v[c] for i, c in enumerate(watch)} for blk, v in dev.items()}
    compare("pruned fold (%d of %d rows)" % (g.fold_rows, g.pre_decimation), oracle, fs, cf, [freqs[c] for c in watch], x, dev, FLOOR[fs], gate=False, rms_tol=RMS_TOL)


def test_subnormal_range_against_the_float64_model(gpu, oracle, monkeypatch):
    """Low-level input (a receiver with the antenna off): noise and tones scaled by 2^-100, 2^-115 and 2^-122 so that fold products,
    partial sums and finally the outputs themselves pass below the fp32 minimum normal.  Absolute error against the model in units
    of the minimum normal u = 2^-126, device and oracle alike: e_gpu <= 4 max(e_ora, floor), floor = the relative floor times the
    model's RMS + 2^-20 u (sixteen roundings of half an ulp 2^-23 u on the subnormal grid).  "Both flushed to zero" cannot pass
    unseen: the share of non-zero outputs is printed, and the device's and the oracle's may differ by no more than the share of
    model outputs smaller than the allowed error (those may round either way)."""
    fs, cf = 250_000, 10_000_000
    freqs = case1_freqs(fs, 5)
    u = 2.0 ** -126
    monkeypatch.setenv("HFDL_GPU_FOLD_BATCH", "32")
    fe = gpu.Frontend(fs, cf, freqs)
    g = fe.geometry
    n = fe.input_size
    dec = oracle.lib().orc_compute_fft_decimation_rate(fs, 5400)
    base = M.make_signal(fs, cf, freqs, freqs, 21 * n, 500, dec, g.pre_decimation, level=0.1 / 1000)          # the strong tone at 0.1
    scales = [2.0 ** -100] * 7 + [2.0 ** -115] * 7 + [2.0 ** -122] * 7
    x = np.concatenate([base[b * n:(b + 1) * n] * np.float32(sc) for b, sc in enumerate(scales)])
    assert np.isfinite(x.view(np.float32)).all()
    fe.reset_timers(True)
    for b in range(21):
        fe.push_block(x[b * n:(b + 1) * n])
    fe.sync()
    assert fe.fold_launch_shapes() == {21: 1}
    stats = fe.all_channel_stats()
    assert all(np.isfinite(v) for st in stats for v in st.values()), stats          # no preamble in this input: the demodulator's state stays finite
    got = {b: [fe.read_tap(F.TAP_CHAN_OUT, c, back=20 - b) for c in range(5)] for b in range(21)}
    ph = {b: [fe.read_tap(F.TAP_NCO_PHASORS, c, back=20 - b) for c in range(5)] for b in range(21)}
    fe.close()
    plans = [M.channel_plan(oracle, fs, cf, f) for f in freqs]
    ora = oracle.Frontend(fs, cf, freqs)
    st = M.Stream(x, plans[0][0])
    bad = []
    for b in range(21):
        ora.push_block(x[b * n:(b + 1) * n])
        for c, (plan, taps) in enumerate(plans):
            model = M.ddc_reference(st, taps, plan, nco_phasors=[ph[b][c]], blocks=[b])[0]
            want_o = ora.channel_view(c)["chan_out"]
            rms = float(np.sqrt(np.mean(np.abs(model) ** 2)))
            eg = np.abs(got[b][c].astype(np.complex128) - model) / u
            eo = np.abs(want_o.astype(np.complex128) - model) / u
            floor = (FLOOR[fs][0] * rms / u + 2.0 ** -20, FLOOR[fs][1] * rms / u + 2.0 ** -20)
            e_g, e_o = (float(np.sqrt(np.mean(eg ** 2))), float(eg.max())), (float(np.sqrt(np.mean(eo ** 2))), float(eo.max()))
            lim = [4 * max(e_o[i], floor[i]) for i in range(2)]
            nz_g, nz_o = float(np.mean(got[b][c] != 0)), float(np.mean(want_o != 0))
            either = float(np.mean(np.abs(model) / u <= lim[1]))
            if c in (0, 4):
                print("block %2d (x %.0e) ch %d: model rms %.3g u | e_gpu rms %.3g max %.3g u | e_ora rms %.3g max %.3g u | non-zero: device %.3f oracle %.3f"
                      % (b, scales[b], c, rms / u, e_g[0], e_g[1], e_o[0], e_o[1], nz_g, nz_o))
            if not (e_g[0] <= lim[0] and e_g[1] <= lim[1] and abs(nz_g - nz_o) <= either):
                bad.append((b, c, e_g, e_o, nz_g, nz_o))
        st.forget(b)
    ora.close()
    assert not bad, (len(bad), bad[:6])


def test_low_level_burst_keeps_the_demodulator_state_finite(gpu, oracle):
    """A burst 2^-40 below its usual level (far under one step of a 16-bit converter): decoded like the oracle decodes it, and
    every per-channel statistic finite.  The limit of this claim is DESIGN section 4.5: from about 2^-83 down the reference's own
    equaliser update divides 0 by 0 once a preamble has been found (oracle and device alike); such input is not fed here."""
    import hfdl_synth as synth
    fs, cf = 250_000, 10_000_000
    freqs = [9_972_000, 10_026_000]
    rng = np.random.default_rng(5)
    bursts = [dict(freq=freqs[0], mode=1, octets=synth.make_pdu(rng, 1), t0=0.3, amp=0.05, cfo=4.0)]
    x = synth.synth_wideband(fs, cf, int(3.5 * fs), bursts, noise_sigma=0.004, seed=31) * np.float32(2.0 ** -40)
    fe = gpu.Frontend(fs, cf, freqs)
    ora = oracle.Frontend(fs, cf, freqs)
    n = fe.input_size
    for b in range(len(x) // n):
        fe.push_block(x[b * n:(b + 1) * n])
        ora.push_block(x[b * n:(b + 1) * n])
    got = sorted((p["freq"], p["octets"]) for p in fe.poll_pdus())
    stats = fe.all_channel_stats()
    fe.close()
    assert got == sorted((p["freq"], p["octets"]) for p in ora.pdus) and len(got) == 1
    assert all(np.isfinite(v) for st in stats for v in st.values()), stats
