"""GPU tests: the device channelizer against the float64 direct-form model (tests/ddc_f64.py) in every fold form.

One gate everywhere, calibrated by the oracle on the same input so that no tolerance is invented: per (block, channel)
e_gpu = error of the device chan_out against the model, e_ora = error of the oracle's chan_out against the same model, both as
relative RMS and as worst element / RMS of the model output, and

    e_gpu <= 4 * max(e_ora, floor)

with floor = the oracle-against-model figures of oracle/PINNING.md for the geometry.  Device and oracle are two fp32 evaluations of
the same sums with different FFT factorisations and summation orders; a wrong alias row, bin, scrap index or block column is orders
of magnitude outside a factor of 4.  For e_gpu the model runs with the device's own NCO phasor tables (tap 9: the fp32 phasor recurrence's drift is not the
fold's; the tables themselves are bounded against the float64 phase); e_ora, the calibrating side, uses the float64 phase.  The
device is never compared with itself.

Both fold paths are covered.  The matrix-pipe fold (pre_decimation a multiple of 8: 96 ksps, its smallest geometry, 250 ksps, 2.048,
2.4, 40 and 80 Msps) and, in the second half of the file, the plain-VALU fold_ref_kernel on the unpadded tap layout, which is the
shipped fold of every receiver below 86 400 sps (pre_decimation 1, 2 or 4): its passes of four blocks, full and ragged, its branch
for fewer than four alias rows, several receivers, a retune, post_decimation = 1 and the inverse FFT at M = N.  Where the comparison
is between two runs of the device (batching, retune, HFDL_GPU_FOLD_PRUNE) it is a comparison of uint32 words that says "this launch
shape changes nothing"; what the words ARE is held to the model by the tests beside it on the same geometry."""
import numpy as np
import pytest

import ddc_f64 as M
from dumphfdl_amd import frontend as F

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-4
# oracle against model as measured on the CPU (oracle/PINNING.md, tests/test_channelizer_f64_cpu.py): (relative RMS, worst / RMS)
FLOOR = {250_000: (6.3e-5, 1.6e-4), 2_400_000: (3.6e-5, 1.3e-4),
         # the geometries of 1 .. 8 alias rows (MEASURED of the CPU test; PINNING section 3's table)
         12_000: (1.8e-5, 6.2e-5), 24_000: (6.6e-5, 1.9e-4), 48_000: (9.9e-5, 2.5e-4), 64_000: (1.1e-4, 3.2e-4), 96_000: (6.2e-5, 1.7e-4),
         # pre = post = 1, against the model times (-1)^K (MEASURED_HALF_RATE of the CPU test)
         8_000: (9.2e-6, 3.8e-5), 10_799: (3.2e-5, 1.3e-4)}
FLOOR_ANY = (6.3e-5, 1.6e-4)          # the worst over the five rates measured first: the large geometries outside that table
# (pre_decimation, inverse FFT size) of the receivers below 250 ksps.  pre < 8: TAPL_PLAIN, the unpadded tap layout, which
# fold_ref_kernel folds on the vector ALUs (frontend_create.cpp, fold_kernels.hip pick_variant); pre = 8: the smallest geometry of the
# matrix-pipe fold, one look-ahead group of two quads of alias rows
SMALL_RATES = {8_000: (1, 2048), 10_799: (1, 2048), 12_000: (1, 2048), 24_000: (2, 2048), 48_000: (4, 2048), 64_000: (4, 4096), 96_000: (8, 2048)}


def read_blocks(fe, held, first_block, channels, dev):
    """chan_out (tap 3) and NCO phasors (tap 9) of the `held` newest blocks, which are stream blocks first_block .. first_block + held - 1."""
    with pytest.raises(F.GpuError):
        fe.read_tap(F.TAP_CHAN_OUT, channels[0], back=held)                 # exactly `held` blocks are in the newest half
    for j in range(held):
        back = held - 1 - j
        dev[first_block + j] = {c: (fe.read_tap(F.TAP_CHAN_OUT, c, back=back), fe.read_tap(F.TAP_NCO_PHASORS, c, back=back)) for c in channels}


def compare(tag, oracle, fs, cf, freqs, x, dev, floor, gate=True, rms_tol=None, half_rate=False):
    """dev: {block: {index into freqs: (chan_out, phasors)}} of one receiver's stream x.  Returns the worst (e_gpu, e_ora, ratio) pairs.
    half_rate: the model times (-1)^K on both sides (pre_decimation = post_decimation = 1: oracle/PINNING.md section 3)."""
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
            if half_rate:
                assert plan.pre_decimation == plan.post_decimation == 1
                model = model * M.half_rate_sign(K)
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
    matrix pipe (rows per slice a multiple of 4: asserted); the plain-VALU fold has
    test_small_geometries_in_every_launch_shape_against_the_float64_model below."""
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


# ---------------------------------------------------------------- the receivers below 250 ksps: 1 .. 8 alias rows

def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def small_rate_freqs(oracle, fs, cf, pick=(0, 1, 2), extra=()):
    """Channels as the CPU test picks them (ddc_f64.channel_offsets: within 1 kHz of +fs / 2, on a multiple of v, ordinary) + extra offsets."""
    _, _, d = oracle.geometry(fs)
    offs = M.channel_offsets(fs, d.overlap_length)
    return [cf + f - 1440 for f in [offs[i] for i in pick] + list(extra)]


def assert_fold_path(g, fs):
    """The geometry is the one meant and the fold path the one meant: True where fold_ref_kernel folds (the plain layout)."""
    pre, m = SMALL_RATES[fs]
    assert (g.pre_decimation, g.fft_inv_size, g.fold_slices, g.fold_rows) == (pre, m, 1, pre)
    rows = g.pre_decimation // g.fold_slices
    if pre % 8 == 0:
        assert rows == 8 and g.fft_inv_size % 16 == 0, "the matrix form is not what folds here"
        return False
    assert rows % 4 != 0 or rows < 8, "the matrix-pipe fold on this geometry: the plain-VALU kernel is not covered"
    return True


def fold_launches(k, nb_max, thirty_two):
    """Launch sizes of a half of k blocks: fold_launch_blocks (fold_kernels.hip) as it reads, unpruned.  Up to nb_max (at most 32) blocks a
    launch; 17 .. 20 go as sixteen and the rest; more than 16 need a thirty-two-column tiling, which only an octet layout has."""
    out = []
    while k:
        take = min(k, nb_max, 32)
        if 16 < take <= 20 or (take > 16 and not thirty_two):
            take = 16
        out.append(take)
        k -= take
    return out


def shape_counts(halves, nb_max, thirty_two):
    want = {}
    for k in halves:
        for nb in fold_launches(k, nb_max, thirty_two):
            want[nb] = want.get(nb, 0) + 1
    return want


@pytest.mark.parametrize("fs", [12_000, 24_000, 48_000, 64_000, 96_000])
def test_small_geometries_in_every_launch_shape_against_the_float64_model(gpu, oracle, monkeypatch, fs):
    """1, 2 and 4 alias rows (fold_ref_kernel on the plain layout: its `rows - r < 4` branch at 1 and 2 rows, M = 2048 and 4096 at 4) and
    8 rows (the matrix-pipe fold's smallest geometry), where EVERY alias row reaches the output.  One continuous stream in halves of
    1, 3, 4, 5, 8, 9, 16 and 21 blocks, each closed by a sync, every block of every half against the model: fold_ref_kernel's passes of
    four blocks full, ragged (3, 5 = 4 + 1, 9 = 4 + 4 + 1) and repeated; 21 blocks are 16 + 5 on the plain layout (no thirty-two-column
    tiling) and one launch at 96 ksps."""
    cf = 10_000_000
    freqs = small_rate_freqs(oracle, fs, cf, extra=[int(0.127 * fs)] + ([-fs // 2 + 2200] if fs >= 24_000 else []))
    counts = [1, 3, 4, 5, 8, 9, 16, 21]
    monkeypatch.setenv("HFDL_GPU_FOLD_BATCH", "32")
    fe = gpu.Frontend(fs, cf, freqs)
    g = fe.geometry
    assert g.fold_batch == 32
    plain = assert_fold_path(g, fs)
    n = fe.input_size
    dec = oracle.lib().orc_compute_fft_decimation_rate(fs, 5400)
    x = M.make_signal(fs, cf, freqs, freqs, sum(counts) * n, 600 + fs // 1000, dec, g.pre_decimation)
    fe.reset_timers(True)
    dev, b = {}, 0
    for k in counts:
        for j in range(k):
            fe.push_block(x[(b + j) * n:(b + j + 1) * n])
        fe.sync()
        read_blocks(fe, k, b, list(range(len(freqs))), dev)
        b += k
    shapes = fe.fold_launch_shapes()
    stats = fe.all_channel_stats()
    fe.close()
    want = shape_counts(counts, 32, not plain)
    print("fs %d (%s layout) fold launches by block count:" % (fs, "plain" if plain else "octet"), shapes)
    assert shapes == want, (shapes, want)
    assert want == ({1: 1, 3: 1, 4: 1, 5: 2, 8: 1, 9: 1, 16: 2} if plain else {1: 1, 3: 1, 4: 1, 5: 1, 8: 1, 9: 1, 16: 1, 21: 1})
    assert all(np.isfinite(v) for st in stats for v in st.values()), stats
    compare("fs %d x %d channels, %d alias rows, %d blocks" % (fs, len(freqs), g.pre_decimation, len(dev)), oracle, fs, cf, freqs, x, dev, FLOOR[fs])


@pytest.mark.parametrize("fs,offs", [(12_000, [-2_000]), (48_000, [-15_000, 9_000, 20_500])])
def test_fold_batching_changes_nothing_on_the_plain_layout(gpu, oracle, monkeypatch, fs, offs):
    """The reduced twin of test_gpu_parity.py::test_fold_batching_changes_nothing where fold_ref_kernel is the shipped fold: chan_out of
    every block as uint32, every PDU and every statistic of a launch per block (HFDL_GPU_FOLD_BATCH=1) against batches of 4, 8 and 16 cut
    ragged by draining polls (13, 3, 1, 5, 9 blocks: halves that close full on the way and passes of one to four blocks).  31 blocks
    with one burst per channel; the bursts decode, and as the oracle decodes them."""
    import hfdl_synth as synth
    cf = 10_000_000
    freqs = [cf + o for o in offs]
    rng = np.random.default_rng(fs)
    bursts = [dict(freq=f, mode=int(rng.integers(0, 4)), octets=b"", t0=0.4 + 0.1 * i, amp=0.05, cfo=float(rng.uniform(-10, 10))) for i, f in enumerate(freqs)]
    for bu in bursts:
        bu["octets"] = synth.make_pdu(rng, bu["mode"])
    dec, _, d = oracle.geometry(fs)
    n, nblk = d.input_size, 31
    x = synth.synth_wideband(fs, cf, nblk * n, bursts, noise_sigma=0.01 * np.sqrt(dec / 32.0), seed=3)
    chans = list(range(len(freqs)))

    def run(fold_env, cuts):
        monkeypatch.setenv("HFDL_GPU_FOLD_BATCH", str(fold_env))
        fe = gpu.Frontend(fs, cf, freqs)
        g = fe.geometry
        assert g.fold_batch == fold_env and fe.input_size == n and assert_fold_path(g, fs)
        half = min(32, -(-max(g.fold_batch, g.demod_batch) // g.fold_batch) * g.fold_batch)      # blocks a half holds (planner.h plan_batches, half_blocks)
        outs, got, b, i = {}, [], 0, 0
        while b < nblk:
            k = min(cuts[i % len(cuts)], nblk - b)
            i += 1
            for j in range(k):
                fe.push_block(x[(b + j) * n:(b + j + 1) * n])
            got += fe.poll_pdus()                 # closes the half as it is
            held = k % half or min(k, half)       # blocks of the newest half: what read_tap(back=...) still reaches
            for j in range(held):
                outs[b + k - held + j] = [u32(fe.read_tap(F.TAP_CHAN_OUT, c, back=held - 1 - j)).copy() for c in chans]
            b += k
        stats = fe.all_channel_stats()
        fe.close()
        return outs, sorted(got, key=lambda p: (p["freq"], p["sample_index"])), stats

    ref_outs, ref_pdus, ref_stats = run(1, [1])
    assert sorted(ref_outs) == list(range(nblk)) and all(len(a) == 2 * (d.post_input_size // d.post_decimation) for v in ref_outs.values() for a in v)
    ora = oracle.Frontend(fs, cf, freqs)
    for b in range(nblk):
        ora.push_block(x[b * n:(b + 1) * n])
    want = sorted((p["freq"], p["sample_index"], p["octets"]) for p in ora.pdus)
    ora.close()
    assert [(p["freq"], p["sample_index"], p["octets"]) for p in ref_pdus] == want and len(want) == len(freqs)
    for fold_env in (4, 8, 16):
        outs, pdus, stats = run(fold_env, [13, 3, 1, 5, 9])
        assert len(outs) >= 5, (fold_env, sorted(outs))
        for blk, v in outs.items():
            for c, a in zip(chans, v):
                assert np.array_equal(a, ref_outs[blk][c]), (fold_env, blk, c)
        assert pdus == ref_pdus, fold_env               # every field of every PDU
        assert stats == ref_stats, fold_env


@pytest.mark.parametrize("fs,pick", [(8_000, (0, 2)), (10_799, (2,))])
def test_post_decimation_1_against_the_float64_model_and_the_oracle(gpu, oracle, fs, pick):
    """Below 10 800 sps pre_decimation = post_decimation = 1: the inverse FFT has the forward FFT's size, every sample of it past the
    scrap is an output, and the reference's bin arithmetic leaves (-1)^K on the output (oracle/PINNING.md section 3;
    tests/test_channelizer_f64_cpu.py::test_half_rate_shift_below_10800_sps).  The device is held to the REFERENCE's arithmetic: its
    chan_out against the model times (-1)^K under the gate of every other geometry, six blocks in one half; every block yields
    post_input_size outputs; the statistics stay finite; and on a stream with one clean burst the PDU list is the oracle's, which is
    empty: such a receiver is accepted, as the reference accepts it, and decodes nothing.  10 799 sps: resampling rate 0.50005, the
    resampler's lower edge."""
    import hfdl_synth as synth
    cf = 10_000_000
    freqs = small_rate_freqs(oracle, fs, cf, pick=pick)
    fe = gpu.Frontend(fs, cf, freqs)
    g = fe.geometry
    assert assert_fold_path(g, fs) and g.post_decimation == 1 and g.fft_inv_size == g.fft_size
    assert abs(g.resamp_rate - 5400.0 / fs) < 1e-6 and 0.5 < g.resamp_rate < (0.5001 if fs == 10_799 else 0.7)
    n = fe.input_size
    x = M.make_signal(fs, cf, freqs, freqs, 6 * n, 700 + fs // 1000, 1, 1)
    fe.reset_timers(True)
    for b in range(6):
        fe.push_block(x[b * n:(b + 1) * n])
    fe.sync()
    dev = {}
    read_blocks(fe, 6, 0, list(range(len(freqs))), dev)
    assert fe.fold_launch_shapes() == {6: 1}
    for b, v in dev.items():
        for c, (out, ph) in v.items():
            assert len(out) == len(ph) == g.post_input_size, (b, c, len(out))
    stats = fe.all_channel_stats()
    fe.close()
    assert all(np.isfinite(v) for st in stats for v in st.values()), stats
    compare("fs %d x %d channels, post_decimation 1" % (fs, len(freqs)), oracle, fs, cf, freqs, x, dev, FLOOR[fs], half_rate=True)
    # one clean burst on channel 0, the stream of test_other_sample_rates: decoded at 12 ksps, not here
    rng = np.random.default_rng(fs)
    mode = int(rng.integers(0, 4))
    bursts = [dict(freq=freqs[0], mode=mode, octets=synth.make_pdu(rng, mode), t0=0.4, amp=0.05, cfo=float(rng.uniform(-10, 10)))]
    nblk = int(3.4 * fs) // n + 1
    y = synth.synth_wideband(fs, cf, nblk * n, bursts, noise_sigma=0.01 * np.sqrt(1 / 32.0), seed=3)
    fe = gpu.Frontend(fs, cf, freqs)
    ora = oracle.Frontend(fs, cf, freqs)
    for b in range(nblk):
        fe.push_block(y[b * n:(b + 1) * n])
        ora.push_block(y[b * n:(b + 1) * n])
    got = sorted((p["freq"], p["sample_index"], p["octets"]) for p in fe.poll_pdus())
    stats = fe.all_channel_stats()
    fe.close()
    want = sorted((p["freq"], p["sample_index"], p["octets"]) for p in ora.pdus)
    ora.close()
    assert got == want and want == []
    assert all(np.isfinite(v) for st in stats for v in st.values()), stats


def test_three_receivers_on_the_plain_layout_against_the_float64_model(gpu, oracle, monkeypatch):
    """Receivers of 3, 1 and 2 channels at 48 ksps with centres and streams of their own, nine blocks in one half.  The plain layout
    pads nothing (tap_layout_group = 1): slot = channel, and fold_ref_kernel finds a channel's spectrum by rx_of_channel.  Every
    channel against the model of ITS receiver's centre and stream."""
    fs = 48_000
    centres = [10_000_000, 11_500_000, 8_700_000]
    picks = [((0, 1, 2), ()), ((2,), ()), ((0,), (int(0.127 * fs),))]
    recv = [(cf, small_rate_freqs(oracle, fs, cf, pick=p, extra=e)) for cf, (p, e) in zip(centres, picks)]
    nchs = [len(fr) for _, fr in recv]
    monkeypatch.setenv("HFDL_GPU_FOLD_BATCH", "32")
    fe = gpu.MultiFrontend(fs, recv)
    g = fe.geometry
    assert g.fold_batch == 32 and g.channels == 6 and nchs == [3, 1, 2] and assert_fold_path(g, fs)
    n = fe.input_size
    dec = oracle.lib().orc_compute_fft_decimation_rate(fs, 5400)
    xs = [M.make_signal(fs, cf, fr, fr, 9 * n, 800 + r, dec, g.pre_decimation) for r, (cf, fr) in enumerate(recv)]
    fe.reset_timers(True)
    for b in range(9):
        fe.push_blocks([x[b * n:(b + 1) * n] for x in xs])
    fe.sync()
    dev = {}
    read_blocks(fe, 9, 0, list(range(6)), dev)
    shapes = fe.fold_launch_shapes()
    fe.close()
    assert shapes == {9: 1}, shapes
    base = np.concatenate([[0], np.cumsum(nchs)])
    for r, (cf, fr) in enumerate(recv):
        d = {blk: {i: v[int(base[r]) + i] for i in range(nchs[r])} for blk, v in dev.items()}
        compare("receiver %d (%d channels) of 3 on the plain layout, fs %d" % (r, nchs[r], fs), oracle, fs, cf, fr, xs[r], d, FLOOR[fs])


def test_retune_on_the_plain_layout(gpu, oracle):
    """Cases 1 - 3 of tests/test_gpu_retune.py at 48 ksps, where the retuned channel's taps go through store_out's plain branch into the
    unpadded layout: channel 1 of 3 moves at block 5 of 10, everything pushed at once (the retune closes the half of five).  Block 4 is
    zeros, so the history at the boundary is a fresh front end's.  After the boundary channel 1's filter and chan_out are, as uint32,
    those of a front end created with the new frequency and fed blocks 5 .. 9; before it they are the never-retuned run's; channels 0
    and 2 are the never-retuned run's throughout."""
    fs, cf, CH, K, NALL = 48_000, 10_000_000, 1, 5, 10
    freqs = [cf - 15_000, cf + 9_000, cf + 20_500]
    f_new = cf + 2_300
    fresh = list(freqs)
    fresh[CH] = f_new
    dec, _, d = oracle.geometry(fs)
    n = d.input_size
    x = M.make_signal(fs, cf, freqs + [f_new], freqs + [f_new], NALL * n, 900, dec, d.pre_decimation)
    x[(K - 1) * n:K * n] = 0

    def run(fr, first, retune_at=None):
        fe = gpu.Frontend(fs, cf, fr)
        assert assert_fold_path(fe.geometry, fs) and fe.input_size == n
        fe.export_enable([0, 1, 2], ring_blocks=64)
        for b in range(first, NALL):
            if b == retune_at:
                fe.retune(CH, f_new)
            fe.push_block(x[b * n:(b + 1) * n])
        fe.sync()
        samples, counts, _, _, blocks, _ = fe.export_read(0, wait=True)
        assert blocks == list(range(NALL - first))
        filters = [u32(fe.read_tap(F.TAP_FILTER, c)).copy() for c in range(3)]
        fe.close()
        return u32(samples), counts, filters              # [block][channel][P]

    A, A_cnt, A_fil = run(freqs, 0, retune_at=K)
    B, B_cnt, B_fil = run(fresh, K)
    A1, A1_cnt, A1_fil = run(freqs, 0)
    P = d.post_input_size // d.post_decimation
    assert np.all(A_cnt == P) and np.all(B_cnt == P) and np.all(A1_cnt == P)
    assert np.array_equal(A_fil[CH], B_fil[CH]) and not np.array_equal(A_fil[CH], A1_fil[CH])
    for c in (0, 2):
        assert np.array_equal(A_fil[c], A1_fil[c]) and np.array_equal(A_fil[c], B_fil[c]), c
        assert np.array_equal(A[:, c], A1[:, c]), c
    assert np.array_equal(A[K:, CH], B[:, CH])
    assert np.array_equal(A[:K, CH], A1[:K, CH])
    assert not np.array_equal(A[K:, CH], A1[K:, CH])
    assert np.mean(A[K:, CH, :2 * P] != 0) > 0.99 and np.mean(A[:K - 1, CH, :2 * P] != 0) > 0.99          # (the words compared are not zeros)


def test_fold_prune_is_off_on_the_plain_layout(gpu, oracle, monkeypatch):
    """HFDL_GPU_FOLD_PRUNE is the octet layout's (row windows per octet): on a plain geometry create reads it as off --
    geometry.fold_rows reports every row, and chan_out is, as uint32, the unset run's."""
    fs, cf = 48_000, 10_000_000
    freqs = small_rate_freqs(oracle, fs, cf)
    dec, _, d = oracle.geometry(fs)
    n = d.input_size
    x = M.make_signal(fs, cf, freqs, freqs, 5 * n, 950, dec, d.pre_decimation)
    words = []
    for prune in (None, "3e-7"):
        if prune:
            monkeypatch.setenv("HFDL_GPU_FOLD_PRUNE", prune)
        else:
            monkeypatch.delenv("HFDL_GPU_FOLD_PRUNE", raising=False)
        fe = gpu.Frontend(fs, cf, freqs)
        assert assert_fold_path(fe.geometry, fs) and fe.geometry.fold_rows == fe.geometry.pre_decimation
        for b in range(5):
            fe.push_block(x[b * n:(b + 1) * n])
        fe.sync()
        words.append([u32(fe.read_tap(F.TAP_CHAN_OUT, c, back=4 - b)).copy() for b in range(5) for c in range(3)])
        fe.close()
    assert all(len(a) and np.array_equal(a, b) for a, b in zip(*words))
    assert np.mean(np.concatenate(words[0]) != 0) > 0.99
