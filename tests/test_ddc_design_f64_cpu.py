"""CPU tests: the channel plan and the filter taps of the oracle (oracle/csdr_restated.c) and of the product (planner.h, compiled for the
host by tests/hostsim) against tests/ddc_design_f64.py, a statement of both from the definition that borrows nothing from either.

Integers and the fp32 words handed between functions are compared for equality; the taps within 4 x what the oracle shows against the
sharpest form of the model (phase register and normalising sum in fp32: oracle/PINNING.md section 7, where every figure behind a gate
here is written down); the bare float64 definition is measured and printed, and carries the properties that come from no code: where
the bin shift and the NCO put the carrier, and what the filter does at its centre, at its cut-offs, in its stop band and in the alias
rows."""
import ctypes as C
import math
import time
from fractions import Fraction

import numpy as np
import pytest

import ddc_design_f64 as D
from dumphfdl_amd import frontend as F
from test_host_logic_cpu import Plan, build_sim

CF = 100_000_000
RATES = [12_000, 250_000, 345_599, 1_000_000, 2_400_000, 8_000_000, 40_000_000, 80_000_000]
TAP_RATES = [250_000, 2_400_000, 40_000_000, 80_000_000]          # 4097, 65 537, 1 048 577 and 2 097 153 taps

# Oracle taps against the form "phase32+sum32", worst over the three channels of every length (oracle/PINNING.md section 7):
# relative RMS 1.6e-7, worst tap / largest tap 2.9e-7.  The gates are 4 x that, rounded up to one digit.
GATE_RMS, GATE_MAX = 7e-7, 2e-6
# |H| at the nominal cut-offs of the float64 definition: 0.50003 .. 0.50006 measured (a windowed sinc passes 1/2 at the ideal cut-off
# up to the window's own asymmetry about it); the margin
CUTOFF_MARGIN = 1e-4


def spectrum_errors(got, want):
    """(relative RMS error, worst element error / largest |H|) of a filter spectrum."""
    d = np.abs(np.asarray(got, np.complex128) - want)
    return float(np.sqrt(np.sum(d ** 2) / np.sum(np.abs(want) ** 2))), float(d.max() / np.abs(want).max())


# The oracle's filter spectrum against the model's as measured here, worst over the channels of a rate and rounded up to two digits
# (oracle/PINNING.md section 7): the floor of the device gate e_gpu <= 4 max(e_ora, floor); the oracle itself is held to 4 x the figure
SPECTRUM_FLOOR = {250_000: (1.7e-7, 2.2e-7), 2_400_000: (2.0e-7, 2.6e-7), 40_000_000: (2.4e-7, 3.3e-7)}


@pytest.fixture(scope="module")
def sim():
    return build_sim("libhostsim.so", [])


def u32(x):
    return int(np.float32(x).view(np.uint32))


def offsets(fs, g):
    """Channel frequencies as offsets from the receiver's centre, each inside the span check |offset| < fs / 2 (integer division):
    400 seeded ones, the edges, carriers on and beyond +fs/2, and carriers on and 1 Hz either side of a tie between two multiples of v."""
    half = fs // 2
    rng = np.random.default_rng(fs)
    offs = [int(o) for o in rng.integers(-(half - 1), half, 400)]
    offs += [half - 1, -(half - 1), 0, 1, -1, -1440]
    offs += [half - 1441, half - 1440, half - 1439, half - 720, half - 2]            # carrier just below, on and beyond +fs/2
    n, v = g.fft_size, g.v
    for k in (-(n // (3 * v)), n // (5 * v), n // (2 * v) - 3):
        tie = Fraction((v * k + v // 2) * fs, n)                                       # the carrier, in Hz, whose bin is v k + v / 2
        hz = math.ceil(tie)
        offs += [hz - 1440 + d for d in (-1, 0, 1)]
    return [o for o in offs if abs(o) < half]


@pytest.mark.parametrize("fs", RATES)
def test_plan_of_three_sides_is_the_models(sim, oracle, fs):
    """Geometry field by field on four sides (model, oracle, planner.h, hfdl_gpu_plan_geometry); per channel offsetbin, startbin and the
    fp32 words of post_shift, nco_rate, sindelta and cosdelta on three.  The oracle plans from the integers (centre, frequency) -- its
    own 1440 Hz, its own sign --, planner.h from the model's fp32 shift (the product forms that word in design_channel, which only a
    device test reaches: tests/test_gpu_filter_taps_f64.py).  And what no code says: offsetbin is the multiple of v nearest N fc, and bin
    shift and NCO together put the carrier on zero within three fp32 roundings."""
    g = D.geometry(fs)
    dec, tbw, d = oracle.geometry(fs)
    assert (g.decimation, u32(float(g.transition_bw))) == (dec, u32(tbw))
    assert sim.sim_fft_decimation_rate(fs, 5400) == dec and u32(sim.sim_transition_bw(fs, 250)) == u32(tbw)
    p = Plan()
    assert sim.sim_plan(tbw, dec, 0.0, C.byref(p)) == 0
    pg = F.plan_geometry(dec, tbw)
    names = [("pre_decimation", "pre"), ("post_decimation", "post"), ("taps_min_length", "taps_min_length"), ("taps_length", "taps_length"),
             ("fft_size", "n"), ("overlap_length", "overlap"), ("input_size", "input_size"), ("fft_inv_size", "m"), ("v", "v"), ("scrap", "scrap"),
             ("post_input_size", "post_input_size")]
    for name, short in names:
        want = getattr(g, name)
        assert getattr(d, name) == want and getattr(p, short) == want, name
        if hasattr(pg, name):
            assert getattr(pg, name) == want, name
    assert pg.decimation == dec and g.fft_size == g.overlap_length + g.input_size and g.v * g.overlap_length == g.fft_size
    n, v = g.fft_size, g.v
    beyond, worst_hz, worst_of = 0, 0.0, 0.0
    offs = offsets(fs, g)
    for off in offs:
        c = D.channel(fs, CF, CF + off, g)
        och = oracle.Channel(fs, CF, CF + off, want_channelizer=False)
        od = och.ddc
        assert sim.sim_plan(tbw, dec, float(c.shift), C.byref(p)) == 0
        mine = (c.offsetbin, c.startbin, u32(c.post_shift32), u32(c.nco_rate32), u32(c.sindelta), u32(c.cosdelta))
        assert mine == (od.offsetbin, od.startbin, u32(od.post_shift), u32(od.nco_rate), u32(od.nco_sindelta), u32(od.nco_cosdelta)), off
        assert mine == (p.offsetbin, p.startbin, u32(p.post_shift), u32(p.rate), u32(p.sindelta), u32(p.cosdelta)), off
        och.close()
        # not from the code
        assert c.offsetbin % v == 0 and abs(c.offsetbin - n * c.fc) <= Fraction(v, 2) + 1, off
        if off + 1440 >= fs / 2:
            assert c.offsetbin >= n // 2 - v // 2
        beyond += c.offsetbin > n // 2
        err, bound = abs(D.downmix_error_hz(c)), D.downmix_bound_hz(c)
        assert err <= bound, (off, err, bound)
        assert abs(D.downmix_error_hz(c, c.nco_rate)) <= bound * 2 / 3           # the float64 rate: two roundings, both in `shift`
        worst_hz, worst_of = max(worst_hz, err), max(worst_of, err / bound if bound else 0.0)
    print("fs %d: %d channels, %d with offsetbin > N/2; centre of the down-mix off by <= %.3g Hz (%.2f of the bound, %.3g Hz at +-fs/2)"
          % (fs, len(offs), beyond, worst_hz, worst_of, 3 * 2.0 ** -24 * 0.5 * fs))
    assert beyond >= 2


def test_rounding_helpers_are_the_loops_written_out():
    """f32() against numpy's float32 on awkward rationals; sum32() against the register loop; the phase register against the same loop
    on numpy float32 scalars."""
    rng = np.random.default_rng(3)
    for _ in range(2000):                                                       # a correctly rounded fp32 quotient and sum
        a, b = np.float32(rng.integers(-2 ** 40, 2 ** 40)), np.float32(rng.integers(1, 2 ** 33))
        assert D.f32(Fraction(float(a)) / Fraction(float(b))) == Fraction(float(a / b))
        assert D.f32(Fraction(float(a)) + Fraction(float(b))) == Fraction(float(a + b))
    for k in range(2000):                                                       # ties and their neighbours
        m, e = int(rng.integers(2 ** 23, 2 ** 24)), int(rng.integers(-60, 60))
        for num in (4 * m + 1, 4 * m + 2, 4 * m + 3, 4 * m + 6):                 # below, on (to even), above a tie; a tie that goes up
            q = Fraction(num, 4) * Fraction(2) ** e
            assert D.f32(q) == Fraction(float(np.float32(float(q)))), (num, e)
    t = D.lowpass_unnormalised(4097, D.f32(Fraction(1, 64)))
    s = np.float32(0)
    for x in t.astype(np.float32):
        s = np.float32(s + x)
    assert float(s) == D.sum32(t)
    center = D.f32(Fraction(48211, 250000))
    want, ph = np.empty(4097), np.float32(0)
    for i in range(4097):
        want[i] = ph
        ph = np.float32(np.float64(ph) + 2 * np.pi * np.float64(float(center)))
        while ph > 2 * np.pi:
            ph = np.float32(np.float64(ph) - 2 * np.pi)
        while ph < 0:
            ph = np.float32(np.float64(ph) + 2 * np.pi)
    assert np.array_equal(D.phase_register(4097, center), want)
    neg = D.phase_register(4097, -center)                                      # a negative centre wraps upwards
    assert neg.min() >= 0 and neg.max() <= 2 * np.pi and abs(np.exp(1j * neg[-1]) - np.exp(-1j * want[-1])) < 1e-3


def tap_channels(fs):
    """Channel frequencies as offsets from the centre: carrier 600 Hz below +fs/2, carrier 37 Hz from the centre, one ordinary."""
    return [fs // 2 - 600 - 1440, 37 - 1440, -int(0.3137 * fs) - 1440]


def circular(a, n):
    return (a + n // 2) % n - n // 2


def response_properties(tag, c, h, H, cut_tol):
    """What the filter does, read from its response H on the N bins of the block (and from direct sums at the three named
    frequencies): returns the printed figures."""
    n, fs = c.fft_size, c.sample_rate
    center, cutoff = float(c.center), float(c.cutoff)
    g0 = D.response_at(h, center)
    lo, hi = D.response_at(h, center - cutoff), D.response_at(h, center + cutoff)
    b = np.arange(n)
    dist = np.abs(circular(b - int(round(center * n)), n)) / n                        # cycles per sample from the centre, to half a bin
    stop = dist >= cutoff + 250.0 / fs + 1.0 / n
    stop_db = 20 * np.log10(np.abs(H[stop]).max() / g0)
    # alias rows: decimation by pre folds bin offsetbin + j + k M onto offsetbin + j
    pre, m, ob = c.pre_decimation, c.fft_inv_size, c.offsetbin
    if pre > 1:
        P = (np.abs(np.roll(H, -((ob - m // 2) % n))) ** 2).reshape(pre, m)            # row 0: bins ob - M/2 .. ob + M/2 - 1
        j = np.arange(m) - m // 2
        band = np.abs(j + (ob - center * n)) <= cutoff * n                              # the pass band, cut-off to cut-off
        fold_db = 10 * np.log10((P[1:].sum(axis=0)[band] / P[0][band]).max())
        fold0_db = 10 * np.log10(P[1:, m // 2].sum() / P[0, m // 2])
    else:
        fold_db = fold0_db = -np.inf
    print("%s: |H| centre %.7f, cut-offs %.5f / %.5f, stop band from cut-off + 250 Hz %.1f dB, folded onto the pass band %.1f dB (worst bin) %.1f dB (bin offsetbin)"
          % (tag, g0, lo, hi, stop_db, fold_db, fold0_db))
    assert abs(lo - 0.5) <= cut_tol and abs(hi - 0.5) <= cut_tol, (tag, lo, hi)
    assert stop_db <= -50.0, (tag, stop_db)
    assert fold_db <= -50.0 and fold0_db <= -50.0, (tag, fold_db, fold0_db)
    return g0, lo, hi


@pytest.mark.parametrize("fs", TAP_RATES)
def test_taps_of_oracle_and_product_against_the_three_forms(sim, oracle, fs):
    """Per tap count three channels.  Oracle and planner.h are handed the model's two fp32 cut-offs and must give the same words as each
    other; against the definition and the phase32 form the distance is printed, against phase32+sum32 it is gated.  Then the response:
    the float64 definition has gain 1 at its centre, 1/2 at both cut-offs, 50 dB from cut-off + 250 Hz on and 50 dB between what the
    decimation folds onto the pass band and the pass band; the fp32 taps are held to the sharp form's response at those frequencies by
    sum |dh| <= taps x GATE_MAX x largest tap."""
    g = D.geometry(fs)
    L, n = g.taps_length, g.fft_size
    for off in tap_channels(fs):
        t0 = time.time()
        c = D.channel(fs, CF, CF + off, g)
        forms = D.channel_taps(fs, CF, CF + off)
        t_model = time.time() - t0
        a, b = np.zeros(L, np.complex64), np.zeros(L, np.complex64)
        oracle.lib().orc_firdes_bandpass_c(a.ctypes.data, L, float(c.lowcut), float(c.highcut))
        sim.sim_bandpass(b.ctypes.data, L, float(c.lowcut), float(c.highcut))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        tag = "fs %d, %d taps, carrier %+d Hz" % (fs, L, off + 1440)
        for name, side in (("oracle", a), ("planner.h", b)):
            e = [D.tap_errors(side, forms[f]) for f in D.FORMS]
            print("%s, %s: definition %.3g / %.3g | phase32 %.3g / %.3g | phase32+sum32 %.3g / %.3g  (relative RMS / worst tap over largest)"
                  % (tag, name, *e[0], *e[1], *e[2]))
            assert e[2][0] <= GATE_RMS and e[2][1] <= GATE_MAX, (tag, name, e[2])
        sharp, defn = forms["phase32+sum32"], forms["definition"]
        print("%s: register off 2 pi center (taps - 1) by %+.3g rad at the last tap; sum32 / sum - 1 = %+.3g; model %.2f s"
              % (tag, D.phase_drift(L, c.center), np.abs(defn).sum() / np.abs(sharp).sum() - 1, t_model))
        H = D.spectrum(defn, n)
        g0, _, _ = response_properties(tag + ", definition", c, defn, H, CUTOFF_MARGIN)
        assert abs(g0 - 1) < 1e-9
        del H
        # the fp32 sides at the same three frequencies, against the sharp form's response there
        lim = L * GATE_MAX * np.abs(sharp).max()
        for f in (float(c.center), float(c.center - c.cutoff), float(c.center + c.cutoff)):
            dh = D.response_at(a.astype(np.complex128) - sharp, f)
            assert dh <= lim, (tag, f, dh, lim)
        print("%s: oracle |H| at the cut-offs %.5f / %.5f (sharp form %.5f / %.5f), |dH| limit %.2g"
              % (tag, D.response_at(a, float(c.center - c.cutoff)), D.response_at(a, float(c.center + c.cutoff)),
                 D.response_at(sharp, float(c.center - c.cutoff)), D.response_at(sharp, float(c.center + c.cutoff)), lim))


@pytest.mark.parametrize("fs", [250_000, 2_400_000, 40_000_000])
def test_oracle_filter_spectrum_against_the_model(oracle, fs):
    """The oracle's frequency-domain filter (fp32 taps through its fp32 transform, halves swapped) against the float64 transform of the
    sharp-form taps: the figures that are the `floor` of the device gate in tests/test_gpu_filter_taps_f64.py."""
    worst = [0.0, 0.0]
    for off in tap_channels(fs)[:2 if fs > 2_400_000 else 3]:
        c = D.channel(fs, CF, CF + off)
        want = np.fft.fftshift(D.spectrum(D.channel_taps(fs, CF, CF + off)["phase32+sum32"], c.fft_size))
        och = oracle.Channel(fs, CF, CF + off)
        e = spectrum_errors(och.taps_fft(), want)
        och.close()
        print("fs %d carrier %+d Hz, N = 2^%d: oracle filter spectrum rel rms %.3g, worst / largest |H| %.3g" % (fs, off + 1440, c.fft_size.bit_length() - 1, *e))
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    assert worst[0] <= 4 * SPECTRUM_FLOOR[fs][0] and worst[1] <= 4 * SPECTRUM_FLOOR[fs][1], worst


def test_oracle_channelizer_on_the_models_plan_and_taps(oracle):
    """ddc_f64.ddc_reference fed channel_plan_f64 -- plan and taps from the definition, nothing of the oracle's -- against the oracle's
    chan_out at 250 ksps (edge, on a multiple of v, ordinary; four blocks): the gates of tests/test_channelizer_f64_cpu.py, which were
    measured with the oracle's own plan and taps in the model (the taps differ by 2e-7, the gates are 3e-4 and 7e-4)."""
    import ddc_f64 as M
    import test_channelizer_f64_cpu as T
    fs = 250_000
    g, freqs, x, got = T.run_case(oracle, fs)
    worst = [0.0, 0.0]
    for c, f in enumerate(freqs):
        plan, taps = M.channel_plan_f64(fs, T.CF, f)
        mine, _ = M.channel_plan(oracle, fs, T.CF, f)
        assert (plan.offsetbin, u32(plan.nco_rate)) == (mine.offsetbin, u32(mine.nco_rate))
        for b, want in enumerate(M.ddc_reference(x, taps, plan)):
            e = M.errors(got[c][b], want)
            worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    print("fs %d, the model's own plan and taps: oracle chan_out rel rms %.3g worst/rms %.3g" % (fs, worst[0], worst[1]))
    assert worst[0] <= T.GATE_RMS and worst[1] <= T.GATE_MAX, worst
