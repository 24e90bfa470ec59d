"""CPU tests: the float64 model of the demodulator's per-sample front (tests/demod_f64.py) against the product's table design, against
an analytic property of the resampler, and against the oracle (oracle/PINNING.md section 4 holds the measured figures behind every gate
that is not derived)."""
import ctypes as C

import numpy as np
import pytest

import demod_f64 as M
from test_constants_cpu import DemodTables
from test_host_logic_cpu import build_sim

RATES = [0.6912, 0.55296, 0.500001, 1.0]
# sample rate -> resampler rate 5400 / (fs / decimation): 0.6912, 0.500001 (the slowest the geometry allows, branch step just above 2),
# exactly 1 (every output on branch 0)
STREAM_FS = [250_000, 345_599, 345_600]
SEEDS = [11, 12, 13]                 # one stream per channel of tests/test_gpu_demod_front_f64.py

# Oracle table against the float64 design, worst |difference| / largest tap: 5.2e-7, 8.1e-7, 1.2e-6, 2.3e-6 at the four rates.  Both
# designs hand the cut-off to the prototype as fp32 (6e-8 of an argument of sinc that reaches 7 at the prototype's end), round the
# prototype to fp32 and sum its gain in fp32, in an order that may differ.  The product's gate: 4 x the worst, rounded up to one digit.
TABLE_GATE = 9e-6

# Oracle against the model on the edge stream, worst over three seeds and both elementary-function sets (oracle/PINNING.md section 4).
# (resampler relative RMS, worst / RMS, matched filter relative RMS, worst / RMS, AGC level relative RMS, worst sample)
MEASURED = {
    250_000: (7.3e-7, 3.6e-6, 1.9e-7, 4.2e-6, 2.5e-5, 9.0e-5),
    345_599: (2.1e-6, 1.1e-5, 2.0e-7, 4.5e-6, 2.6e-5, 9.3e-5),
    345_600: (8.1e-8, 5.0e-7, 2.2e-7, 6.4e-6, 2.4e-5, 8.7e-5),
}


def gate(v):
    """4 x the measured figure, rounded up to one digit"""
    e = np.floor(np.log10(4 * v))
    return float(np.ceil(4 * v / 10 ** e - 1e-9) * 10 ** e)


@pytest.fixture(scope="module")
def sim():
    H = build_sim("libhostsim.so", [])
    H.sim_tables.argtypes = [C.c_float, C.c_void_p]
    return H


def product_tables(sim, rate):
    t = DemodTables()
    sim.sim_tables(rate, C.byref(t))
    return np.frombuffer(t.rs_h, np.float32).copy(), int(t.rs_step), np.frombuffer(t.mf, np.float32).copy()


def oracle_tables(oracle, rate):
    h = np.zeros(M.NPFB * M.RS_TAPS, np.float32)
    step = C.c_uint32(0)
    oracle.lib().orc_resamp_filter(C.c_float(rate), h.ctypes.data_as(C.c_void_p), C.byref(step))
    return h, int(step.value)


def stream_rate(oracle, fs):
    dec = oracle.lib().orc_compute_fft_decimation_rate(fs, 5400)
    return float(np.float32(5400) / (np.float32(fs) / np.float32(dec)))


def test_the_stream_rates_are_the_three_cases(oracle):
    r = [stream_rate(oracle, fs) for fs in STREAM_FS]
    assert r[0] == float(np.float32(0.6912)) and abs(r[1] - 0.5000014) < 1e-7 and r[2] == 1.0
    # the branch sequences differ in kind: every branch / every other branch with a slow drift / branch 0 only
    steps = [M.design(v)[1] for v in r]
    assert steps[2] == 1 << 24 and 0 < (1 << 25) - steps[1] < 256 and steps[0] % (1 << 16) != 0


@pytest.mark.parametrize("rate", RATES)
def test_tables_against_the_float64_design(sim, oracle, rate):
    want, step = M.design(rate)
    want = want.ravel()
    ph, ps, pm = product_tables(sim, rate)
    oh, os_ = oracle_tables(oracle, rate)
    e_ora = float(np.abs(oh - want).max() / np.abs(want).max())
    e_prod = float(np.abs(ph - want).max() / np.abs(want).max())
    print("rate %g: table against the float64 design, worst / largest tap: oracle %.3g product %.3g" % (rate, e_ora, e_prod))
    assert ps == os_ == step
    assert e_ora <= TABLE_GATE and e_prod <= TABLE_GATE
    assert np.array_equal(pm.astype(np.float64), M.matched_filter_taps())


@pytest.mark.parametrize("f", [0.0, 0.05, -0.05, 0.18, -0.18])
@pytest.mark.parametrize("rate", [0.6912, 1.0])
def test_a_tone_comes_out_delayed_by_seven_samples(sim, rate, f):
    """Not from liquid's text: a polyphase interpolator of a linear-phase prototype centred on tap 7 * 256 is a pure delay of 7 input
    samples inside its pass band.  Output k sits at input time t_k / 2^24; the branch is that time's fraction cut to 1 / 256, which
    moves the phase by at most 2 pi |f| / 256; the design's 60 dB ripple adds 1e-3.  (0.18 cycles per input sample is the edge of an
    HFDL channel at rate 0.6912: 1400 Hz of 7812.5.)  Rates 0.6912 and 1 only: the Kaiser transition is 256 (60 - 7.95) / (14.36 n) =
    0.26 cycles per input sample wide around fc = 0.515 rate, so the pass band ends at 0.227 and 0.36 there but at 0.128 for rate
    0.500001 -- 0.18 is in its transition band -- and at that rate the float64 design's own branches are off a pure delay by 2.4e-3 at
    f = 0.05 (measured on the design alone, exact branch times): the 60 dB figure is not a property of that design."""
    m = M.DemodFrontF64(tables=product_tables(sim, rate))
    n = 2000
    out = m.resample(np.exp(2j * np.pi * f * np.arange(n)))
    t = m.t / float(1 << 24)
    ok = t >= M.RS_TAPS - 1                       # the zero history has left the window
    want = np.exp(2j * np.pi * f * (t - 7.0))
    err = float(np.abs(out - want)[ok].max())
    print("rate %g f %+.2f: |out - exp(2 pi j f (t - 7))| <= %.3g, bound %.3g" % (rate, f, err, 2 * np.pi * abs(f) / 256 + 1e-3))
    assert ok.sum() > 900 and err <= 2 * np.pi * abs(f) / 256 + 1e-3


@pytest.mark.parametrize("rate", [0.6912, 0.55296])
def test_a_tone_beyond_the_transition_band_is_rejected(sim, rate):
    """0.495 cycles per input sample: the design says 60 dB; 50 dB asserted (at rate 0.6912 the transition band ends at 0.486)."""
    m = M.DemodFrontF64(tables=product_tables(sim, rate))
    out = m.resample(np.exp(2j * np.pi * 0.495 * np.arange(2000)))
    ok = m.t / float(1 << 24) >= M.RS_TAPS - 1
    worst = float(np.abs(out)[ok].max())
    print("rate %g: tone at 0.495 comes out at %.1f dB" % (rate, 20 * np.log10(worst)))
    assert worst <= 10 ** (-50 / 20)


def oracle_front(oracle, fs, x, blocks=10):
    """(resampled, level, mf_out) of the oracle's channel on baseband x pushed in `blocks` blocks, and the per-block output counts."""
    ch = oracle.Channel(fs, 10_000_000, 10_000_000, want_channelizer=False)
    blk = len(x) // blocks + 1
    R, L, F, counts = [], [], [], []
    for i in range(0, len(x), blk):
        ch.process_baseband(x[i:i + blk])
        v = ch.view()
        R.append(v["resampled"]); L.append(v["agc_level"]); F.append(v["mf_out"]); counts.append(len(v["resampled"]))
    ch.close()
    return np.concatenate(R), np.concatenate(L), np.concatenate(F), counts


def model_front(tables, x, blocks=10):
    m = M.DemodFrontF64(tables=tables)
    blk = len(x) // blocks + 1
    out = [m.push(x[i:i + blk]) for i in range(0, len(x), blk)]
    return m, [np.concatenate([o[j] for o in out]) for j in range(4)], [len(o[0]) for o in out]


def edge_condition(m):
    """What the edge stream must do to the model for the comparison to mean something: the gain stays inside fp32's normal range, sits in
    the 1e6 clamp for a while, and no y2 is so close to the 1e-6 threshold that two roundings could decide differently."""
    g, y2 = np.array(m.g_trace), np.array(m.y2_trace)
    assert 1e-30 <= g.min() and g.max() <= 1e6
    assert int((g >= 1e6).sum()) >= 100
    assert float(np.abs(y2 / M.Y2_MIN - 1.0).min()) > 1e-3
    return float(g.min()), int((g >= 1e6).sum())


@pytest.mark.parametrize("shared_math", [0, 1])
@pytest.mark.parametrize("fs", STREAM_FS)
def test_oracle_against_the_model_on_the_edge_stream(oracle, fs, shared_math):
    rate = stream_rate(oracle, fs)
    oh, step = oracle_tables(oracle, rate)
    tables = (oh, step, M.matched_filter_taps())
    worst = np.zeros(6)
    oracle.set_variant(shared_math=shared_math)
    try:
        for seed in SEEDS:
            x = M.edge_stream(seed, rate)
            R, L, F, counts = oracle_front(oracle, fs, x)
            m, (r, _, l, f), mcounts = model_front(tables, x)
            assert counts == mcounts
            gmin, clamped = edge_condition(m)
            e = np.array([M.rel_rms(R, r), M.worst_over_rms(R, r), M.rel_rms(F, f), M.worst_over_rms(F, f), *M.level_errors(L, l)])
            print("fs %d seed %d shared_math %d: %d outputs, gain in [%.2g, 1e6], clamped on %d; resampler rms %.2g worst %.2g, "
                  "matched filter rms %.2g worst %.2g, level rms %.2g worst %.2g" % (fs, seed, shared_math, len(r), gmin, clamped, *e))
            worst = np.maximum(worst, e)
    finally:
        oracle.set_variant()
    for v, meas in zip(worst, MEASURED[fs]):
        assert v <= gate(meas), (fs, worst, MEASURED[fs])
