"""CPU tests: the float64 model of the demodulator's back half (tests/demod_loops_f64.py: symbol-timing loop, carrier loop, equaliser,
slicer, sampler, framer) against the product's and the oracle's table designs, against an analytic property that comes from neither, and,
on three edge streams, against the oracle and against the product's serial loop (tests/hostsim) plain and with the SUM and SLICER fast
forms compiled in.  oracle/PINNING.md section 5 holds the measured figures behind every gate that is not derived.

What is compared.  The model is fed the tested side's own matched-filter output and AGC level, launch by launch, and must give the same
number of on-time symbols per launch, the same symbols (relative RMS over all of them; worst element over RMS), the same integer counters
and the same frequency error per frame.  These loops feed back through discrete decisions -- the branch round(16 tau), the slicer, the
runaway limit -- so symbols and launches that the model itself decided within rounding (`decided_within_rounding`) are left out of the
worst-element and per-launch-count comparisons (never of the RMS, the total count, the counters, the PDUs), and may be at most 1 %.

Two forms of the model (demod_loops_f64's docstring, "The rate register"): all float64 ("f64"), against which every fp32 side stands
1e-2 .. 1e-1 branch off in tau and so differs by 1e-2 in the symbols; and with the timing loop's rate register, and nothing else, rounded
to fp32 ("r32"), which an fp32 side follows to 1e-6.  Every side is held to both, each with the gates measured for it; the count of every
launch is asserted against r32, where `decided within rounding` means what it says."""
import ctypes as C
import math

import numpy as np
import pytest

import demod_f64 as F
import demod_loops_f64 as M
import hfdl_synth as synth
from test_constants_cpu import DemodTables
from test_demod_front_f64_cpu import gate
from test_host_logic_cpu import FrameRec, build_sim

FS, CF = 250_000, 10_000_000
RATE = float(np.float32(5400) / (np.float32(FS) / np.float32(32)))        # 0.6912
NAMES = ["A", "B", "C"]
BLOCK = 896                        # input samples per launch of the CPU comparisons

# Oracle tables against the float64 design: worst |difference| / largest tap of the matched bank, the derivative bank and the equaliser's
# initial taps; relative difference of lf_b0, lf_a1, rate_adj.  (The derivative bank is a difference of fp32-rounded neighbours.)
TABLES_MEASURED = (5.0e-8, 1.1e-6, 2.7e-8, 1.6e-7, 1.2e-7, 4.8e-8)

# Oracle against the model, worst over the three channels of a stream and over libm / shared_math (oracle/PINNING.md section 5), for the
# all-float64 model ("f64") and for the model with the rate register in fp32 ("r32"):
# (symbols relative RMS, worst element / RMS, |frequency error difference| in Hz)
MEASURED = {
    "A": dict(f64=(6.8e-3, 6.1e-2, 4.1e-3), r32=(8.9e-7, 1.2e-5, 2.7e-6)),
    "B": dict(f64=(1.1e-2, 8.3e-2, 1.8e-3), r32=(2.0e-4, 9.0e-3, 1.4e-6)),
    "C": dict(f64=(6.6e-3, 7.2e-2, 8.1e-4), r32=(4.9e-4, 3.3e-2, 2.4e-6)),
}


# ---------------------------------------------------------------- tables

@pytest.fixture(scope="module")
def sim():
    H = build_sim("libhostsim.so", [])
    H.sim_tables.argtypes = [C.c_float, C.c_void_p]
    return H


def loop_tables(t):
    """A DemodTables image -> the model's tables."""
    return M.tables_from(np.frombuffer(t.ss_mf, np.float32), np.frombuffer(t.ss_dmf, np.float32), t.lf_b0, t.lf_a1, t.ss_rate_adj,
                         np.frombuffer(t.eq_h0, np.float32))


def product_tables(sim):
    t = DemodTables()
    sim.sim_tables(RATE, C.byref(t))
    return loop_tables(t)


def oracle_tables(oracle):
    mf, dmf, w = np.zeros(288, np.float32), np.zeros(288, np.float32), np.zeros(15, np.float32)
    L = oracle.lib()
    L.orc_symsync_filters(mf.ctypes.data, dmf.ctypes.data)
    L.orc_eq_initial_taps(w.ctypes.data)
    s = [C.c_float(0) for _ in range(3)]
    L.orc_symsync_loop_filter(*[C.byref(v) for v in s])
    return M.tables_from(mf, dmf, s[0].value, s[1].value, s[2].value, w)


def table_figures(t, d):
    big = lambda k: float(np.abs(t[k] - d[k]).max() / np.abs(d[k]).max())
    rel = lambda k: abs(t[k] / d[k] - 1.0)
    return big("ss_mf"), big("ss_dmf"), big("eq_h0"), rel("lf_b0"), rel("lf_a1"), rel("rate_adj")


def test_tables_against_the_float64_design(sim, oracle):
    d = M.design()
    e_ora, e_prod = table_figures(oracle_tables(oracle), d), table_figures(product_tables(sim), d)
    print("matched bank, derivative bank, equaliser taps (worst / largest tap), lf_b0, lf_a1, rate_adj (relative):")
    print("  oracle  " + " ".join("%.3g" % v for v in e_ora))
    print("  product " + " ".join("%.3g" % v for v in e_prod))
    for o, p, meas in zip(e_ora, e_prod, TABLES_MEASURED):
        assert o <= gate(meas) and p <= gate(meas), (e_ora, e_prod)
    # properties of the design itself: the derivative bank is odd about the prototype's centre where the matched bank is even, and it
    # is the matched bank's slope with a POSITIVE sign (later branch = later in the pulse): rising before the peak
    H = np.concatenate([d["ss_mf"].T.ravel(), [0.0]])
    dH = np.concatenate([d["ss_dmf"].T.ravel(), [0.0]])
    assert np.allclose(H[1:144], H[287:144:-1], atol=1e-12) and np.allclose(dH[1:144], -dH[287:144:-1], atol=1e-12)
    assert int(np.argmax(H)) == 144 and np.all(dH[100:144] > 0) and abs(np.abs(H * dH).max() - 0.06) < 1e-12
    assert abs(d["eq_h0"].argmax() - 7) == 0 and np.allclose(d["eq_h0"], d["eq_h0"][::-1])


# ---------------------------------------------------------------- an analytic property

def cascade_pulses(d, scale):
    """On a grid of 16 points per sample (48 per symbol), from the float64 design: the pulse a sent symbol of amplitude `scale` leaves at
    the matched bank's output, at the derivative bank's, and at the equaliser's (initial taps) -- transmit pulse * matched filter *
    branch prototype.  A branch sums every 16th point of the prototype against the samples; the full convolution over 16 taken here is
    that sum averaged over where the sample grid lies against the pulse."""
    k = np.arange(-6 * 48, 6 * 48 + 1)
    synth.set_tx_pulse("mf_table")
    try:
        tx = scale * synth.tx_pulse(k / 48.0)
    finally:
        synth.set_tx_pulse()
    mfk = np.zeros(18 * 16 + 1)
    mfk[::16] = F.matched_filter_taps()
    front = np.convolve(tx, mfk)
    pm = np.convolve(front, np.concatenate([d["ss_mf"].T.ravel(), [0.0]])) / 16.0
    pd = np.convolve(front, np.concatenate([d["ss_dmf"].T.ravel(), [0.0]])) / 16.0
    eq = np.zeros(14 * 24 + 1)                         # the equaliser's taps are one output = 1.5 samples apart
    eq[::24] = d["eq_h0"]
    return pm, pd, np.convolve(pm / 3.0, eq)


def test_a_clean_bpsk_pattern_settles_on_the_pulse_peak(sim):
    """Not from liquid's text.  A noiseless random BPSK pattern shaped with the receiver's own pulse, at unit power, zero carrier offset and
    a fixed timing offset that is no multiple of a branch (0.37 sample): a timing loop whose derivative bank, loop filter and on-time
    choice are right climbs to the peak of the pulse and stays there, and the equalised on-time symbols are then +-A with the sent signs.

    Tolerances from the bank's 1 / 16-sample quantisation.  In lock tau keeps to the two branches around the peak, so the timing error e
    is at most one branch.  With the cascade pulse p of cascade_pulses() the symbols are sum_m a_m p(e + 48 m): their modulus lies in
    [p(e) - I(e), p(e) + I(e)], I(e) = sum_{m != 0} |p(e + 48 m)|, for e in {-1, 0, 1} branches; every settled modulus and their median lie
    in the union [LO, HI] of those, so modulus / median lies in [LO / HI, HI / LO].  A loop that settles elsewhere -- with a flipped
    derivative bank half a symbol off, where the eye is shut -- leaves that band by far.  The timing error q = Re(conj(m) d) has the mean
    S(e) = sum_m pm(e + 48 m) pd(e + 48 m) over random data; the loop hunts between the two branches that bracket S = 0, so the mean of q
    lies between S at those two: |mean q| <= the largest step of S between adjacent branches around the peak, plus, over a window of N
    updates, two standard errors 2 sigma_q / sqrt(N) of the pattern's own self-noise in q."""
    rng = np.random.default_rng(9)
    nsym = 2600
    bits = rng.integers(0, 2, nsym)
    synth.set_tx_pulse("mf_table")
    try:
        x = synth.shape_burst((1.0 - 2.0 * bits).astype(np.complex64), 5400.0, (20 + 0.37) / 5400.0, nsym * 3 + 60)
    finally:
        synth.set_tx_pulse()
    scale = 1.0 / math.sqrt(np.mean(np.abs(x[200:-200]) ** 2))
    x = x * scale
    mf_out, _, _, _ = F.fir(F.matched_filter_taps(), x, np.zeros(F.MF_TAPS - 1, np.complex128))
    d = M.design()
    pm, pd, p = cascade_pulses(d, scale)
    c = int(np.argmax(np.abs(p)))
    band = []
    for e in (-1, 0, 1):
        isi = sum(abs(p[c + e + 48 * j]) for j in range(-12, 13) if j and 0 <= c + e + 48 * j < len(p))
        band.append((abs(p[c + e]) - isi, abs(p[c + e]) + isi))
    LO, HI = min(b[0] for b in band), max(b[1] for b in band)
    cm = int(np.argmax(np.abs(pm)))
    S = np.array([sum(pm[cm + e + 48 * j] * pd[cm + e + 48 * j] for j in range(-12, 13) if 0 <= cm + e + 48 * j < len(pm)) for e in range(-3, 4)])
    q_step = float(np.abs(np.diff(S)).max())
    print("design: eye [%.4f, %.4f] of a peak of %.4f; S over -3 .. 3 branches %s" % (LO, HI, abs(p[c]), ["%.4f" % v for v in S]))
    assert LO / HI > 0.5, "the design's own eye is open (half a symbol off LO is negative: the band then excludes nothing)"
    assert S[0] > 0 > S[-1] or S[0] < 0 < S[-1], "the timing error changes sign at the pulse's peak"
    for tables in (None, product_tables(sim)):
        m = M.DemodLoopsF64(tables)
        s = m.push(mf_out, np.ones(len(mf_out)))
        assert m.cnt["a1_found"] == 0 and m.resets_runaway == 0          # the pattern is no preamble: nothing ever resets the loops
        settled = np.abs(s[1200:2400])
        amp = float(np.median(settled))
        q = np.array(m.q_trace[1200:2400])
        print("tables %s: settled modulus / median in [%.4f, %.4f], band [%.4f, %.4f]; mean q %.3g (mean |q| %.3g), bound %.3g; branches %s"
              % ("design" if tables is None else "product", settled.min() / amp, settled.max() / amp, LO / HI, HI / LO, q.mean(), np.abs(q).mean(),
                 q_step, sorted(set(m.banks[2400:4800]))))
        assert LO / HI <= settled.min() / amp and settled.max() / amp <= HI / LO
        # decision points: the sent signs, at one fixed delay, through one polarity
        got = (s[1200:2400].real < 0).astype(int)
        agree = [float(np.mean(got == bits[1200 - dly:1200 - dly + len(got)])) for dly in range(40)]
        assert max(max(agree), 1.0 - min(agree)) == 1.0, "every settled decision is a sent bit"
        # tau keeps to two adjacent branches for each of the two outputs of a symbol
        assert len(set(m.banks[2400:4800])) <= 4
        assert abs(q.mean()) <= q_step + 2.0 * q.std() / math.sqrt(len(q))


# ---------------------------------------------------------------- the edge streams and their conditions

_streams = {}


def stream(name):
    if name not in _streams:
        _streams[name] = M.STREAMS[name](synth)
    return _streams[name]


PATTERN = [0, 1, 5, 12, 13, 14, 1, 1, 40]          # input samples per launch: the small-launch cut of the GPU tests


def shares(m, counts):
    """(per symbol, per launch, share of symbols, share of launches) the model decided within rounding; a launch counts when its last
    sample is such a sample."""
    sym, smp = m.decided_within_rounding()
    last = np.cumsum(counts) - 1
    launch = np.array([bool(smp[i]) if n else False for i, n in zip(last, counts)])
    return sym, launch, float(sym.mean()), float(launch.mean())


@pytest.mark.parametrize("name", NAMES)
def test_the_streams_do_what_they_are_for(name):
    """On the model alone -- the float64 front of tests/demod_f64.py and the float64 loops, both on their float64 designs -- before
    anything is compared."""
    xs, bursts = stream(name)
    for c, x in enumerate(xs):
        assert len(x) <= 3.6 * M.FS_IN
        front = F.DemodFrontF64(rate=RATE)
        m = M.DemodLoopsF64()
        counts, at, i = [], 0, 0
        while at < len(x):                             # the small-launch cut: the one with enough launches for a share of them to mean something
            n = PATTERN[i % len(PATTERN)]
            _, _, lvl, mf = front.push(x[at:at + n])
            m.push(mf, lvl)
            counts.append(len(mf))
            at, i = at + n, i + 1
        _, _, s_sym, s_launch = shares(m, counts)
        print("stream %s channel %d: %d symbols, decided within rounding: %.2f %% of the symbols, %.2f %% of the launches; counters %s; resets: "
              "runaway %d, failed search %d; |w - h0| up to %.2f; branches %d; outputs per sample %s; frequency errors %s"
              % (name, c, len(m.sym_margin), 100 * s_sym, 100 * s_launch, m.cnt, m.resets_runaway, m.resets_failed_search, max(m.w_dist),
                 len(set(m.banks)), sorted(set(m.outputs)), ["%.2f" % v for v in m.freq_err]))
        assert s_sym <= 0.01 and s_launch <= 0.01
        assert m.cnt["frames"] == 1 and m.frames[0]["mode"] == bursts[c][0]["mode"], "the burst is framed"
        # every branch; samples with no output and with one.  (Two outputs in one sample cannot happen with k = 3, k_out = 2: an output
        # advances tau by del = rate + q_hat >= 1.5 - 0.037 - the rate's drift, |q_hat| <= b0 / (1 + a1) = 0.037 at |q| <= 1, so after
        # one output tau >= 1 and the loop ends.  Asserted as such.)
        assert set(m.banks) == set(range(16)) and set(m.outputs) == {0, 1}
        if name == "A":
            assert [b[0]["mode"] for b in bursts] == [0, 2, 3] and min(b[0]["cfo"] for b in bursts) < 0 and bursts[2][0]["cfo"] >= 25.0
        if name == "B":
            assert max(m.w_dist) > 0.2, "the equaliser moved well away from its initial taps (their peak is 0.9)"
        if name == "C":
            assert m.resets_failed_search == (1 if c < 2 else 0) and m.resets_runaway == (0 if c == 1 else 1)
            assert m.cnt["a1_found"] == m.cnt["frames"] + m.resets_failed_search


# ---------------------------------------------------------------- a side against the model

class Models:
    """The two forms of the model side by side, fed the same taps: "f64" all float64, "r32" with the rate register in fp32
    (demod_loops_f64's docstring)."""

    def __init__(self, tables):
        self.m = dict(f64=M.DemodLoopsF64(tables), r32=M.DemodLoopsF64(tables, rate_fp32=True))
        self.want = dict(f64=[], r32=[])
        self.counts = []

    def push(self, mf_out, level):
        for k, m in self.m.items():
            self.want[k].append(m.push(mf_out, level))
        self.counts.append(len(mf_out))


def compare(tag, m, counts, got, want, per_launch):
    """got / want: the side's and the model's symbols per launch; counts: samples per launch.  Returns (relative RMS, worst / RMS)."""
    sym, launch, s_sym, s_launch = shares(m, counts)
    off = [i for i, (g, w) in enumerate(zip(got, want)) if len(g) != len(w)]
    bad = [i for i in off if not (launch[i] or (i > 0 and launch[i - 1]))]
    G, W = np.concatenate(got), np.concatenate(want)
    assert len(G) == len(W), (tag, "total symbol count", len(G), len(W))
    # what is left out: at most 1 % of the symbols; of the launches, those whose count was excused
    assert s_sym <= 0.01, (tag, s_sym)
    if per_launch:
        assert not bad, (tag, "symbol count of launches", bad[:8])
        assert len(off) <= 0.01 * len(counts), (tag, len(off), len(counts))
    rms = F.rel_rms(G, W)
    worst = float(np.abs(G - W)[~sym].max() / np.sqrt(np.mean(np.abs(W) ** 2)))
    print("%s: %d launches (%d counted apart, %d of them not within rounding), %d symbols, %.2f %% of them left out of the worst; symbols rms "
          "%.3g worst / rms %.3g" % (tag, len(counts), len(off), len(bad), len(W), 100 * s_sym, rms, worst))
    return rms, worst


def check_side(tag, models, got, counters, freq_err):
    """One channel of one side against both forms of the model.  Against the all-float64 form the symbols' figures, the total count, the
    counters and the frequency errors; against the form with the fp32 rate register the count of every launch as well (against the
    all-float64 form an fp32 side shifts a symbol across a launch boundary wherever tau is within its standing offset of branch 16,
    far outside `decided within rounding`: counted and printed, not asserted).  Returns {form: (rms, worst / rms, Hz)}."""
    out = {}
    for k in ("f64", "r32"):
        m = models.m[k]
        rms, worst = compare("%s [%s]" % (tag, k), m, models.counts, got, models.want[k], per_launch=(k == "r32"))
        assert counters == m.cnt, (tag, k, counters, m.cnt)
        assert len(freq_err) == len(m.frames)
        df = max([abs(a - f["freq_err_hz"]) for a, f in zip(freq_err, m.frames)] + [0.0])
        print("  frequency error per frame: side %s model %s" % (["%.5f" % v for v in freq_err], ["%.5f" % f["freq_err_hz"] for f in m.frames]))
        out[k] = (rms, worst, df)
    return out


def worse(a, b):
    return {k: tuple(np.maximum(a[k], b[k])) for k in b} if a else b


def assert_gates(tag, name, worst):
    for k in ("f64", "r32"):
        print("%s [%s]: rms %.3g worst / rms %.3g frequency %.3g Hz" % (tag, k, *worst[k]))
    for k in ("f64", "r32"):
        for v, meas in zip(worst[k], MEASURED[name][k]):
            assert v <= gate(meas), (tag, k, worst[k], MEASURED[name][k])


def oracle_run(oracle, x, tables, block=BLOCK):
    """The oracle's channel on baseband x, and both models on the oracle's own matched-filter and level taps."""
    ch = oracle.Channel(FS, CF, CF, want_channelizer=False)
    models = Models(tables)
    got = []
    for i in range(0, len(x), block):
        ch.process_baseband(x[i:i + block])
        v = ch.view()
        got.append(v["symbols"].astype(np.complex128))
        models.push(v["mf_out"], v["agc_level"])
    cnt = (C.c_uint32 * 4)()
    nf, st = C.c_float(0), C.c_int(0)
    oracle.lib().orc_channel_counters(ch.h, cnt, C.byref(nf), C.byref(st))
    s = ch.summary()
    counters = dict(a1_found=s["a1_found"], a2_found=s["a2_found"], m1_found=s["m1_found"], m1_not_found=s["m1_not_found"], frames=cnt[3],
                    train_bits_total=s["train_bits_total"], train_bits_bad=s["train_bits_bad"])
    pdus = list(ch.pdus)
    ch.close()
    return models, got, counters, pdus


def sent(bursts):
    return [(b["mode"], b["octets"]) for b in bursts]


@pytest.mark.parametrize("shared_math", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_oracle_against_the_model(oracle, name, shared_math):
    xs, bursts = stream(name)
    tables = oracle_tables(oracle)
    worst = None
    oracle.set_variant(shared_math=shared_math)
    try:
        for c, x in enumerate(xs):
            models, got, counters, pdus = oracle_run(oracle, x, tables)
            e = check_side("stream %s channel %d shared_math %d" % (name, c, shared_math), models, got, counters, [p["freq_err_hz"] for p in pdus])
            assert [(p["mode"], p["octets"][:len(b["octets"])]) for p, b in zip(pdus, bursts[c])] == sent(bursts[c]) and len(pdus) == len(bursts[c])
            worst = worse(worst, e)
    finally:
        oracle.set_variant()
    assert_gates("stream %s shared_math %d" % (name, shared_math), name, worst)


# ---------------------------------------------------------------- the product's serial loop, plain and with the fast forms a CPU can run

def serial_run(H, oracle, x, tables):
    """tests/hostsim's serial loop on baseband x and both models on its own taps."""
    s = H.sim_create(np.float32(RATE), 1024)
    models = Models(tables)
    frames = (FrameRec * 16)()
    syms = np.zeros((16, 5040), np.complex64)
    got, freq_err, pdus = [], [], []
    for i in range(0, len(x), BLOCK):
        blk = np.ascontiguousarray(x[i:i + BLOCK])
        nf = H.sim_block(s, blk.ctypes.data, len(blk), frames, syms.ctypes.data)
        rs, mf, sy = (np.zeros(1024, np.complex64) for _ in range(3))
        lv = np.zeros(1024, np.float32)
        cnt = (C.c_int * 2)()
        H.sim_taps(s, rs.ctypes.data, mf.ctypes.data, sy.ctypes.data, lv.ctypes.data, cnt)
        got.append(sy[:cnt[1]].astype(np.complex128))
        models.push(mf[:cnt[0]], lv[:cnt[0]])
        for k in range(nf):
            f = frames[k]
            freq_err.append(float(f.freq_err_hz))
            pdus.append((f.mode, bytes(oracle.decode_user_data(f.mode, syms[k][:synth.mode_sizes(f.mode)["nsym"]], f.bitmask_lsb))))
    c = (C.c_uint32 * 7)()
    H.sim_counters(C.c_void_p(s), c)
    H.sim_destroy(s)
    return models, got, dict(zip(M.COUNTERS, c)), freq_err, pdus


@pytest.fixture(scope="module", params=[0, 1, 8, 9])
def serial(request):
    """fast forms compiled in: none; SUM (the balanced-tree sums with taps t and t + 16 in one lane); SLICER (nearest point); both"""
    fast = request.param
    H = build_sim("libhostsim_fast%d.so" % fast, ["-DHFDL_DM_STRICT_FAST=%d" % fast])
    H.sim_tables.argtypes = [C.c_float, C.c_void_p]
    H.sim_counters.argtypes = [C.c_void_p, C.c_void_p]
    return fast, H


@pytest.mark.parametrize("name", NAMES)
def test_serial_loop_against_the_model(serial, oracle, name):
    fast, H = serial
    xs, bursts = stream(name)
    tables = product_tables(H)
    worst = None
    for c, x in enumerate(xs):
        models, got, counters, freq_err, pdus = serial_run(H, oracle, x, tables)
        e = check_side("stream %s channel %d fast forms %d" % (name, c, fast), models, got, counters, freq_err)
        assert [(p[0], p[1][:len(b["octets"])]) for p, b in zip(pdus, bursts[c])] == sent(bursts[c]) and len(pdus) == len(bursts[c])
        worst = worse(worst, e)
    assert_gates("stream %s fast forms %d" % (name, fast), name, worst)


# ---------------------------------------------------------------- the slicer where two points are equally near

def exact_slice(arity, re, im):
    """The reference ladder in exact arithmetic at points of the form (+-a, +-a), (+-a, 0), (0, +-a): arg s is a multiple of pi / 4 and
    every ladder value a multiple of pi / 8, held here as an integer number of pi / 8.  Returns the linear index."""
    eighth = {(1, 0): 0, (1, 1): 2, (0, 1): 4, (-1, 1): 6, (-1, 0): 8, (-1, -1): -6, (0, -1): -4, (1, -1): -2}[(int(np.sign(re)), int(np.sign(im)))]
    M_ = 1 << arity
    v = eighth - 8 * (M_ - 1) // M_
    if v < -8:
        v += 16
    idx = 0
    for k in range(arity - 1, -1, -1):
        ref = (1 << k) * 8 // M_
        idx <<= 1
        if v > 0:
            idx |= 1
            v -= ref
        else:
            v += ref
    return idx


def test_the_nearest_point_slicer_at_exact_ties(sim):
    """The fast build's slicer takes the point with the largest Re(x conj p).  On a decision boundary two points tie; the reference's
    ladder decides `v > 0`, so the boundary belongs to the LOWER index (and the boundary between the last point and point 0 to point 0).
    QPSK's boundaries are the diagonals, which fp32 holds exactly: there the nearest-point form must give the ladder's answer in exact
    arithmetic, and the phase error that goes with it.  (8-PSK's boundaries are no fp32 numbers; its constellation points and the
    diagonals' neighbours are decided alike by both forms, checked too.  The float64 model's own slicer is checked against the same
    exact ladder one ulp to either side of every boundary.)"""
    sim.sim_slice.restype = C.c_uint32
    sim.sim_slice.argtypes = [C.c_int, C.c_float, C.c_float, C.c_int, C.POINTER(C.c_float)]
    pe = C.c_float(0)
    for a in (0.5, 0.7071067690849304, 1.0, 3.0):
        for sr, si in ((1, 1), (-1, 1), (-1, -1), (1, -1)):
            idx = exact_slice(2, sr, si)
            got = sim.sim_slice(2, sr * a, si * a, 1, C.byref(pe))
            ang = idx * math.pi / 2
            want_pe = (complex(sr * a, si * a) * complex(math.cos(ang), -math.sin(ang))).imag
            assert got == idx ^ (idx >> 1), ("QPSK tie", sr, si, got, idx)
            assert abs(pe.value - want_pe) <= 1e-6 * a, ("QPSK tie phase error", sr, si, pe.value, want_pe)
    # away from ties both forms and the model agree: every constellation point of both arities, and one part in a thousand off each diagonal
    for arity in (2, 3):
        n = 1 << arity
        for k in range(n):
            for dev in ((0.0,) if arity == 3 else (0.0, math.pi / 4 - 1e-3, math.pi / 4 + 1e-3)):
                z = 0.9 * complex(math.cos(2 * math.pi * k / n + dev), math.sin(2 * math.pi * k / n + dev))
                want, _, margin = M.psk_slice(arity, complex(np.complex64(z)))
                assert margin > 5e-4
                for nearest in (0, 1):
                    assert sim.sim_slice(arity, z.real, z.imag, nearest, C.byref(pe)) == want, (arity, k, dev, nearest)
    # the model's own ladder next to the boundaries
    for arity in (2, 3):
        n = 1 << arity
        for k in range(n):
            edge = 2 * math.pi * (k + 0.5) / n
            for dev, lin in ((-1e-9, k), (1e-9, (k + 1) % n)):
                sym, point, margin = M.psk_slice(arity, complex(math.cos(edge + dev), math.sin(edge + dev)))
                assert sym == lin ^ (lin >> 1) and abs(margin - 1e-9) < 1e-12 and abs(point - complex(math.cos(2 * math.pi * lin / n), math.sin(2 * math.pi * lin / n))) < 1e-12
