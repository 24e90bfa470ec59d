"""GPU tests: the device's symbol-timing loop, carrier loop, equaliser, slicer and framer (demod_core.h: the three-wave pipeline with the
tree sums, the hardware sin / cos and the nearest-point slicer) against the float64 model of tests/demod_loops_f64.py, symbol by symbol.

Three streams of three channels each (demod_loops_f64.STREAMS: every arity acquired and tracked; a two-path channel with a clock offset;
a cut-off burst, a carrier swept past the runaway limit, then a clean burst) go through hfdl_gpu_frontend_push_baseband; after every
launch the matched-filter output, the AGC level and the symbols are read back.  The model runs on the loop tables read back from the
DEVICE (bit for bit the host design's, which tests/test_demod_loops_f64_cpu.py holds to a float64 design) and is fed the device's own
matched-filter and level taps, cut as the launches were, in both its forms (all float64; rate register in fp32).  Per channel:

  symbols      relative RMS and worst element / RMS, e_gpu <= 4 max(e_oracle, floor) against either form: e_oracle the oracle's error
               against the same model on the same stream, floor the figures of oracle/PINNING.md section 5 (MEASURED in the CPU file)
  counts       the total exact; every launch's against the form with the fp32 rate register, but for launches the model decided within
               rounding, at most 1 % of them
  counters     a1 / a2 / m1 found, m1 not found, frames, training bits total and bad: the model's
  frequency    every frame's freq_err_hz within the section 5 gate
  PDUs         what was sent, and what the oracle decodes

Cuts: launches as long as a call takes; the repeating pattern 0, 1, 5, 12, 13, 14, 1, 1, 40 input samples.  The strict build with every
fast form on (build/strict/libhfdl_gpu_strict_15.so) must give the shipped build's taps, PDUs and statistics word for word, and with
them its figures.  Afterwards the statistics are finite and a clean burst appended to channel 0 decodes."""
import ctypes as C
import math
import os
import subprocess
import time

import numpy as np
import pytest

import demod_loops_f64 as M
import test_demod_loops_f64_cpu as T
from dumphfdl_amd import frontend as F
from test_constants_cpu import DemodTables, HfdlConstants
from test_demod_front_f64_cpu import gate
from test_gpu_demod_front_f64 import burst_tail
from test_host_logic_cpu import build_sim

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS, CF = T.FS, T.CF
FREQS = [9_979_000, 10_003_000, 10_030_000]
LOOP_FIELDS = ("ss_mf", "ss_dmf", "eq_h0")


@pytest.fixture(scope="module")
def sim():
    H = build_sim("libhostsim.so", [])
    H.sim_tables.argtypes = [C.c_float, C.c_void_p]
    return H


@pytest.fixture(scope="module")
def tables(gpu, sim):
    """The loop tables as the device holds them (laboratory build, the same sources), bit for bit the host design's."""
    lab = F.load_lab()
    fe = gpu.Frontend(FS, CF, FREQS, lib=lab)
    try:
        t, k = DemodTables(), HfdlConstants()
        F._check(lab.hfdl_gpu_lab_read_constants(fe._h, C.byref(t), C.sizeof(t), C.byref(k), C.sizeof(k)), lab)
        rate = float(fe.geometry.resamp_rate)
    finally:
        fe.close()
    assert rate == T.RATE
    host = DemodTables()
    sim.sim_tables(rate, C.byref(host))
    for f in LOOP_FIELDS:
        assert bytes(getattr(t, f)) == bytes(getattr(host, f)), f
    for f in ("lf_b0", "lf_a1", "ss_rate_adj"):
        assert np.float32(getattr(t, f)).tobytes() == np.float32(getattr(host, f)).tobytes(), f
    return T.loop_tables(t)


@pytest.fixture(scope="module", params=T.NAMES)
def case(request, oracle, tables):
    """Per stream: the three channels, what was sent, and per channel the oracle's PDUs and its error against both forms of the model."""
    name = request.param
    xs, bursts = T.stream(name)
    ora_tables = T.oracle_tables(oracle)
    e_ora, ora_pdus = [], []
    for c, x in enumerate(xs):
        models, got, counters, pdus = T.oracle_run(oracle, x, ora_tables)
        e_ora.append(T.check_side("stream %s channel %d oracle" % (name, c), models, got, counters, [p["freq_err_hz"] for p in pdus]))
        ora_pdus.append([(p["mode"], p["octets"]) for p in pdus])
    # the clean burst that follows channel 0's stream is one the oracle decodes there (seed 7's, behind stream B, it does not: a false A1
    # in the burst's prekey, a weak A2, no M1, and the real preamble has passed)
    tail, octets = burst_tail(T.RATE, seed=8)
    ch = oracle.Channel(FS, CF, CF, want_channelizer=False)
    both = np.concatenate([xs[0], tail])
    for i in range(0, len(both), T.BLOCK):
        ch.process_baseband(both[i:i + T.BLOCK])
    assert [p["octets"][:len(octets)] for p in ch.pdus][len(bursts[0]):] == [octets]
    ch.close()
    return dict(name=name, xs=xs, bursts=bursts, e_ora=e_ora, ora_pdus=ora_pdus, tail=tail, octets=octets)


def whole(block):
    return lambda i, left: [min(block, v) for v in left]


def pattern(block):
    return lambda i, left: [min(T.PATTERN[i % len(T.PATTERN)], v) for v in left]


CUTS = dict(whole=whole, pattern=pattern)


def drive(fe, streams, cut):
    """Pushes the streams launch by launch; returns per channel the (matched-filter, level, symbols) taps of every launch, and the PDUs."""
    n = len(streams)
    at = [0] * n
    taps = [[] for _ in range(n)]
    pdus = []
    i = 0
    while any(at[c] < len(streams[c]) for c in range(n)):
        take = cut(i, [len(streams[c]) - at[c] for c in range(n)])
        assert i < 20000
        fe.push_baseband([streams[c][at[c]:at[c] + take[c]] for c in range(n)])
        for c in range(n):
            at[c] += take[c]
            taps[c].append((fe.read_tap(F.TAP_MF_OUT, c), fe.read_tap(F.TAP_AGC_LEVEL, c), fe.read_tap(F.TAP_SYMBOLS, c)))
        i += 1
    pdus += fe.poll_pdus()
    return taps, pdus


def check_channel(tag, case, c, tables, taps, stats, pdus):
    name = case["name"]
    models = T.Models(tables)
    got = []
    for mf, lvl, sym in taps:
        assert len(mf) == len(lvl)
        models.push(mf, lvl)
        got.append(sym.astype(np.complex128))
    mine = sorted((p for p in pdus if p["channel"] == c), key=lambda p: p["sample_index"])
    counters = {k: int(stats[k]) for k in M.COUNTERS}
    e_gpu = T.check_side(tag, models, got, counters, [p["freq_err_hz"] for p in mine])
    for form in ("f64", "r32"):
        e_o, floor = case["e_ora"][c][form], T.MEASURED[name][form]
        print("  [%s] device rms %.3g worst %.3g frequency %.3g Hz | oracle %.3g %.3g %.3g | floor %.3g %.3g %.3g" % (form, *e_gpu[form], *e_o, *floor))
        for i in range(2):
            assert e_gpu[form][i] <= 4 * max(e_o[i], floor[i]), (tag, form, "symbols", e_gpu[form], e_o, floor)
        assert e_gpu[form][2] <= gate(floor[2]), (tag, form, "frequency error", e_gpu[form][2], floor[2])
    sent = T.sent(case["bursts"][c])
    assert [(p["mode"], p["octets"][:len(o)]) for p, (_, o) in zip(mine, sent)] == sent and len(mine) == len(sent), (tag, "PDUs against what was sent")
    assert [(p["mode"], p["octets"]) for p in mine] == case["ora_pdus"][c], (tag, "PDUs against the oracle's")


@pytest.mark.parametrize("cut", list(CUTS))
def test_loops_against_the_float64_model(gpu, case, tables, cut):
    fe = gpu.Frontend(FS, CF, FREQS)
    try:
        g = fe.geometry
        assert float(g.resamp_rate) == T.RATE and g.channels == 3
        block = g.max_outputs_per_block
        t0 = time.time()
        taps, pdus = drive(fe, case["xs"], CUTS[cut](block))
        t1 = time.time()
        stats = fe.all_channel_stats()
        if cut == "pattern":
            outs = [len(t[0]) for t in taps[0]]
            assert 0 in outs and len(outs) > 1000
        for c in range(3):
            check_channel("stream %s %s channel %d" % (case["name"], cut, c), case, c, tables, taps[c], stats[c], pdus)
        print("stream %s %s: %d launches driven in %.1f s, checked in %.1f s" % (case["name"], cut, len(taps[0]), t1 - t0, time.time() - t1))
        # afterwards: nothing is poisoned, and a clean burst on channel 0 decodes
        tail, octets = case["tail"], case["octets"]
        quiet = np.zeros(0, np.complex64)
        for i in range(0, len(tail), block):
            fe.push_baseband([tail[i:i + block], quiet, quiet])
        after = fe.poll_pdus()
        assert [(p["channel"], p["octets"][:len(octets)]) for p in after] == [(0, octets)]
        for st in fe.all_channel_stats():
            assert all(math.isfinite(v) for v in st.values()), st
    finally:
        fe.close()


@pytest.fixture(scope="module")
def strict(gpu):
    """The strict build of this tree with the four fast forms on, loaded beside the product library."""
    lib = os.path.join(ROOT, "build", "strict", "libhfdl_gpu_strict_15.so")
    product = os.path.join(ROOT, "dumphfdl_amd", "libhfdl_gpu.so")
    if not (os.path.exists(lib) and os.path.getmtime(lib) >= os.path.getmtime(product)):
        subprocess.check_call(["bash", os.path.join(ROOT, "dumphfdl_amd", "csrc", "build_strict.sh"), "15"], stdout=subprocess.DEVNULL)
    return F._bind(C.CDLL(lib, mode=C.RTLD_LOCAL))


def words(v):
    return np.ascontiguousarray(v).view(np.uint32)


def test_the_strict_build_with_every_fast_form_gives_the_same_figures(gpu, strict, case):
    """The serial loop with the emulated fast forms against the three-wave pipeline on the same streams: the taps the figures are made
    of, the PDUs and the statistics are the same 32-bit words, so every figure of the comparison above is the shipped build's exactly."""
    runs = []
    for lib in (None, strict):
        fe = gpu.Frontend(FS, CF, FREQS, lib=lib)
        try:
            taps, pdus = drive(fe, case["xs"], whole(fe.geometry.max_outputs_per_block))
            stats = fe.all_channel_stats()
        finally:
            fe.close()
        key = lambda v: int(words(np.float32(v))[0]) if isinstance(v, float) else v
        # frames that end in one launch (stream B's channels 0 and 2: same start, same length) claim their PDU slots in the order their
        # workgroups get there, so the ring's order is not a figure of either build: every PDU is compared, by channel and sample index
        pdus = sorted(pdus, key=lambda p: (p["channel"], p["sample_index"]))
        runs.append((taps, [{k: key(v) for k, v in p.items()} for p in pdus], [{k: key(v) for k, v in s.items()} for s in stats]))
    (ta, pa, sa), (tb, pb, sb) = runs
    for c in range(3):
        assert len(ta[c]) == len(tb[c])
        for i, (la, lb) in enumerate(zip(ta[c], tb[c])):
            for k, (a, b) in enumerate(zip(la, lb)):
                assert np.array_equal(words(a), words(b)), "stream %s channel %d launch %d tap %d differs" % (case["name"], c, i, k)
    assert pa == pb and sa == sb
