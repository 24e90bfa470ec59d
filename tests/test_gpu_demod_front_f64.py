"""GPU tests: the device's resampler, AGC and matched filter (demod_core.h resample_outputs, agc_mf_chunk and demod_block's hand-over
code) against the float64 model of tests/demod_f64.py, sample by sample, under launch cuts that take every hand-over branch.

Three channels, each with a stream of its own (demod_f64.edge_stream: burst on noise, exact zeros that drive the gain into its 1e6 clamp,
an onset, a tone 40 dB up in the resampler's transition band), pushed through hfdl_gpu_frontend_push_baseband; the taps of every launch
are read back.  The model runs on the fp32 tables read back from the DEVICE (which equal the host design bit for bit; the design itself is
checked in tests/test_demod_front_f64_cpu.py), so the rounding bounds are exact statements about the kernel:

  resampler       |dev - model| <= 1.01 * 15 * 2^-24 * sum_j |h_j| |x_{i-j}| + 2^-126 per real component: the forward error bound of a
                  14-term fp32 sum in any order, with or without FMA contraction.  Every sample; every launch's output count.
  matched filter  the AGC output the device used is rebuilt from its own taps, y_k = resampled[k] * (1 / level[k - 1]) (g = 1 before the
                  stream), and |dev - model| <= 1.01 * (20 + 4) * 2^-24 * sum_t |mf_t| |y_{k-t}| + 2^-126: 19 terms, and the reciprocal
                  the device took (1 ulp), the model's inversion of it, and the product x g.  Every sample.
  AGC             the model's recurrence fed the device's own resampled tap; level by relative RMS and worst sample,
                  e_gpu <= 4 * max(e_oracle, floor) -- the rule of tests/test_gpu_channelizer_f64.py -- with e_oracle the oracle's error
                  against the model on the same stream and floor the figures of oracle/PINNING.md section 4.

Cuts: launches as long as a call takes; the repeating pattern 0, 1, 5, 12, 13, 14, 1, 1, 40 input samples (n_in < 13: the new resampler
history reaches into the old one; n_out < 18: so does the matched filter's; n_out == 0: the early return); unequal counts in one call
(a full block, five samples, none, the roles rotating over the channels).  After every run the channel statistics are finite and a
clean single-slot burst appended to channel 0 decodes."""
import ctypes as C
import math

import numpy as np
import pytest

import demod_f64 as M
import hfdl_synth as synth
from dumphfdl_amd import frontend as F
from test_constants_cpu import DemodTables, HfdlConstants
from test_demod_front_f64_cpu import MEASURED, SEEDS, STREAM_FS, build_sim, edge_condition

pytestmark = pytest.mark.gpu

CF = 10_000_000
FREQS = [9_979_000, 10_003_000, 10_030_000]
U = 2.0 ** -24
TINY = 2.0 ** -126
PATTERN = [0, 1, 5, 12, 13, 14, 1, 1, 40]


@pytest.fixture(scope="module")
def sim():
    H = build_sim("libhostsim.so", [])
    H.sim_tables.argtypes = [C.c_float, C.c_void_p]
    return H


def device_tables(gpu, sim, fs):
    """rs_h, rs_step, mf as the device holds them (laboratory build, the same sources), bit for bit the host design's."""
    lab = F.load_lab()
    fe = gpu.Frontend(fs, CF, FREQS, lib=lab)
    try:
        t, k = DemodTables(), HfdlConstants()
        F._check(lab.hfdl_gpu_lab_read_constants(fe._h, C.byref(t), C.sizeof(t), C.byref(k), C.sizeof(k)), lab)
        rate = float(fe.geometry.resamp_rate)
    finally:
        fe.close()
    host = DemodTables()
    sim.sim_tables(rate, C.byref(host))
    assert bytes(t.rs_h) == bytes(host.rs_h) and t.rs_step == host.rs_step and bytes(t.mf) == bytes(host.mf)
    assert t.rs_step == int(round(float(1 << 24) / rate))
    return rate, (np.frombuffer(t.rs_h, np.float32).copy(), int(t.rs_step), np.frombuffer(t.mf, np.float32).copy())


def burst_tail(rate, seed=7):
    """Three seconds of channelizer output holding one clean 300 bps single-slot burst, and its octets."""
    rng = np.random.default_rng(seed)
    octets = synth.make_pdu(rng, 0)
    fs_in = 5400.0 / rate
    x = synth.synth_channel_baseband(fs_in, int(3.0 * fs_in), [dict(mode=0, octets=octets, t0=0.4, amp=0.1, cfo=5.0)], noise_sigma=0.003, seed=seed)
    return x, octets


def whole(block, n):
    """launches as long as a call takes, the same for every channel"""
    return lambda i, left: [min(block, v) for v in left]


def pattern(block, n):
    return lambda i, left: [min(PATTERN[i % len(PATTERN)], v) for v in left]


def unequal(block, n):
    return lambda i, left: [min((block, 5, 0)[(c + i) % 3], left[c]) for c in range(n)]


CUTS = dict(whole=whole, pattern=pattern, unequal=unequal)


def drive(fe, streams, cut):
    """Pushes the streams launch by launch, cut(i, samples left per channel) -> samples per channel of launch i; returns per channel the
    input counts of its launches and their resampled / level / matched-filter taps."""
    n = len(streams)
    at = [0] * n
    counts, taps = [[] for _ in range(n)], [[] for _ in range(n)]
    i = 0
    while any(at[c] < len(streams[c]) for c in range(n)):
        take = cut(i, [len(streams[c]) - at[c] for c in range(n)])
        assert i < 20000
        fe.push_baseband([streams[c][at[c]:at[c] + take[c]] for c in range(n)])
        for c in range(n):
            at[c] += take[c]
            counts[c].append(take[c])
            taps[c].append((fe.read_tap(F.TAP_RESAMPLED, c), fe.read_tap(F.TAP_AGC_LEVEL, c), fe.read_tap(F.TAP_MF_OUT, c)))
        i += 1
    return counts, taps


def check_channel(tag, tables, x, counts, taps, e_ora, floor, level_from=0):
    """One channel of one run against the model, cut identically.  Returns the measured figures."""
    m = M.DemodFrontF64(tables=tables)
    want_rs, mag_re, mag_im = [], [], []
    at = 0
    for n_in, (rs, lvl, mf) in zip(counts, taps):
        r = m.resample(x[at:at + n_in].astype(np.complex128))
        at += n_in
        assert len(rs) == len(lvl) == len(mf) == len(r), (tag, "output count of a launch", n_in, len(rs), len(r))
        want_rs.append(r); mag_re.append(m.rs_mag[0]); mag_im.append(m.rs_mag[1])
    want_rs, mag_re, mag_im = map(np.concatenate, (want_rs, mag_re, mag_im))
    rs = np.concatenate([t[0] for t in taps]).astype(np.complex128)
    lvl = np.concatenate([t[1] for t in taps]).astype(np.float64)
    mf = np.concatenate([t[2] for t in taps]).astype(np.complex128)
    # --- resampler: every sample, per real component
    b_re, b_im = 1.01 * 15 * U * mag_re + TINY, 1.01 * 15 * U * mag_im + TINY
    q_rs = max(float((np.abs(rs.real - want_rs.real) / b_re).max()), float((np.abs(rs.imag - want_rs.imag) / b_im).max()))
    # --- matched filter on the AGC output the device used, rebuilt from its own taps
    g_used = np.concatenate([[1.0], 1.0 / lvl[:-1]])
    want_mf, f_re, f_im, _ = M.fir(tables[2].astype(np.float64), rs * g_used, np.zeros(M.MF_TAPS - 1, np.complex128))
    q_mf = max(float((np.abs(mf.real - want_mf.real) / (1.01 * 24 * U * f_re + TINY)).max()),
               float((np.abs(mf.imag - want_mf.imag) / (1.01 * 24 * U * f_im + TINY)).max()))
    # --- AGC: the model's recurrence on the device's own resampled tap
    _, want_lvl = M.DemodFrontF64(tables=tables).agc(rs)
    e_gpu = M.level_errors(lvl[level_from:], want_lvl[level_from:])
    print("%s: %d launches, %d outputs | resampler worst error / bound %.3f | matched filter %.3f | level rms %.3g worst %.3g (oracle %.3g %.3g)"
          % (tag, len(counts), len(rs), q_rs, q_mf, e_gpu[0], e_gpu[1], e_ora[0], e_ora[1]))
    assert q_rs <= 1.0, (tag, "resampler", q_rs)
    assert q_mf <= 1.0, (tag, "matched filter", q_mf)
    for i in range(2):
        assert e_gpu[i] <= 4 * max(e_ora[i], floor[i]), (tag, "AGC level", e_gpu, e_ora, floor)
    return q_rs, q_mf, e_gpu


def oracle_level(oracle, fs, x, block=900):
    ch = oracle.Channel(fs, CF, CF, want_channelizer=False)
    L = []
    for i in range(0, len(x), block):
        ch.process_baseband(x[i:i + block])
        L.append(ch.view()["agc_level"])
    pdus = [p["octets"] for p in ch.pdus]
    ch.close()
    return np.concatenate(L).astype(np.float64), pdus


@pytest.fixture(scope="module", params=STREAM_FS)
def case(request, gpu, oracle, sim):
    """Per sample rate: the device's tables, the three streams, the condition on them, and the oracle's level error against the model."""
    fs = request.param
    rate, tables = device_tables(gpu, sim, fs)
    streams = [M.edge_stream(seed, rate) for seed in SEEDS]
    e_ora = []
    for x in streams:
        m = M.DemodFrontF64(tables=tables)
        _, _, lvl, _ = m.push(x)
        edge_condition(m)
        e_ora.append(M.level_errors(oracle_level(oracle, fs, x)[0], lvl))
    tail, octets = burst_tail(rate)
    # the burst behind the stream is one the oracle decodes
    assert [o[:len(octets)] for o in oracle_level(oracle, fs, np.concatenate([streams[0], tail]))[1]] == [octets]
    return dict(fs=fs, rate=rate, tables=tables, streams=streams, e_ora=e_ora, tail=tail, octets=octets)


@pytest.mark.parametrize("cut", list(CUTS))
def test_front_against_the_float64_model(gpu, case, cut):
    fe = gpu.Frontend(case["fs"], CF, FREQS)
    try:
        g = fe.geometry
        assert float(g.resamp_rate) == case["rate"] and g.channels == 3
        block = g.max_outputs_per_block
        counts, taps = drive(fe, case["streams"], CUTS[cut](block, 3))
        if cut == "pattern":
            outs = [len(t[0]) for t in taps[0]]
            assert 0 in outs and min(v for v in outs if v) < M.MF_TAPS - 1 and min(v for v in counts[0] if v) < M.RS_TAPS - 1
        for c in range(3):
            check_channel("fs %d %s channel %d" % (case["fs"], cut, c), case["tables"], case["streams"][c], counts[c], taps[c],
                          case["e_ora"][c], MEASURED[case["fs"]][4:6])
        # afterwards: nothing is poisoned, and a clean burst on channel 0 decodes
        fe.poll_pdus()
        tail = case["tail"]
        quiet = np.zeros(0, np.complex64)
        for i in range(0, len(tail), block):
            fe.push_baseband([tail[i:i + block], quiet, quiet])
        pdus = fe.poll_pdus()
        assert [(p["channel"], p["octets"][:len(case["octets"])]) for p in pdus] == [(0, case["octets"])]
        for st in fe.all_channel_stats():
            assert all(math.isfinite(v) for v in st.values()), st
    finally:
        fe.close()


def test_the_gain_below_fp32_normal_range(gpu, oracle, sim):
    """An onset of amplitude 0.2 out of exact zeros (gain in its 1e6 clamp) drives the model's gain to 1.7e-41, through fp32's subnormals.
    What the oracle does there (oracle/PINNING.md section 4): its level overflows for some hundred samples and is finite again, the gain
    then freezes far below the signal (y2 has fallen under 1e-6 before the gain is back) and the later burst is NOT decoded.  The device
    must give the same verdict, and from 2000 samples after the minimum its level meets the AGC gate again."""
    fs = STREAM_FS[0]
    rate, tables = device_tables(gpu, sim, fs)
    tail, octets = burst_tail(rate)
    x = np.concatenate([M.edge_stream(21, rate, onset=0.2, tone=False), tail])
    m = M.DemodFrontF64(tables=tables)
    _, _, lvl, _ = m.push(x)
    gmin, kmin = float(np.min(m.g_trace)), int(np.argmin(m.g_trace))
    assert 1e-44 <= gmin <= 1e-39 and kmin + 2000 < len(lvl) - 4000
    L, ora_pdus = oracle_level(oracle, fs, x)
    ora_finite = bool(np.isfinite(L[kmin + 2000:]).all())
    ora_decodes = [o[:len(octets)] for o in ora_pdus] == [octets]
    fe = gpu.Frontend(fs, CF, FREQS)
    try:
        block = fe.geometry.max_outputs_per_block
        counts, taps = drive(fe, [x, x[:0], x[:0]], whole(block, 3))
        pdus = fe.poll_pdus()
        dev = np.concatenate([t[1] for t in taps[0]]).astype(np.float64)
        dev_finite = bool(np.isfinite(dev[kmin + 2000:]).all())
        dev_decodes = [(p["channel"], p["octets"][:len(octets)]) for p in pdus] == [(0, octets)]
        print("model gain minimum %.3g at sample %d; level finite again / burst decoded: oracle %s %s, device %s %s; non-finite levels: oracle %d, device %d"
              % (gmin, kmin, ora_finite, ora_decodes, dev_finite, dev_decodes, int((~np.isfinite(L)).sum()), int((~np.isfinite(dev)).sum())))
        assert (dev_finite, dev_decodes) == (ora_finite, ora_decodes)
        assert len(pdus) == len(ora_pdus)
        if ora_finite:
            e_ora = M.level_errors(L[kmin + 2000:], lvl[kmin + 2000:])
            rs = np.concatenate([t[0] for t in taps[0]]).astype(np.complex128)
            _, want = M.DemodFrontF64(tables=tables).agc(rs)
            e_gpu = M.level_errors(dev[kmin + 2000:], want[kmin + 2000:])
            print("level from 2000 samples after the minimum: device rms %.3g worst %.3g, oracle %.3g %.3g" % (*e_gpu, *e_ora))
            for i in range(2):
                assert e_gpu[i] <= 4 * max(e_ora[i], MEASURED[fs][4 + i]), (e_gpu, e_ora)
    finally:
        fe.close()
