"""CPU tests of the product's host-side logic: the C ABI exports, the planner / tap design in the shim, and the
demodulator control logic (dumphfdl_amd/csrc/demod_core.h compiled for the host by tests/hostsim -- test harness only)."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest

import hfdl_synth as synth
import dumphfdl_amd as hf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_sim(name, flags):
    d = os.path.join(ROOT, "tests", "hostsim")
    so = os.path.join(d, name)
    # HOSTSIM_CXXFLAGS: e.g. "-fsanitize=address,undefined -g" (then run pytest with the sanitizer runtimes in LD_PRELOAD)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off"] + flags + os.environ.get("HOSTSIM_CXXFLAGS", "").split() +
                          ["-o", so, os.path.join(d, "hostsim.cpp")])
    H = C.CDLL(so)
    H.sim_create.restype = C.c_void_p
    H.sim_create.argtypes = [C.c_float, C.c_int]
    H.sim_destroy.argtypes = [C.c_void_p]
    H.sim_block.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    H.sim_taps.argtypes = [C.c_void_p] + [C.c_void_p] * 5
    H.sim_plan.argtypes = [C.c_float, C.c_int, C.c_float, C.c_void_p]
    H.sim_transition_bw.restype = C.c_float
    H.sim_bandpass.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float]
    H.sim_psk_soft.argtypes = [C.c_int, C.c_float, C.c_float, C.c_void_p]
    H.sim_sizeof_framerec.restype = C.c_size_t
    return H


@pytest.fixture(scope="module")
def sim():
    return build_sim("libhostsim.so", [])


@pytest.fixture(scope="module")
def sim_strict():
    """The serial loop on the fixed-sequence elementary functions (tests/hostsim/shared_math.h): what the device's test-only build
    -DHFDL_DM_STRICT runs, compiled for the host."""
    return build_sim("libhostsim_strict.so", ["-DHFDL_DM_STRICT"])


class FrameRec(C.Structure):
    _fields_ = [("channel", C.c_int32), ("slot", C.c_int32), ("mode", C.c_int32), ("bitmask_lsb", C.c_int32),
                ("freq_err_hz", C.c_float), ("signal_level", C.c_float), ("noise_floor", C.c_float),
                ("train_bad", C.c_int32), ("train_total", C.c_int32), ("pad", C.c_int32), ("sample_index", C.c_uint64)]


class Plan(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("pre", "post", "taps_min_length", "taps_length", "overlap", "n", "m", "input_size",
                                         "post_input_size", "scrap", "v", "startbin", "offsetbin")] + \
        [(n, C.c_float) for n in ("pre_shift", "post_shift", "sindelta", "cosdelta", "rate")]


def test_abi_exports_match_header():
    """libhfdl_gpu.so loads without a GPU and exports every symbol include/hfdl_gpu.h declares."""
    hdr = open(os.path.join(ROOT, "include", "hfdl_gpu.h")).read()
    declared = set(re.findall(r"\b(hfdl_gpu_[a-z0-9_]+)\s*\(", hdr))
    declared.discard("hfdl_gpu_frontend")
    L = hf.load()
    assert declared, "no declarations parsed"
    for name in sorted(declared):
        assert hasattr(L, name), name
    assert set(hf.frontend.EXPORTS) == declared


def test_product_library_exports_exactly_the_public_header():
    """`nm -D libhfdl_gpu.so`: the dynamic symbols named hfdl_gpu_* are EXACTLY the declarations of include/hfdl_gpu.h -- no probe, no
    tiling sweep, no laboratory entry point (those live in libhfdl_gpu_lab.so, include/hfdl_gpu_lab.h) -- the product library carries
    the kernels the front end can launch and nothing else (round 4's, with the 47-tiling sweep inside, was twice the size; half of
    what is left are the fifteen register-resident FFT passes: three radices x three sample formats of pass 1, three of pass 2 and 3)
    and reads no laboratory switch from the environment; the laboratory build exports the public header plus its own."""
    def dyn(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {l.split()[-1] for l in out.splitlines() if " T " in l and l.split()[-1].startswith("hfdl_gpu_")}
    pub = set(re.findall(r"\b(hfdl_gpu_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", "hfdl_gpu.h")).read())) - {"hfdl_gpu_frontend"}
    lab = set(re.findall(r"\b(hfdl_gpu_lab_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", "hfdl_gpu_lab.h")).read()))
    prod = dyn(hf.lib_path())
    assert prod == pub, (sorted(prod - pub), sorted(pub - prod))
    assert not [s for s in prod if "probe" in s or "variant" in s or "_lab_" in s]
    assert os.path.getsize(hf.lib_path()) < 800 * 1024        # (round 6: + the two thirty-two-column tilings and their left-over forms)
    strings = subprocess.run(["strings", hf.lib_path()], capture_output=True, text=True).stdout
    for knob in ("HFDL_GPU_FFT_STREAM", "HFDL_GPU_DECODE_STREAM", "HFDL_GPU_FOLD_TILE", "HFDL_GPU_FOLD_BOUND", "HFDL_GPU_PROBE_VERBOSE"):
        assert knob not in strings, knob
    for knob in ("HFDL_GPU_FOLD_BATCH", "HFDL_GPU_DEMOD_BATCH", "HFDL_GPU_HOST_THREADS", "HFDL_GPU_PDU_RING", "HFDL_GPU_FOLD_PRUNE"):      # the documented create-time configuration
        assert knob in strings, knob
    lab_path = hf.frontend.lab_lib_path()
    if os.path.exists(lab_path):
        assert dyn(lab_path) == pub | lab and set(hf.frontend.LAB_EXPORTS) == lab
    # and INTEGRATION.md names no entry point the header does not declare
    named = set(re.findall(r"\b(hfdl_gpu_[a-z0-9_]+)\b", open(os.path.join(ROOT, "INTEGRATION.md")).read()))
    named -= {"hfdl_gpu_frontend", "hfdl_gpu_geometry", "hfdl_gpu_pdu", "hfdl_gpu_channel_stats", "hfdl_gpu_lab"}
    assert not [n for n in named if n not in pub and n not in lab and not n.startswith("hfdl_gpu_lab")], sorted(named - pub - lab)


def test_no_cpu_fallback_without_device():
    if hf.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(hf.GpuError, match="no HIP device|no CPU fallback"):
        hf.Frontend(250000, 10_000_000, [10_010_000])
    with pytest.raises(hf.GpuError):
        hf.fft_forward(np.zeros(1024, np.complex64))
    with pytest.raises(hf.GpuError):
        hf.viterbi27(np.zeros((1, 1080), np.uint8), 540)


def test_product_does_not_touch_the_oracle():
    """The shipped package must never import, link or dlopen anything under oracle/ (or fall back to a CPU path)."""
    for dirpath, _, files in os.walk(os.path.join(ROOT, "dumphfdl_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h", ".c", ".sh")) or f == "Makefile":
                txt = open(os.path.join(dirpath, f), errors="replace").read()
                assert "pyoracle" not in txt and "liboracle" not in txt and "hfdl_oracle.h" not in txt, f
                assert not re.search(r"(from|import)\s+oracle\b", txt), f
    out = subprocess.run(["ldd", hf.lib_path()], capture_output=True, text=True).stdout
    assert "oracle" not in out


def test_hip_resources_are_released_by_their_owners_alone():
    """hip_handles.h: device memory, page-locked memory, events and streams are released by the destructors of their owning types
    (DevBuf in kernels.h, the others in hip_handles.h) and nowhere else under csrc/ -- hfdl_gpu_host_free() excepted, whose memory is
    the caller's.  No translation unit keeps a list of raw handles to free by hand: no release(), no untyped `void *priv`, and no
    D_TRY (a HIP error without text; HIP_TRY / CREATE_TRY name the call, and CREATE_TRY reports an allocation that does not fit as
    HFDL_GPU_ENOMEM).  The one `release()` in the sources is std::unique_ptr's, where create hands the finished front end to the
    caller of the C interface."""
    csrc = os.path.join(ROOT, "dumphfdl_amd", "csrc")
    calls = ("hipFree(", "hipHostFree(", "hipEventDestroy(", "hipStreamDestroy(")
    found = {}
    for f in sorted(os.listdir(csrc)):
        for ln in open(os.path.join(csrc, f), errors="replace").read().splitlines():
            for c in calls:
                if c in ln:
                    found.setdefault(f, set()).add(c)
            assert "void *priv" not in ln and "D_TRY" not in ln, (f, ln)
            if "release()" in ln:
                assert (f, ln.strip()) == ("frontend_create.cpp", "*out = fe.release();"), (f, ln)
    assert found.pop("kernels.h") == {"hipFree("}
    assert found.pop("hip_handles.h") == {"hipHostFree(", "hipEventDestroy(", "hipStreamDestroy("}
    assert found == {"frontend_query.cpp": {"hipHostFree("}}, found
    q = open(os.path.join(csrc, "frontend_query.cpp")).read()
    assert q.count("hipHostFree(") == 1 and "hipHostFree(" in q[q.index("hfdl_gpu_host_free("):].split("\n}\n")[0]


@pytest.mark.parametrize("fs,off", [(250000, 37000), (250000, -101500), (1000000, 412345), (8000000, -3163000), (40000000, 19081440)])
def test_planner_matches_oracle(sim, oracle, fs, off):
    dec, tbw, _ = oracle.geometry(fs)
    assert sim.sim_fft_decimation_rate(fs, 5400) == dec
    assert np.float32(sim.sim_transition_bw(fs, 250)) == np.float32(tbw)
    shift = float(np.float32(-(off + 1440)) / np.float32(fs))
    p = Plan()
    assert sim.sim_plan(tbw, dec, shift, C.byref(p)) == 0
    d = oracle.fastddc_init(tbw, dec, shift)
    assert (p.pre, p.post, p.taps_length, p.n, p.m, p.input_size, p.post_input_size, p.scrap, p.v, p.startbin, p.offsetbin) == \
        (d.pre_decimation, d.post_decimation, d.taps_length, d.fft_size, d.fft_inv_size, d.input_size, d.post_input_size,
         d.scrap, d.v, d.startbin, d.offsetbin)
    for a, b in ((p.post_shift, d.post_shift), (p.sindelta, d.nco_sindelta), (p.cosdelta, d.nco_cosdelta), (p.rate, d.nco_rate)):
        assert np.float32(a) == np.float32(b)


def test_tap_design_matches_oracle_bit_for_bit(sim, oracle):
    n = 4097
    a = np.zeros(n, np.complex64); b = np.zeros(n, np.complex64)
    lo, hi = np.float32(0.1234 - 1 / 64), np.float32(0.1234 + 1 / 64)
    sim.sim_bandpass(a.ctypes.data, n, float(lo), float(hi))
    oracle.lib().orc_firdes_bandpass_c(b.ctypes.data, n, float(lo), float(hi))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert abs(np.abs(np.sum(a * np.exp(-2j * np.pi * 0.1234 * np.arange(n)))) - 1.0) < 1e-4     # unity gain at band centre


def test_demod_tables_match_oracle(sim, oracle):
    class T(C.Structure):
        _fields_ = [("rs_h", C.c_float * (256 * 14)), ("rs_step", C.c_uint32), ("mf", C.c_float * 19),
                    ("ss_mf", C.c_float * 288), ("ss_dmf", C.c_float * 288), ("lf_b0", C.c_float), ("lf_a1", C.c_float),
                    ("ss_rate_adj", C.c_float), ("eq_h0", C.c_float * 15), ("a_hi", C.c_uint64), ("a_lo", C.c_uint64),
                    ("m1_hi", C.c_uint64 * 8), ("m1_lo", C.c_uint64 * 8), ("scrambler", C.c_uint8 * 120), ("scr_pad", C.c_uint8 * 8), ("psk_pts", C.c_float * 32),
                    ("corr_tab", C.c_float * 128), ("a1_lo", C.c_int32), ("a1_hi", C.c_int32), ("a2_lo", C.c_int32),
                    ("a2_hi", C.c_int32), ("pos_min", C.c_int32), ("thr_pad", C.c_int32)]
    sim.sim_sizeof_tables.restype = C.c_size_t
    assert sim.sim_sizeof_tables() == C.sizeof(T)
    for rate in (0.6912, 0.55296):
        t = T()
        sim.sim_tables.argtypes = [C.c_float, C.c_void_p]
        sim.sim_tables(rate, C.byref(t))
        h = np.zeros(256 * 14, np.float32); step = C.c_uint32(0)
        oracle.lib().orc_resamp_filter(rate, h.ctypes.data, C.byref(step))
        assert step.value == t.rs_step and np.array_equal(np.frombuffer(t.rs_h, np.float32), h)
        assert abs(h.reshape(256, 14).sum(axis=1) - 1).max() < 2e-3        # every polyphase branch ~ unity DC gain
    mf = np.zeros(288, np.float32); dmf = np.zeros(288, np.float32)
    oracle.lib().orc_symsync_filters(mf.ctypes.data, dmf.ctypes.data)
    assert np.array_equal(np.frombuffer(t.ss_mf, np.float32), mf) and np.array_equal(np.frombuffer(t.ss_dmf, np.float32), dmf)
    w = np.zeros(15, np.float32)
    oracle.lib().orc_eq_initial_taps(w.ctypes.data)
    assert np.array_equal(np.frombuffer(t.eq_h0, np.float32), w)
    sb = np.zeros(120, np.uint8)
    oracle.lib().orc_scrambler_bits(sb.ctypes.data, 120)
    assert bytes(t.scrambler) == bytes(sb)
    # the constellation table = the oracle's modem_modulate_psk of every symbol, by linear (Gray-decoded) index
    class CF(C.Structure):
        _fields_ = [("re", C.c_float), ("im", C.c_float)]
    oracle.lib().orc_modem_modulate.restype = CF
    oracle.lib().orc_modem_modulate.argtypes = [C.c_int, C.c_uint32]
    pts = np.frombuffer(t.psk_pts, np.float32).reshape(16, 2)
    for arity in (1, 2, 3):
        for lin in range(1 << arity):
            p = oracle.lib().orc_modem_modulate(arity, lin ^ (lin >> 1))
            assert (np.float32(p.re), np.float32(p.im)) == tuple(pts[(1 << arity) - 2 + lin]), (arity, lin)
    m = np.arange(128, dtype=np.float32)
    corr = np.float32(2.0) * m / np.float32(127) - np.float32(1.0)
    assert np.array_equal(np.frombuffer(t.corr_tab, np.float32), corr)
    # the integer form of the preamble thresholds decides exactly like the fp32 comparisons of src/hfdl.c:781-800
    for k in range(128):
        assert (abs(corr[k]) > np.float32(0.36)) == (k <= t.a1_lo or k >= t.a1_hi)
        assert (abs(corr[k]) > np.float32(0.3)) == (k <= t.a2_lo or k >= t.a2_hi)
        assert (corr[k] > 0) == (k >= t.pos_min)


def test_psk_soft_matches_oracle(sim, oracle):
    rng = np.random.default_rng(8)
    f2 = oracle.Cf
    for arity in (1, 2, 3):
        for _ in range(400):
            x = complex(rng.normal(0, 0.8), rng.normal(0, 0.8))
            a = np.zeros(3, np.uint8); b = np.zeros(3, np.uint8)
            sim.sim_psk_soft(arity, x.real, x.imag, a.ctypes.data)
            oracle.lib().orc_modem_demod_soft(arity, f2(x.real, x.imag), b.ctypes.data)
            assert np.array_equal(a[:arity], b[:arity])


def test_strict_arithmetic_matches_oracle_shared_math(sim, sim_strict, oracle):
    """The arithmetic the device's strict build runs (serial loop + shared_math.h) equals the oracle's under orc_variant.shared_math,
    every stage, bit for bit -- on the CPU; tests/test_gpu_strict.py then holds the device's strict build to the same oracle.  And it
    is NOT the libm arithmetic: somewhere in the stream the two oracles' gains differ in the last bit (rounding inside expf / logf)."""
    try:
        oracle.set_variant(shared_math=1)
        levels_sm = _demod_core_vs_oracle(sim_strict, oracle)
    finally:
        oracle.set_variant()
    levels_libm = _demod_core_vs_oracle(sim, oracle)
    assert len(levels_sm) == len(levels_libm) and not np.array_equal(levels_sm.view(np.uint32), levels_libm.view(np.uint32))
    assert np.allclose(levels_sm, levels_libm, rtol=2e-4)        # ... and only in rounding: the AGC level tracks within 2e-4 over the stream


def test_demod_core_matches_oracle_bit_for_bit(sim, oracle):
    """Same plain-C arithmetic, same order, no FMA contraction on either side: every stage must agree exactly."""
    _demod_core_vs_oracle(sim, oracle)


def _demod_core_vs_oracle(sim, oracle):
    assert sim.sim_sizeof_framerec() == C.sizeof(FrameRec)
    rng = np.random.default_rng(7)
    ch = oracle.Channel(250000, 10_000_000, 10_030_000, want_channelizer=False)
    rate = 7812.5
    s = sim.sim_create(np.float32(5400) / np.float32(rate), 1024)
    t, bursts = 0.2, []
    for mode in (3, 0, 6, 5):
        bursts.append(dict(mode=mode, octets=synth.make_pdu(rng, mode), t0=t, amp=0.08, cfo=-11.0))
        t += synth.burst_symbols_len(mode) / 1800 + 0.3
    x = synth.synth_channel_baseband(rate, int((t + 0.3) * rate), bursts, noise_sigma=0.004, seed=2)
    frames = (FrameRec * 16)()
    syms = np.zeros((16, 5040), np.complex64)
    got, levels = [], []
    for i in range(0, len(x) - 896, 896):
        blk = np.ascontiguousarray(x[i:i + 896])
        ch.process_baseband(blk)
        v = ch.view()
        nf = sim.sim_block(s, blk.ctypes.data, len(blk), frames, syms.ctypes.data)
        rs = np.zeros(1024, np.complex64); mf = np.zeros(1024, np.complex64); sy = np.zeros(1024, np.complex64)
        lv = np.zeros(1024, np.float32); cnt = (C.c_int * 2)()
        sim.sim_taps(s, rs.ctypes.data, mf.ctypes.data, sy.ctypes.data, lv.ctypes.data, cnt)
        assert cnt[0] == len(v["resampled"]) and cnt[1] == len(v["symbols"])
        assert np.array_equal(rs[:cnt[0]], v["resampled"]) and np.array_equal(mf[:cnt[0]], v["mf_out"])
        assert np.array_equal(lv[:cnt[0]], v["agc_level"]) and np.array_equal(sy[:cnt[1]], v["symbols"])
        levels.append(lv[:cnt[0]].copy())
        for k in range(nf):
            f = frames[k]
            octets = oracle.decode_user_data(f.mode, syms[k][:synth.mode_sizes(f.mode)["nsym"]], f.bitmask_lsb)
            got.append((f.mode, bytes(octets), f.sample_index, f.train_bad, f.train_total, np.float32(f.freq_err_hz)))
    sim.sim_destroy(s)
    want = [(p["mode"], p["octets"], p["sample_index"], p["train_bits_bad"], p["train_bits_total"], np.float32(p["freq_err_hz"]))
            for p in ch.pdus]
    assert got == want and len(got) == 4
    return np.concatenate(levels)


def test_pdu_triage_matches_oracle(sim, oracle):
    """Device-side FCS / SPDU-MPDU triage (same source compiled for the host) against the oracle's restatement."""
    rng = np.random.default_rng(21)
    sim.sim_pdu_triage.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_uint32)]
    cases = [synth.make_spdu(rng) + bytes(2)] + [synth.make_mpdu(rng, n) for n in (20, 66, 133, 268, 403)]
    for _ in range(300):                                   # random octets: exercises uplink headers, short frames, bad FCS
        cases.append(rng.integers(0, 256, int(rng.integers(1, 300)), dtype=np.uint8).tobytes())
    cases += [c[:-1] + bytes([c[-1] ^ 0x40]) for c in cases[:6]]
    seen = set()
    for c in cases:
        a = np.frombuffer(c, np.uint8).copy()
        kind, hl = C.c_int(0), C.c_uint32(0)
        st = sim.sim_pdu_triage(a.ctypes.data, len(a), C.byref(kind), C.byref(hl))
        assert (st, kind.value, hl.value) == oracle.pdu_triage(c)
        seen.add((st, kind.value))
    assert {(0, 0), (0, 1), (2, 2), (1, 1)} <= seen
    good = synth.make_spdu(rng)
    assert oracle.pdu_triage(good)[:2] == (0, 0) and oracle.pdu_triage(good[:40])[0] == 2


def lpdu_cases(rng):
    """MPDUs with real LPDU lists (down- and uplink, clean and with spoiled LPDU FCS), truncated ones, too-short LPDUs,
    SPDUs, header-FCS failures and random octets."""
    cases = []
    for i in range(40):
        total = int(rng.integers(120, 404))
        up = bool(i & 1)
        spoil = () if i % 4 < 2 else (int(rng.integers(0, 3)),)
        cases.append(synth.make_mpdu_with_lpdus(rng, total, uplink=up, spoil=spoil)[0])
    cases += [c[:int(len(c) * 0.6)] for c in cases[:8]]                         # announced LPDUs run past the end
    short = bytearray([0x03 | (2 << 2), 1, 2, 3, 4, 5, 1, 0])                   # downlink, two LPDUs of 2 and 1 octets
    fcs = synth.crc16_x25(short)
    cases.append(bytes(short) + bytes([fcs & 0xFF, fcs >> 8]) + bytes(3))
    cases.append(synth.make_spdu(rng) + bytes(2))
    cases.append(cases[0][:3] + bytes([cases[0][3] ^ 1]) + cases[0][4:])        # header FCS broken: nothing is walked
    cases += [rng.integers(0, 256, int(rng.integers(1, 300)), dtype=np.uint8).tobytes() for _ in range(300)]
    return cases


def test_lpdu_walk_matches_oracle(sim, oracle):
    """The device-side LPDU list walk (parse_lpdu_list + lpdu_parse's length / FCS checks; same source compiled for the
    host) against the oracle's restatement, and against what the generator wrote."""
    rng = np.random.default_rng(33)
    sim.sim_lpdu_walk.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    for up in (False, True):
        pdu, cnt = synth.make_mpdu_with_lpdus(rng, 300, uplink=up)
        assert oracle.lpdu_walk(pdu) == (cnt, cnt, 0, 0, 0)
        pdu, cnt = synth.make_mpdu_with_lpdus(rng, 300, uplink=up, spoil=(0,))
        assert oracle.lpdu_walk(pdu) == (cnt, cnt - 1, 1, 0, 0)
    seen = set()
    for c in lpdu_cases(rng):
        a = np.frombuffer(c, np.uint8).copy()
        counts = np.zeros(5, np.uint8)
        sim.sim_lpdu_walk(a.ctypes.data, len(a), counts.ctypes.data)
        got = tuple(int(v) for v in counts)
        assert got == oracle.lpdu_walk(c)
        seen.add(tuple(bool(v) for v in got))
    assert {(True, True, False, False, False), (True, True, True, False, False), (False,) * 5} <= seen
    assert any(s[4] for s in seen) and any(s[3] for s in seen)


def test_lpdu_walk_arbitrary_headers(sim, oracle):
    """Headers with a GOOD FCS but arbitrary contents -- any LPDU / aircraft counts, any size octets (0 = a 1-octet LPDU, 255 = 256
    octets), any PDU length from just the header to far beyond the announced LPDUs: the device-side walk and the oracle's agree on
    every count, and neither reads past the PDU (the buffers end where the PDU ends)."""
    from hypothesis import given, settings, strategies as st
    sim.sim_lpdu_walk.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]

    def with_fcs(hdr):
        fcs = synth.crc16_x25(bytes(hdr))
        return bytes(hdr) + bytes([fcs & 0xFF, fcs >> 8])

    sizes = st.lists(st.sampled_from([0, 1, 2, 3, 5, 17, 64, 200, 255]), min_size=0, max_size=15)

    @settings(max_examples=300, deadline=None)
    @given(st.booleans(), st.lists(sizes, min_size=1, max_size=8), st.integers(0, 700), st.binary(min_size=0, max_size=64), st.integers(0, 3))
    def run(uplink, groups, body_len, salt, fix_fcs_of):
        if not uplink:
            lens = groups[0]
            hdr = bytearray([0x03 | (len(lens) << 2), 1, 2, 3, 4, 5]) + bytes(lens)
        else:
            hdr = bytearray([0x01 | ((len(groups) - 1) << 4), 9])
            for g in groups:
                hdr += bytes([7, (len(g) << 4) | 5]) + bytes(g)
        pdu = bytearray(with_fcs(hdr))
        body = bytearray((salt * (body_len // max(1, len(salt)) + 1))[:body_len]) if salt else bytearray(body_len)
        # give the first `fix_fcs_of` LPDUs that fit a good FCS of their own, so that "good" is exercised as well as "bad"
        at = 0
        flat = [n for g in (groups if uplink else [groups[0]]) for n in g]
        for n in flat[:fix_fcs_of]:
            L = n + 1
            if L >= 3 and at + L <= len(body):
                f = synth.crc16_x25(bytes(body[at:at + L - 2]))
                body[at + L - 2] = f & 0xFF; body[at + L - 1] = f >> 8
            at += L
        pdu += body
        a = np.frombuffer(bytes(pdu), np.uint8).copy()
        counts = np.zeros(5, np.uint8)
        sim.sim_lpdu_walk(a.ctypes.data, len(a), counts.ctypes.data)
        got = tuple(int(v) for v in counts)
        want = oracle.lpdu_walk(bytes(pdu))
        assert got == want
        assert got[0] == got[1] + got[2] + got[3] and got[0] <= len(flat)
        if not got[4]:
            assert got[0] == len(flat)                       # nothing truncated: every announced LPDU was looked at

    run()


def test_bench_traffic_plans():
    """bench.py's synthetic traffic: bursts of a channel never overlap, all end inside the resident stretch, the burst-dense
    workload cycles all eight modes (BASELINE.json configs[3]) and the plan is a pure function of the seed."""
    import bench
    import hfdl_synth as synth
    for name, input_size in (("cfg3", 7340032), ("cfg4", 7340032), ("cfg2", 917504)):
        w = bench.WORKLOADS[name]
        freqs = bench.channel_plan(w)
        assert len(set(freqs)) == w["nch"] and all(abs(f + 1440 - w["centerfreq"]) < 0.48 * w["fs"] for f in freqs)
        dur = w["blocks"] * input_size / w["fs"]
        bursts = bench.plan_bursts(w, freqs, dur, w["seed"])
        again = bench.plan_bursts(w, freqs, dur, w["seed"])
        assert [(b["freq"], b["mode"], b["t0"], b["octets"]) for b in bursts] == [(b["freq"], b["mode"], b["t0"], b["octets"]) for b in again]
        by_freq = {}
        for b in bursts:
            by_freq.setdefault(b["freq"], []).append(b)
        assert set(by_freq) == set(freqs)
        for bl in by_freq.values():
            bl.sort(key=lambda b: b["t0"])
            ends = [b["t0"] + synth.burst_symbols_len(b["mode"]) / 1800 for b in bl]
            assert all(e < dur for e in ends)
            assert all(bl[i + 1]["t0"] > ends[i] for i in range(len(bl) - 1))
        modes = {b["mode"] for b in bursts}
        assert modes == (set(range(8)) if w.get("dense") else set(range(4)))


def _make_input_worker(q):
    import bench
    w = dict(fs=250_000, centerfreq=10_000_000, nch=2, grid=60_000, blocks=24, seed=77, noise=0.01, name="tiny")
    x, bursts = bench.make_input(w, 28672, 0, 1)
    q.put((float(np.abs(x).sum()), len(x), len(bursts)))


def test_bench_input_is_made_once_per_seed(tmp_path):
    """Ranks that share a stream (--shard channels) call make_input() at the same moment: the file lock lets one synthesise and the others
    load its file; all get the same samples, and the cache file carries the traffic plan's tag (a file left by another plan is not reused)."""
    import glob
    import multiprocessing as mp
    for f in glob.glob("/tmp/hfdl_bench_250000_seed77_*"):
        os.remove(f)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_make_input_worker, args=(q,)) for _ in range(3)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(30)
        assert p.exitcode == 0
    assert len(set(res)) == 1 and res[0][1] == 24 * 28672 and res[0][2] == 2
    files = [f for f in glob.glob("/tmp/hfdl_bench_250000_seed77_*") if f.endswith(".npy")]
    assert len(files) == 1 and len(os.path.basename(files[0]).split("_")[-1]) == 12          # <crc32 tag>.npy
    for f in glob.glob("/tmp/hfdl_bench_250000_seed77_*"):
        os.remove(f)


def test_abi_argument_checks_need_no_device():
    """Every front-end entry point rejects a NULL handle / NULL outputs with HFDL_GPU_EINVAL before touching HIP (the
    reference ASSERTs its arguments: src/fft.c:31, src/hfdl.c:648); the error text is per calling thread."""
    import ctypes as C
    from dumphfdl_amd import frontend as F
    L = F.load()
    EINVAL = -1
    n = C.c_int32(0)
    buf = (F.Pdu * 4)()
    assert L.hfdl_gpu_frontend_poll_pdus(None, buf, 4, C.byref(n)) == EINVAL
    assert L.hfdl_gpu_frontend_poll_pdus_ready(None, buf, 4, C.byref(n), 1) == EINVAL
    assert L.hfdl_gpu_frontend_counters(None, C.byref(F.FrontendCounters())) == EINVAL
    assert L.hfdl_gpu_frontend_all_channel_stats(None, None, 0, C.byref(n)) == EINVAL
    assert L.hfdl_gpu_frontend_channel_stats(None, 0, C.byref(F.ChannelStats())) == EINVAL
    assert L.hfdl_gpu_frontend_push_block(None, None, 0, 0) == EINVAL
    assert L.hfdl_gpu_frontend_push_block_raw(None, None, 0, 0, 0) == EINVAL
    assert L.hfdl_gpu_frontend_sync(None) == EINVAL
    assert L.hfdl_gpu_frontend_input_done(None) == EINVAL
    assert L.hfdl_gpu_frontend_enable_taps(None, 0) == EINVAL
    assert L.hfdl_gpu_frontend_reset_timers(None, 0) == EINVAL
    assert b"null" in L.hfdl_gpu_last_error()
    L.hfdl_gpu_frontend_destroy(None)                      # like free(NULL)
    assert L.hfdl_gpu_frontend_stream(None) is None


def test_tap_layout_is_the_matrix_operand_order(tmp_path):
    """kernels.h tap_index_f (TAPL_OCTET) on the host: a bijection; one KiB = four alias rows x eight channels x four bins with lane =
    16 (row % 4) + 2 (c % 8) + comp and register = bin % 4 -- operand A of v_mfma_f32_16x16x4_f32 for one bin, register by register;
    the bin quads of an octet, the octets and the quads of rows in that order (tests/hostsim/tap_layout_check.cpp; the device side of
    the same contract is tests/test_gpu_parity.py::test_fold_mfma_equals_fma_chain and the channelizer's parity with the oracle)."""
    exe = str(tmp_path / "tap_layout_check")
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "dumphfdl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "hostsim", "tap_layout_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
