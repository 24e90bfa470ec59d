"""CPU tests of the frame quality records (include/hfdl_gpu.h hfdl_gpu_frame_quality): the float64 definition's closed forms, the host
build of the per-frame function the device runs (dumphfdl_amd/csrc/quality.h) against that definition on the burst decoder's frame
set, the argument checks that need no device, the headers and the ABI, and the host library's frame log against the two stand-ins."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import burst_frames
import fec_model as fm
import quality_f64 as Q
from dumphfdl_amd import frontend as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dumphfdl_amd", "host")
EINVAL = -1
NAMES = ("hfdl_gpu_frontend_quality_enable", "hfdl_gpu_frontend_quality_read", "hfdl_gpu_frame_quality_batch")


# ---------------------------------------------------------------- the definition

def constellation(mode, rng):
    """A frame of exact constellation points of the mode, drawn at random (complex128)."""
    sz = fm.sizes(mode)
    M = 1 << sz["arity"]
    return np.exp(2j * np.pi * rng.integers(0, M, sz["nsym"]) / M)


@pytest.mark.parametrize("mode", range(8))
def test_closed_forms(mode):
    """A clean constellation at amplitude a: err_power = (1 - a)^2, gain = a, sym_power = a^2; a constant rotation inside the decision
    region: gain = a e^{j phi}; one bad segment shows in exactly its entry; the descrambler's +-1 changes nothing."""
    rng = np.random.default_rng(100 + mode)
    sz = fm.sizes(mode)
    pts = constellation(mode, rng)
    a = 0.8
    m = Q.model((a * pts).astype(np.complex64), mode)
    assert abs(m["err_power"] - (1 - a) ** 2) < 1e-6 and abs(m["sym_power"] - a * a) < 1e-6 and abs(m["gain"] - a) < 1e-6
    assert abs(m["err_max"] - (1 - a) ** 2) < 1e-6 and np.allclose(m["seg_err_power"], (1 - a) ** 2, atol=1e-6)
    phi = 0.4 * np.pi / (1 << sz["arity"])                       # inside the decision region, whose half-width is pi / M
    m = Q.model((a * np.exp(1j * phi) * pts).astype(np.complex64), mode)
    assert abs(m["gain"] - a * np.exp(1j * phi)) < 1e-6
    assert abs(m["sym_power"] - abs(m["gain"]) ** 2) < 1e-6      # the gain- and phase-corrected error of a rotated clean frame is 0
    bad = 17
    x = pts.copy()
    x[bad * 30:(bad + 1) * 30] *= 0.5
    m = Q.model(x.astype(np.complex64), mode)
    want = np.zeros(m["segments"])
    want[bad] = 0.25
    assert np.allclose(m["seg_err_power"], want, atol=1e-6) and abs(m["err_power"] - 0.25 / m["segments"]) < 1e-7
    x = (0.7 * pts * np.exp(1j * rng.normal(0, 0.05, len(pts))) + 0.05 * (rng.standard_normal(len(pts)) + 1j * rng.standard_normal(len(pts)))).astype(np.complex64)
    sign = (1 - 2 * fm.scrambler(len(x)).astype(np.float32)) * -1.0    # descrambler and bitmask_lsb = 1
    m0, m1 = Q.model(x, mode), Q.model(x * sign.astype(np.complex64), mode)
    for k in ("sym_power", "err_power", "err_max", "gain"):                     # (in float64, exp(j (t + pi)) is -exp(j t) to within 2e-16)
        assert abs(m0[k] - m1[k]) < 1e-13, k
    assert np.allclose(m0["seg_err_power"], m1["seg_err_power"], rtol=0, atol=1e-13)


# ---------------------------------------------------------------- the host build of the device's function

@pytest.fixture(scope="module")
def host_build(tmp_path_factory):
    """tests/hostsim/quality_check.cpp, contraction off: run([(mode, symbols)]) -> one record (dict) per frame."""
    d = tmp_path_factory.mktemp("q")
    exe = str(d / "quality_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-Wno-unused-parameter",
                           os.path.join(ROOT, "tests", "hostsim", "quality_check.cpp"), "-o", exe])

    def run(frames):
        src, dst = d / "in.bin", d / "out.bin"
        with open(src, "wb") as f:
            f.write(struct.pack("<i", len(frames)))
            for mode, symbols in frames:
                f.write(struct.pack("<i", mode))
                f.write(np.asarray(symbols, np.complex64).tobytes())
        subprocess.check_call([exe, str(src), str(dst)])
        raw = open(dst, "rb").read()
        assert len(raw) == len(frames) * C.sizeof(F.FrameQuality)
        recs = (F.FrameQuality * len(frames)).from_buffer_copy(raw)
        return [F.quality_to_dict(recs[i]) for i in range(len(frames))]
    return run


@pytest.fixture(scope="module")
def host_records(host_build):
    return host_build([(f["mode"], f["symbols"]) for f in burst_frames.frames()])


def test_frame_set_is_clear_of_the_decision_boundaries():
    """No decision-boundary filter is applied below, because the inputs need none: every frame is clear of the boundaries by
    fec_model.margins, except BPSK zeros and 8-PSK at 1e-20, where either decision gives the same figures to within 1e-20.  A change to
    the frame set that breaks this fails HERE and cannot hide a failure of the comparison."""
    frames = burst_frames.frames()
    assert {f["kind"] for f in frames} == set(burst_frames.KINDS) and {f["mode"] for f in frames} == set(range(8)) and {f["mask"] for f in frames} == {0, 1}
    for f in frames:
        assert Q.decisions_are_safe(f), (f["mode"], f["mask"], f["kind"])
    assert sorted({(f["kind"], fm.sizes(f["mode"])["arity"]) for f in frames if not f["cleared"]}) == [("tiny", 3), ("zeros", 1)]


def test_host_build_against_the_model(host_records):
    """The per-frame function of quality.h, compiled for the host without contraction, on every frame of tests/burst_frames.py (every
    mode, both masks, all six kinds, |x| = 50 and 1e-20 included) within quality_f64's bound: K = 96 roundings' worth -- 44 on the
    longest path (3 per term, 30 sequential adds, the division by 30, 2 adds in the lane, 6 over the wave, the final division, 1 for the
    fp32 constellation table), doubled because |e|^2 <= 2 (|x|^2 + 1), and room for second order; 96 <= 256."""
    assert Q.K == 96
    frames = burst_frames.frames()
    for f, rec in zip(frames, host_records):
        what = (f["mode"], f["mask"], f["kind"])
        assert rec["mode"] == f["mode"]
        Q.check(rec, Q.model(f["symbols"], f["mode"]), what)


@pytest.mark.parametrize("mode", [0, 1, 3, 6])
def test_host_build_masks_bad_segment_and_repeat(host_build, mode):
    """A frame computed twice gives the same bits; the descrambler's +-1 changes no bit for BPSK and stays within the bound of the
    same model answer otherwise (the fp32 table's points are cosf / sinf values: opposite points are opposite to within an ulp, not
    exactly); one bad segment shows in exactly its seg_err_power entry, every other entry the same bits as in the undisturbed frame."""
    rng = np.random.default_rng(200 + mode)
    pts = constellation(mode, rng)
    x = (0.7 * pts * np.exp(1j * rng.normal(0, 0.05, len(pts))) + 0.05 * (rng.standard_normal(len(pts)) + 1j * rng.standard_normal(len(pts)))).astype(np.complex64)
    assert Q.decisions_are_safe(dict(symbols=x, mode=mode, cleared=True))
    sign = (-(1 - 2 * fm.scrambler(len(x)).astype(np.float32))).astype(np.complex64)
    bad = fm.sizes(mode)["nsym"] // 30 - 1                       # the last segment: lane 7 (single slot) / lane 39 (double slot) of the wave
    y = x.copy()
    y[bad * 30:(bad + 1) * 30] *= np.float32(0.5)
    a, b, c, d = host_build([(mode, x), (mode, x * sign), (mode, x), (mode, y)])
    words = lambda r: np.frombuffer(r["raw"], np.uint32)
    assert np.array_equal(words(a), words(c))
    if mode == 0:
        assert np.array_equal(words(a), words(b))
    Q.check(a, Q.model(x, mode), "plain")
    Q.check(b, Q.model(x, mode), "descrambled")
    differ = np.flatnonzero(a["seg_err_power"].view(np.uint32) != d["seg_err_power"].view(np.uint32))
    assert differ.tolist() == [bad] and d["seg_err_power"][bad] > 2 * a["seg_err_power"][bad]
    Q.check(d, Q.model(y, mode), "bad segment")


# ---------------------------------------------------------------- the library without a device

def test_entry_points_check_arguments_without_a_device():
    L = F.load()
    err = L.hfdl_gpu_last_error
    for ring, flags in ((64, 0), (0, 0), (1, 2), (-1, 0), (F.QUALITY_RING_MAX + 1, 1)):
        assert L.hfdl_gpu_frontend_quality_enable(None, ring, flags) == EINVAL
        assert b"null" in err(), err()
    rec = (F.FrameQuality * 2)()
    before = bytes(rec)
    sym = (C.c_float * (2 * 2 * F.QUALITY_SYMBOLS_MAX))()
    n, dropped = C.c_int32(7), C.c_uint32(7)
    for wait in (0, 1):
        assert L.hfdl_gpu_frontend_quality_read(None, rec, None, 2, C.byref(n), C.byref(dropped), wait) == EINVAL
        assert b"null" in err(), err()
    # null n, max_frames < 0, out == NULL with max_frames > 0: refused before the handle is looked at and before anything is written
    bogus = C.c_void_p(8)
    assert L.hfdl_gpu_frontend_quality_read(bogus, rec, sym, 2, None, C.byref(dropped), 0) == EINVAL
    assert L.hfdl_gpu_frontend_quality_read(bogus, rec, sym, -1, C.byref(n), C.byref(dropped), 1) == EINVAL
    assert L.hfdl_gpu_frontend_quality_read(bogus, None, None, 1, C.byref(n), C.byref(dropped), 0) == EINVAL
    assert (n.value, dropped.value) == (7, 7) and bytes(rec) == before and not any(sym)
    # the stage entry: null pointers, no frames, a mode out of range -- before a device is selected
    x = np.zeros(2160, np.complex64)
    modes = (C.c_int32 * 1)(1)
    p = x.ctypes.data_as(C.c_void_p)
    for args in ((None, modes, 1, rec), (p, None, 1, rec), (p, modes, 1, None), (p, modes, 0, rec), (p, modes, -3, rec), (p, (C.c_int32 * 1)(8), 1, rec),
                 (p, (C.c_int32 * 1)(-1), 1, rec)):
        assert L.hfdl_gpu_frame_quality_batch(0, *args) == EINVAL, args
    assert bytes(rec) == before


def test_headers_declare_the_records():
    hdr = open(os.path.join(ROOT, "include", "hfdl_gpu.h")).read()
    declared = set(re.findall(r"\b(hfdl_gpu_[a-z0-9_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared and name in F.EXPORTS
    for name, value in (("SYMBOLS", "1u"), ("SEGMENTS_MAX", "168"), ("SYMBOLS_MAX", "5040"), ("RING_MAX", "65536")):
        assert re.search(r"#define\s+HFDL_GPU_QUALITY_%s\s+%s\b" % (name, value), hdr), name
    assert (F.QUALITY_SYMBOLS, F.QUALITY_SEGMENTS_MAX, F.QUALITY_SYMBOLS_MAX, F.QUALITY_RING_MAX) == (1, 168, 5040, 65536)
    assert re.search(r"float\s+seg_err_power\[HFDL_GPU_QUALITY_SEGMENTS_MAX\];\s*\}\s*hfdl_gpu_frame_quality;", hdr)
    assert C.sizeof(F.FrameQuality) == 744 and F.FrameQuality.seg_err_power.offset == 72 and F.FrameQuality.sym_power.offset == 52
    host = open(os.path.join(ROOT, "include", "hfdl_host.h")).read()
    assert re.search(r"\bint\s+hfdl_frontend_set_frame_log\s*\(\s*const char \*path\s*\)\s*;", host)
    src = open(os.path.join(HOST, "frontend.c")).read()
    for name in NAMES[:2]:
        assert re.search(r"#pragma weak %s\b" % name, src), name


def test_abi_is_pinned():
    """tests/abi/hfdl_gpu_quality_abi.c: size and offsets of the record, the constants and the prototypes, in C11 with every warning an
    error; and the host library's setter takes a path or NULL without a device."""
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c11", "-D_GNU_SOURCE", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + inc, os.path.join(ROOT, "tests", "abi", "hfdl_gpu_quality_abi.c")])
    H = C.CDLL(os.path.join(ROOT, "dumphfdl_amd", "libhfdl_host.so"))
    f = H.hfdl_frontend_set_frame_log
    f.argtypes = [C.c_char_p]
    assert f(b"/tmp/frames.log") == 0 and f(None) == 0


# ---------------------------------------------------------------- the host library's frame log, on the CPU

def build_replay(d, standin):
    probe = d / "p.c"
    probe.write_text("int main(void){return 0;}\n")
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]
    if subprocess.run(["gcc"] + san + [str(probe), "-o", str(d / "p")], capture_output=True).returncode != 0:
        san = []                                                 # a gcc without the sanitizers' runtime: the run still checks the behaviour
    exe = str(d / ("replay_" + standin[:-2]))
    subprocess.check_call(["gcc", "-g", "-O1", "-std=c11", "-D_GNU_SOURCE", "-Wall", "-Wextra"] + san + ["-I", os.path.join(ROOT, "include"), "-I", HOST] +
                          [os.path.join(HOST, f) for f in ("hfdl_replay.c", "ring.c", "blocks.c", "input.c", "sink.c", "frontend.c")] +
                          [os.path.join(ROOT, "tests", "hostsim", standin), "-o", exe, "-lpthread", "-lm"])
    return exe


def run_replay(exe, source, *options):
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    cmd = [exe, "--iq-file", source, "--sample-rate", "250000", "--sample-format", "CS16", "--read-buffer-size", "4096", "--centerfreq", "10000"] + \
        list(options) + ["10010", "10020"]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=60, env=env)


@pytest.fixture(scope="module")
def recording(tmp_path_factory):
    path = tmp_path_factory.mktemp("iq") / "in.cs16"
    np.random.default_rng(5).integers(0, 256, (40 * 3072 + 100) * 4, dtype=np.uint8).tofile(path)      # 40 blocks of the stand-in's geometry
    return str(path)


def test_frame_log_is_refused_by_a_library_without_the_records(tmp_path, recording):
    """hfdl_replay --frame-log against the plain stand-in (no quality entry points): the message, a non-zero status, no crash."""
    exe = build_replay(tmp_path, "gpu_standin.c")
    log = tmp_path / "frames.log"
    out = run_replay(exe, recording, "--frame-log", str(log))
    assert out.returncode == 1 and "frame log: this GPU library has no frame quality records" in out.stderr, (out.returncode, out.stderr)
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr and out.stdout == ""
    assert run_replay(exe, recording).returncode == 0              # without the option nothing has changed


def test_frame_log_has_one_line_per_pdu(tmp_path, recording):
    """... and against tests/hostsim/gpu_standin_quality.c, which has them: as many lines as PDUs, each with its PDU's time and
    frequency, and the figures as the line states them."""
    exe = build_replay(tmp_path, "gpu_standin_quality.c")
    log = tmp_path / "frames.log"
    out = run_replay(exe, recording, "--frame-log", str(log))
    assert out.returncode == 0 and "Sanitizer" not in out.stderr and "runtime error" not in out.stderr and "frame log:" not in out.stderr, out.stderr
    pdus = [dict(kv.split("=") for kv in line.split()[1:-1]) for line in out.stdout.splitlines() if line.startswith("PDU ")]
    lines = open(log).read().splitlines()
    assert len(pdus) == 40 and len(lines) == len(pdus)
    got = []
    for line in lines:
        assert line.startswith("FRAME ")
        kv = dict(x.split("=") for x in line.split()[1:])
        got.append((kv["ts"], kv["freq"]))
        assert (kv["mode"], kv["slot"], kv["mer_db"], kv["worst_segment"], kv["worst_mer_db"]) == ("0", "S", "20.00", "5", "10.00"), line
        assert (kv["sym_power"], kv["gain"], kv["gain_phase_deg"]) == ("1.0000", "1.0000", "53.13"), line
    assert sorted(got) == sorted((p["ts"], p["freq"]) for p in pdus)
