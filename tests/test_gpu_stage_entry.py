"""The one-shot stage entry points as entry points (dumphfdl_amd/csrc/stages.cpp, lab.cpp): what the parity tests of the stages do not
pin.  hfdl_gpu_last_stage_ms() -- who sets it, who leaves it alone, what a refused run leaves; the empty CRC; argument errors; the
one layout of frames that hfdl_gpu_burst_decode and the laboratory's hfdl_gpu_lab_burst_soft share, ragged frames of three modes in one
call of each; and the laboratory's clock-probe rings read through hfdl_gpu_lab_clock_probe_read.  Smallest inputs that reach each
path."""
import ctypes as C

import numpy as np
import pytest

import burst_frames as bf
import fec_model as fm
from dumphfdl_amd import frontend as F

pytestmark = pytest.mark.gpu

EINVAL, ERANGE = -1, -5


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def three_frames():
    """BPSK rate 1/4 in 72 segments, QPSK in 72, 8-PSK in 168: three lengths, both masks; points anywhere on the plane, cleared of
    symbols where fp32 rounding could decide a byte (burst_frames.py).  With the model's answers, computed once."""
    want = [(0, 1), (2, 0), (7, 1)]
    fr = [next(f for f in bf.frames() if (f["mode"], f["mask"], f["kind"]) == (m, k, "plane")) for m, k in want]
    assert all(f["model_exact"] for f in fr) and len({len(f["symbols"]) for f in fr}) == 2
    return fr, [fm.decode(f["mode"], f["symbols"], f["mask"]) for f in fr]


def test_last_stage_ms_is_set_by_three_entry_points_only(gpu, three_frames):
    """Set by viterbi27, burst_decode and fft_forward (events around the launches: more than nothing), left alone by the four stages
    that time nothing, 0.0 after a Viterbi run refused for its LDS size -- which comes before anything is launched."""
    rng = np.random.default_rng(60)
    soft = rng.integers(0, 256, (1, 120)).astype(np.uint8)
    assert bytes(gpu.viterbi27(soft, 60)[0]) == bytes(fm.viterbi_octets(soft, 60)[0])
    t_vit = F.last_stage_ms()
    assert t_vit > 0

    frames, answers = three_frames
    few = min(range(8), key=lambda m: fm.sizes(m)["nsym"])          # the mode with the fewest segments
    assert few == frames[0]["mode"]
    assert gpu.burst_decode([frames[0]["symbols"]], [few], [frames[0]["mask"]]) == [answers[0]["octets"]]
    t_dec = F.last_stage_ms()
    assert t_dec > 0

    x = (rng.standard_normal(512) + 1j * rng.standard_normal(512)).astype(np.complex64)      # 2^9: the smallest plan
    with pytest.raises(gpu.GpuError, match=r"error -5\b"):
        gpu.fft_forward(x[:256])
    assert F.last_stage_ms() == t_dec                                # a refused size: no plan, no launch, nothing set
    got = gpu.fft_forward(x)
    assert np.abs(got - np.fft.fft(x.astype(np.complex128))).max() < 1e-3 * np.abs(got).max()
    t_fft = F.last_stage_ms()
    assert t_fft > 0

    pdu = bytes(range(1, 41))
    gpu.crc16_ccitt(pdu)
    assert F.last_stage_ms() == t_fft
    gpu.pdu_triage([pdu, pdu[:7]])
    assert F.last_stage_ms() == t_fft
    gpu.lpdu_walk([pdu, pdu[:7]])
    assert F.last_stage_ms() == t_fft
    gpu.psk_slice(2, x[:70])
    assert F.last_stage_ms() == t_fft

    with pytest.raises(gpu.GpuError, match=r"error -5: a Viterbi run over 20473 bits needs \d+ bytes of LDS"):
        gpu.viterbi27(np.zeros((1, 2 * 20473), np.uint8), 20473)
    assert F.last_stage_ms() == 0.0


@pytest.mark.parametrize("init", [0xFFFF, 0x1D0F])
def test_crc_of_nothing(gpu, oracle, init):
    """len = 0: a one-byte allocation nobody reads, a kernel that returns the initial value as the reference's loop does."""
    assert gpu.crc16_ccitt(b"", init) == oracle.crc16(np.zeros(0, np.uint8), init)
    L, crc = F.load(), C.c_uint16(0x5555)
    assert L.hfdl_gpu_crc16_ccitt(0, None, 0, init, C.byref(crc)) == 0 and crc.value == oracle.crc16(np.zeros(0, np.uint8), init)


def test_argument_errors(gpu):
    """HFDL_GPU_EINVAL, the outputs untouched and the stage time left as it was: nothing is launched for them."""
    L, lab = F.load(), F.load_lab()
    gpu.viterbi27(np.zeros((1, 120), np.uint8), 60)
    t = F.last_stage_ms()
    assert t > 0
    sym = np.zeros(2 * 5040, np.complex64)
    octets, lens = np.full((2, F.PDU_MAX_OCTETS), 0xA5, np.uint8), np.full(2, -7, np.int32)
    vin = np.full((2, F.LAB_VIN_MAX), 0xA5, np.uint8)
    soft, out = np.zeros(120, np.uint8), np.full(8, 0xA5, np.uint8)
    zero = np.zeros(2, np.int32)
    for modes, n in ((zero, 0), (np.array([0, 8], np.int32), 2), (np.array([-1, 0], np.int32), 2)):
        assert L.hfdl_gpu_burst_decode(0, _p(sym), _p(modes), _p(zero), n, _p(octets), _p(lens)) == EINVAL
        assert lab.hfdl_gpu_lab_burst_soft(0, _p(sym), _p(modes), _p(zero), n, _p(vin), _p(lens)) == EINVAL
    assert b"mode out of range" in L.hfdl_gpu_last_error() and b"mode out of range" in lab.hfdl_gpu_last_error()
    assert L.hfdl_gpu_viterbi27(0, _p(soft), 60, 0, _p(out)) == EINVAL
    assert L.hfdl_gpu_viterbi27(0, _p(soft), 0, 1, _p(out)) == EINVAL
    x, s, e = np.zeros(8, np.complex64), np.full(8, 77, np.uint32), np.full(8, 77.0, np.float32)
    for arity in (4, 0):
        assert L.hfdl_gpu_psk_slice(0, arity, _p(x), 8, _p(s), _p(e)) == EINVAL
        assert b"arity %d" % arity in L.hfdl_gpu_last_error()
    assert L.hfdl_gpu_psk_slice(0, 2, _p(x), 0, _p(s), _p(e)) == EINVAL
    stride = 16
    pdus = np.zeros((2, stride), np.uint8)
    fcs, kind, hl, counts = np.full(2, 0xA5, np.uint8), np.full(2, 0xA5, np.uint8), np.full(2, 0xA5A5, np.uint16), np.full((2, 5), 0xA5, np.uint8)
    for bad in (0, stride + 1):
        plens = np.array([stride, bad], np.int32)
        assert L.hfdl_gpu_pdu_triage(0, _p(pdus), _p(plens), 2, stride, _p(fcs), _p(kind), _p(hl)) == EINVAL
        assert b"PDU 1: length %d outside 1..16" % bad in L.hfdl_gpu_last_error()
        assert L.hfdl_gpu_lpdu_walk(0, _p(pdus), _p(plens), 2, stride, _p(counts)) == EINVAL
        assert b"PDU 1: length %d outside 1..16" % bad in L.hfdl_gpu_last_error()
    plens = np.array([stride, stride], np.int32)
    assert L.hfdl_gpu_pdu_triage(0, _p(pdus), _p(plens), 0, stride, _p(fcs), _p(kind), _p(hl)) == EINVAL
    assert L.hfdl_gpu_lpdu_walk(0, _p(pdus), _p(plens), 0, stride, _p(counts)) == EINVAL
    assert (octets == 0xA5).all() and (lens == -7).all() and (vin == 0xA5).all() and (out == 0xA5).all() and (s == 77).all() and (e == 77).all()
    assert (fcs == 0xA5).all() and (kind == 0xA5).all() and (hl == 0xA5A5).all() and (counts == 0xA5).all()
    assert F.last_stage_ms() == t


def test_burst_decode_and_burst_soft_share_one_frame_layout(gpu, three_frames):
    """Three frames of three modes and two lengths in one call of each entry point, in one process: burst_decode returns every frame's
    octets in its own row (PDU slots are claimed in completion order: the rows are routed by channel), burst_soft the model's Viterbi
    input, byte for byte."""
    frames, answers = three_frames
    syms, modes, masks = [f["symbols"] for f in frames], [f["mode"] for f in frames], [f["mask"] for f in frames]
    octets = gpu.burst_decode(syms, modes, masks)
    vin = F.lab_burst_soft(syms, modes, masks)
    for k, (f, a) in enumerate(zip(frames, answers)):
        assert octets[k] == a["octets"] and len(octets[k]) == (fm.sizes(f["mode"])["nbits"] + 7) // 8, (k, f["mode"])
        assert len(vin[k]) == fm.sizes(f["mode"])["vin"] and np.array_equal(vin[k], a["vin"]), (k, f["mode"])
    # and in the other order: a frame's row does not depend on what lies in front of it
    back = gpu.burst_decode(syms[::-1], modes[::-1], masks[::-1])
    assert back == octets[::-1]


def _probe(lab, which, cap=4096):
    buf = np.zeros((cap, 4), np.uint64)
    n = C.c_int32(-1)
    F._check(lab.hfdl_gpu_lab_clock_probe_read(which, _p(buf), cap, C.byref(n)), lab)
    assert 0 <= n.value <= cap
    return [tuple(int(v) for v in r) for r in buf[:n.value]]


def test_clock_probe_rings(gpu):
    """hfdl_gpu_lab_clock_probe_read: the records made since the last read, oldest first, at most `max`, then the ring's count starts
    over.  One record per demodulator launch (tag 1000 + its blocks) and per fold launch (tag columns x 100 + blocks: the four-column
    form up to four blocks, sixteen columns up to sixteen), counted against the front end's launch timers."""
    lab = F.load_lab()
    fs, cf = 250000, 10_000_000
    fe = gpu.Frontend(fs, cf, [9_958_000, 10_061_000], lib=lab)
    try:
        g = fe.geometry
        assert 2 <= g.demod_batch and 2 <= g.fold_batch <= 16
        n = fe.input_size
        rng = np.random.default_rng(9)
        x = (0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
        _probe(lab, 0), _probe(lab, 1)                    # whatever earlier front ends of this process left
        assert _probe(lab, 0) == [] and _probe(lab, 1) == []
        fe.reset_timers(True)
        blocks = 2 * g.fold_batch                         # two halves
        for _ in range(blocks):
            fe.push_block(x)
        fe.sync()
        demod, fold = _probe(lab, 1), _probe(lab, 0)
        _, demod_n, demod_blocks = fe.demod_time_ms()
        _, fold_n = fe.fold_time_ms()
        print("demodulator records", demod, "fold records", fold)
        assert len(demod) == demod_n >= 2 and demod_blocks == blocks
        assert all(1001 <= r[0] <= 1000 + g.demod_batch for r in demod) and sum(r[0] - 1000 for r in demod) == blocks
        assert len(fold) == fold_n >= 2
        assert all(r[0] == 1600 + g.fold_batch for r in fold) if g.fold_batch > 4 else all(r[0] == 400 + g.fold_batch for r in fold)
        assert all(r[1] > 0 and r[2] > 0 and r[3] > 0 for r in demod + fold)
        assert [r[3] for r in demod] == sorted(r[3] for r in demod) and [r[3] for r in fold] == sorted(r[3] for r in fold)      # oldest first
        assert _probe(lab, 1) == [] and _probe(lab, 0) == []         # a second read at once

        # max = 1 with two launches waiting -- a lone block, then two in one launch: the OLDEST one, and the other is gone with the count
        fe.push_block(x)
        fe.sync()
        fe.push_block(x)
        fe.push_block(x)
        fe.sync()
        assert fe.demod_time_ms()[1] == demod_n + 2 and fe.fold_time_ms()[1] == fold_n + 2
        one_d, one_f = _probe(lab, 1, 1), _probe(lab, 0, 1)
        assert len(one_d) == 1 and one_d[0][0] == 1001 and one_d[0][3] > demod[-1][3]
        assert len(one_f) == 1 and one_f[0][0] == 401 and one_f[0][3] > fold[-1][3]
        assert _probe(lab, 1) == [] and _probe(lab, 0) == []
        assert lab.hfdl_gpu_lab_clock_probe_read(1, None, 4, C.byref(C.c_int32(0))) == EINVAL
        assert lab.hfdl_gpu_lab_clock_probe_read(1, _p(np.zeros(4, np.uint64)), 0, C.byref(C.c_int32(0))) == EINVAL
    finally:
        fe.close()
