"""GPU tests of the wideband I/Q imbalance and DC corrector (hfdl_gpu_frontend_iqbal_enable / _seed / _stats, hfdl_gpu_iqbal_blocks;
dumphfdl_amd/csrc/iqbal_kernels.hip) against the host build of dumphfdl_amd/csrc/iqbal.h (tests/hostsim/iqbal_check.cpp), which
tests/test_iqbal_cpu.py sets against the float64 model of tests/iqbal_f64.py.

  1. the stage alone: output and records equal the host build's word for word;
  2. a front end with the corrector on, fed impaired input, equals -- spectrum tap and HFDL_GPU_TAP_CHAN_OUT of every block and channel as
     uint32, the PDUs -- a front end that never enables it, fed the host-build-corrected stream as cf32: every input path, both forms of the
     forward FFT's first pass;  3. two receivers, each with its own estimate;  4. blanker and corrector together, and the blanker
     switched under a running corrector;
  5. the decode scenario through the device;  6. off is off;  7. hfdl_replay --iq-correct."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import blanker_f64 as bf
import iqbal_f64 as iq
from dumphfdl_amd import frontend as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 28672                     # geometry.input_size at 250 ksps: seven chunks
ALPHA = iq.ALPHA
TAP_SPECTRUM, TAP_CHAN_OUT = 1, 3
STAGE_SIZES = (1, 63, 4097, 28672, 1048576 + 4097)
FORMATS = (F.SFMT_CF32, F.SFMT_CS16, F.SFMT_CU8)
SEED = (np.complex64(0.028 * np.exp(0.65j)), np.complex64(0.019 + 0.011j))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def to_raw(x, fmt):
    """a complex64 stream as the interleaved values of a sample format"""
    v = np.ascontiguousarray(x, dtype=np.complex64).view(np.float32)
    if fmt == F.SFMT_CS16:
        return np.clip(np.round(v * 32767.5), -32768, 32767).astype(np.int16)
    if fmt == F.SFMT_CU8:
        return np.clip(np.round(v * 127 + 63.5), 0, 255).astype(np.uint8)
    return v.copy()


def rec_bytes(recs, n=None):
    """records -- the ctypes array of the device, or the host build's REC array -- as bytes"""
    if isinstance(recs, np.ndarray):
        return recs.tobytes()
    return bytes(memoryview(recs).cast("B"))[:(n if n is not None else len(recs)) * 48]


def same_estimate(st, rec):
    """a front end's stats dict against a record of the host build: every word"""
    return (st["blocks"], st["refused"], st["valid"], st["hold"]) == (rec["blocks"], rec["refused"], bool(rec["valid"]), bool(rec["hold"])) and \
        (bits(np.array([st["kappa"], st["dc"]], np.complex64)) == bits(np.array([rec["kappa_re"], rec["kappa_im"], rec["dc_re"], rec["dc_im"]], np.float32))).all() and \
        bits(np.float32(st["power"]))[0] == bits(np.float32(rec["power"]))[0]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("iqbal")
    exe = iq.build_host_check(d, werror=False)
    return lambda x, n, alpha=ALPHA, seed=None, hold=False: iq.host_blocks(exe, d, x, n, alpha, seed, hold)


# ---------------------------------------------------------------- 1. the stage alone

@pytest.fixture(scope="module")
def stage_input():
    x = iq.impair(iq.proper_noise(3 * max(STAGE_SIZES), 21), iq.KAPPA, iq.DC)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("n", STAGE_SIZES)
def test_stage_alone(gpu, host, stage_input, n, fmt):
    """two to four blocks from a fresh enable; alpha = 1 and 1/8; unseeded, seeded, seeded with hold"""
    big = n > N
    nblocks = 3 if big else 4
    raw = to_raw(stage_input[:nblocks * n], fmt)
    x = bf.convert(raw, fmt)
    cases = [(ALPHA, None, False), (1.0, SEED, False)] if big else [(1.0, None, False), (ALPHA, None, False), (ALPHA, SEED, True), (1.0, SEED, False), (ALPHA, SEED, False)]
    for alpha, seed, hold in cases:
        take = nblocks if seed is None else 2 + (not hold)
        want, recs, _, modes = host(x[:take * n], n, alpha, seed, hold)
        out, got = gpu.iqbal_blocks(raw[:2 * take * n], n, fmt, alpha, seed, hold)
        print("n %d fmt %d alpha %g seed %s hold %d: modes %s" % (n, fmt, alpha, seed is not None, hold, modes))
        assert (bits(out) == bits(want)).all(), (alpha, seed, hold, int((bits(out) != bits(want)).sum()))
        assert rec_bytes(got, take) == rec_bytes(recs), (alpha, seed, hold)
        assert modes[0] == (1 if seed is None else 2)
        if n >= 4097:
            assert modes[1:] == [2] * (take - 1)


def test_stage_refusals(gpu, host, stage_input):
    """a real-valued stream, an all-zero block and a NaN block first are copied word for word, as the host build copies them; the block
    after a NaN block is corrected from the state before it"""
    n = 4097
    x = stage_input[:4 * n]
    real = x.real.astype(np.complex64)
    out, recs = gpu.iqbal_blocks(real, n, F.SFMT_CF32, ALPHA)
    assert (bits(out) == bits(real)).all() and recs[3].refused == 4 and rec_bytes(recs, 4) == rec_bytes(host(real, n)[1])
    out, recs = gpu.iqbal_blocks(np.zeros(3 * n, np.complex64), n, F.SFMT_CF32, ALPHA)
    assert not bits(out).any() and recs[2].refused == 3
    for at in (0, 1):
        nan = x.copy()
        nan[at * n + 100] = np.complex64(complex(np.nan, 1.0))
        nan.view(np.uint32)[2 * (at * n + 200)] = 0x7FC01234
        want, hrecs, _, modes = host(nan, n)
        out, recs = gpu.iqbal_blocks(nan, n, F.SFMT_CF32, ALPHA)
        assert modes == ([1, 1, 2, 2] if at == 0 else [1, 2, 2, 2])
        # (a NaN that goes through the correction's arithmetic stays a NaN; which one is the machine's choice)
        o, w = out.view(np.float32), want.view(np.float32)
        assert ((bits(o) == bits(w)) | (np.isnan(o) & np.isnan(w))).all() and np.isnan(w).sum() == (2 if at == 0 else 4) and rec_bytes(recs, 4) == rec_bytes(hrecs), at
        if at == 0:
            assert (bits(out[:2 * n]) == bits(nan[:2 * n])).all()
        else:
            assert (recs[2].kappa_re, recs[2].dc_re) == (recs[1].kappa_re, recs[1].dc_re) and recs[2].valid


# ---------------------------------------------------------------- 2. pipeline == pre-corrected input

def taps(fe):
    """the newest block's spectrum tap (of the first and of the last channel's receiver) and CHAN_OUT of every channel, as uint32"""
    nch = fe.geometry.channels
    return [bits(fe.read_tap(TAP_SPECTRUM, 0)), bits(fe.read_tap(TAP_SPECTRUM, nch - 1))] + [bits(fe.read_tap(TAP_CHAN_OUT, c, 0)) for c in range(nch)]


def same(a, b):
    return len(a) == len(b) and all(len(u) == len(v) and (u == v).all() for u, v in zip(a, b))


def pdu_key(pdus):
    return sorted((p["freq"], p["sample_index"], bytes(p["octets"])) for p in pdus)


def reference_run(make, blocks, push=lambda fe, b: fe.push_block(b)):
    """a front end that never enables the corrector, fed `blocks` (complex64) one by one with a sync after each: ([taps] per block, PDUs)"""
    fe = make()
    out = []
    for b in blocks:
        push(fe, b)
        out.append(taps(fe))
    pdus = pdu_key(fe.poll_pdus())
    fe.close()
    return out, pdus


@pytest.fixture(scope="module")
def small(gpu, host):
    """the scenario's first five blocks at 250 ksps per sample format: raw and converted input, the host build's corrected blocks and
    records, and the never-enabled front end's outputs on the corrected blocks"""
    s = iq.scenario()
    nblk = 5
    out = {}
    for fmt in FORMATS:
        scale = 1.0 if fmt == F.SFMT_CF32 else 0.35                       # (the integer formats clip at 1)
        raw = to_raw(s["impaired"][:nblk * N] * np.float32(scale), fmt)
        x = bf.convert(raw, fmt)
        y, recs, _, modes = host(x, N)
        assert modes == [1, 2, 2, 2, 2]
        ref = reference_run(lambda: gpu.Frontend(iq.FS, iq.CF, iq.FREQS), [y[b * N:(b + 1) * N] for b in range(nblk)])
        out[fmt] = dict(raw=raw.reshape(nblk, -1), x=x, y=y, recs=recs, ref=ref)
    return out


@pytest.mark.parametrize("fmt", FORMATS)
def test_pipeline_equals_precorrected_input_host_pushes(gpu, small, fmt):
    """raw pushes of every sample format (250 ksps: the LDS form of the first pass), a sync after every block; the record after every block"""
    case = small[fmt]
    fe = gpu.Frontend(iq.FS, iq.CF, iq.FREQS)
    assert fe.geometry.input_size == N and fe.geometry.fft_size < 1 << 18
    with pytest.raises(gpu.GpuError):
        fe.iqbal_stats()                                                 # never enabled
    with pytest.raises(gpu.GpuError):
        fe.iqbal_seed(0.01)
    for alpha in (-1.0, 2.0 ** -11, 1.5, float("nan")):
        with pytest.raises(gpu.GpuError):
            fe.iqbal_enable(alpha)
    with pytest.raises(gpu.GpuError):
        fe.iqbal_enable(ALPHA, rx=1)
    fe.iqbal_enable(ALPHA)
    with pytest.raises(gpu.GpuError):
        fe.iqbal_seed(0.3)
    st = fe.iqbal_stats()
    assert (st["blocks"], st["refused"], st["valid"]) == (0, 0, False)
    for b, raw in enumerate(case["raw"]):
        fe.push_block_raw(raw, fmt)
        assert same(taps(fe), case["ref"][0][b]), b
        assert same_estimate(fe.iqbal_stats(), case["recs"][b]), b
    assert pdu_key(fe.poll_pdus()) == case["ref"][1]
    st = fe.iqbal_stats()
    if fmt == F.SFMT_CF32:
        assert abs(st["kappa"] - iq.KAPPA) < 0.02 * abs(iq.KAPPA) and 30 < st["image_rejection_db"] < 31
    fe.close()


def test_pipeline_device_resident_prefetched_and_channelize_only(gpu, small):
    """the other ways a cf32 block reaches the transform: where it lies in HBM (the forward FFT beside the fold, on the input stream), through
    a prefetch, and through channelize_block"""
    import torch
    case = small[F.SFMT_CF32]
    nblk = len(case["raw"])
    # one sample in front: every block starts 8 bytes off a 16-byte boundary, where a cf32 pair is two loads
    dev = torch.from_numpy(np.concatenate([np.zeros(1, np.complex64), case["x"]]).view(np.float32).copy()).cuda()
    torch.cuda.synchronize()
    assert (dev.data_ptr() + 8) % 16 == 8
    fe = gpu.Frontend(iq.FS, iq.CF, iq.FREQS)
    fe.iqbal_enable(ALPHA)
    for b in range(nblk):
        fe.push_block(dev.data_ptr() + 8 + 8 * b * N)
        assert same(taps(fe), case["ref"][0][b]), b
        assert same_estimate(fe.iqbal_stats(), case["recs"][b]), b
    fe.close()
    del dev

    nbytes = case["x"].nbytes
    pinned = gpu.host_alloc(nbytes)
    try:
        ctypes.memmove(pinned, case["x"].ctypes.data, nbytes)
        fe = gpu.Frontend(iq.FS, iq.CF, iq.FREQS)
        fe.iqbal_enable(ALPHA)
        fe.prefetch_host_ptr(pinned)
        for b in range(nblk):
            if b + 1 < nblk:
                fe.prefetch_host_ptr(pinned + 8 * (b + 1) * N)          # the next block's copy is queued before this block is pushed
            fe.push_host_ptr(pinned + 8 * b * N)
            assert same(taps(fe), case["ref"][0][b]), b
        assert same_estimate(fe.iqbal_stats(), case["recs"][nblk - 1])
        fe.close()
    finally:
        gpu.host_free(pinned)

    fe = gpu.Frontend(iq.FS, iq.CF, iq.FREQS)
    fe.iqbal_enable(ALPHA)
    for b in range(nblk):
        fe.channelize_block(case["x"][b * N:(b + 1) * N])
        assert same(taps(fe), case["ref"][0][b]), b
    assert same_estimate(fe.iqbal_stats(), case["recs"][nblk - 1])
    fe.close()


def test_pipeline_eight_blocks_before_one_poll(gpu, host):
    """eight blocks queued before one poll against a sync after every push: the same record, the same PDUs, the same newest blocks"""
    s = iq.scenario()
    first = 20                                                           # blocks 20 .. 27: a frame ends inside them
    x = s["impaired"][first * N:(first + 8) * N]
    y, recs, _, _ = host(x, N)
    ref_out, _ = reference_run(lambda: gpu.Frontend(iq.FS, iq.CF, iq.FREQS), [y[b * N:(b + 1) * N] for b in range(8)])
    got = {}
    for synced in (True, False):
        fe = gpu.Frontend(iq.FS, iq.CF, iq.FREQS)
        fe.iqbal_enable(ALPHA)
        for b in range(8):
            fe.push_block(x[b * N:(b + 1) * N])
            if synced:
                fe.sync()
        pdus = pdu_key(fe.poll_pdus())
        assert same_estimate(fe.iqbal_stats(), recs[7])
        assert same(taps(fe), ref_out[7])
        got[synced] = pdus
        fe.close()
    assert got[True] == got[False]


@pytest.fixture(scope="module")
def big():
    """1.92 Msps, two channels: fft_size 2^18, the register-resident form of the first pass; four impaired blocks"""
    import hfdl_synth as synth
    fs, cf, freqs, n = 1_920_000, 10_000_000, [9_600_000, 10_500_000], 229376
    rng = np.random.default_rng(1)
    bursts = [dict(freq=freqs[0], mode=1, octets=synth.make_pdu(rng, 1), t0=0.01, amp=0.005, cfo=3.0),
              dict(freq=freqs[1], mode=3, octets=synth.make_pdu(rng, 3), t0=0.02, amp=0.006, cfo=-5.0)]
    x = synth.synth_wideband(fs, cf, 4 * n, bursts, noise_sigma=0.01, seed=9)
    return fs, cf, freqs, n, iq.impair(x, iq.KAPPA, iq.DC)


@pytest.mark.parametrize("fmt", [F.SFMT_CF32, F.SFMT_CS16])
def test_pipeline_register_resident_first_pass(gpu, host, big, fmt):
    fs, cf, freqs, n, x = big
    raw = to_raw(x, fmt)
    y, recs, _, modes = host(bf.convert(raw, fmt), n)
    assert modes == [1, 2, 2, 2]
    make = lambda: gpu.Frontend(fs, cf, freqs)
    ref_out, ref_pdus = reference_run(make, [y[b * n:(b + 1) * n] for b in range(4)])
    fe = make()
    assert fe.geometry.fft_size >= 1 << 18 and fe.geometry.input_size == n
    fe.iqbal_enable(ALPHA)
    for b in range(4):
        fe.push_block_raw(raw.reshape(4, -1)[b], fmt)
        assert same(taps(fe), ref_out[b]), b
        assert same_estimate(fe.iqbal_stats(), recs[b]), b
    assert pdu_key(fe.poll_pdus()) == ref_pdus
    fe.close()


# ---------------------------------------------------------------- 3. two receivers

def test_two_receivers_each_with_its_own_estimate(gpu, host):
    """receiver 0 and receiver 1 carry different streams through different kappa and DC, receiver 1 seeded: a state shared between
    receivers would correct one with the other's estimate"""
    s = iq.scenario()
    nblk = 4
    k1, dc1 = -0.05 + 0.02j, -0.03 + 0.04j
    streams = [s["impaired"][:nblk * N], iq.impair(s["clean"][7 * N:(7 + nblk) * N], k1, dc1)]
    fixed = [host(streams[0], N), host(streams[1], N, ALPHA, (k1, dc1), False)]
    assert abs(complex(fixed[1][1][3]["kappa_re"], fixed[1][1][3]["kappa_im"]) - k1) < 0.02 * abs(k1)
    rx = [(iq.CF, iq.FREQS[:2]), (iq.CF, iq.FREQS[1:])]
    ref = gpu.MultiFrontend(iq.FS, rx)
    fe = gpu.MultiFrontend(iq.FS, rx)
    fe.iqbal_enable(ALPHA)
    fe.iqbal_seed(k1, dc1, hold=False, rx=1)
    for b in range(nblk):
        ref.push_blocks([f[0][b * N:(b + 1) * N] for f in fixed])
        fe.push_blocks([x[b * N:(b + 1) * N] for x in streams])
        assert same(taps(fe), taps(ref)), b
        for r in range(2):
            assert same_estimate(fe.iqbal_stats(r), fixed[r][1][b]), (b, r)
    with pytest.raises(gpu.GpuError):
        fe.iqbal_stats(2)
    assert pdu_key(fe.poll_pdus()) == pdu_key(ref.poll_pdus())
    fe.close()
    ref.close()


# ---------------------------------------------------------------- 4. blanker and corrector together

def test_blanker_and_corrector_together(gpu, host):
    """impulses on an impaired stream: the result equals the model's blanking (its guard band kept) followed by the host build's correction"""
    nblk = 4
    x = iq.impair(bf.scenario()["impulsive"][:nblk * N], iq.KAPPA, iq.DC)
    blanked, counts, _ = bf.blank_stream(x, N, bf.THRESHOLD_DB)
    assert min(counts) > 0
    y, recs, _, modes = host(blanked, N)
    assert modes == [1, 2, 2, 2]
    ref_out, ref_pdus = reference_run(lambda: gpu.Frontend(iq.FS, iq.CF, iq.FREQS), [y[b * N:(b + 1) * N] for b in range(nblk)])
    for order in (0, 1):
        fe = gpu.Frontend(iq.FS, iq.CF, iq.FREQS)
        for f in ((fe.blanker_enable, bf.THRESHOLD_DB), (fe.iqbal_enable, ALPHA))[::1 - 2 * order]:
            f[0](f[1])
        for b in range(nblk):
            fe.push_block(x[b * N:(b + 1) * N])
            assert same(taps(fe), ref_out[b]), (order, b)
            assert same_estimate(fe.iqbal_stats(), recs[b]), (order, b)
        assert fe.blanker_stats()["samples_blanked"] == sum(counts)
        assert pdu_key(fe.poll_pdus()) == ref_pdus
        fe.close()


SWITCHED_ON = (0, 1, 4, 5)              # of six blocks: the blanker is on for these, off for 2 and 3


def switched_reference(host, x, nblk):
    """one receiver's converted stream x: (the model's blanking of the blocks of SWITCHED_ON alone followed by the host build's correction
    of the whole stream, the host build's records, the model's count of blanked samples) -- with the conditions on the input asserted"""
    z = x.copy()
    blanked = 0
    for b in range(nblk):
        blk = x[b * N:(b + 1) * N]
        if b in SWITCHED_ON:
            z[b * N:(b + 1) * N], mask, _ = bf.blank(blk, bf.THRESHOLD_DB)
            blanked += int(mask.sum())
        else:
            mask, _, T, p = bf.model(blk, bf.THRESHOLD_DB)
            bf.assert_guard_band(p, T)
        assert mask.sum() > 0, b                                         # on: something is blanked; off: "off" is observable
    y, recs, _, _ = host(z, N)
    return y, recs, blanked


@pytest.mark.parametrize("nrx,fmt", [(1, F.SFMT_CF32), (2, F.SFMT_CS16)])
def test_blanker_switched_under_a_running_corrector(gpu, host, nrx, fmt):
    """The corrector on throughout, the blanker on for blocks 0 - 1, off for 2 - 3 and on again for 4 - 5: the block that reaches the
    transform is made by the blanker and then the corrector, or by the corrector alone, from block to block.  Every block equals the
    model's blanking of blocks 0, 1, 4, 5 followed by the host build's correction of the whole stream, fed to a front end that never
    enables either stage.  The scenario's first six blocks (receiver 1 of the two-receiver case: blocks 7 - 12, through another kappa and
    DC) meet the conditions on the input -- every block holds samples the model blanks, none inside its guard band.  One receiver pushed
    as cf32; two receivers pushed as cs16, where the first stage reads an integer format and the second sees the receiver stride (the
    reference starts from the quantised streams)."""
    nblk = 6
    imp = bf.scenario()["impulsive"]
    scale = np.float32(1.0 if fmt == F.SFMT_CF32 else 0.35)             # (the integer formats clip at 1)
    sent = [iq.impair(imp[:nblk * N], iq.KAPPA, iq.DC), iq.impair(imp[7 * N:(7 + nblk) * N], -0.05 + 0.02j, -0.03 + 0.04j)][:nrx]
    raws = [to_raw(s * scale, fmt).reshape(nblk, -1) for s in sent]
    fixed = [switched_reference(host, bf.convert(r.reshape(-1), fmt), nblk) for r in raws]
    if nrx == 1:
        make = lambda: gpu.Frontend(iq.FS, iq.CF, iq.FREQS)
        push = lambda fe, blocks, f=F.SFMT_CF32: fe.push_block_raw(blocks[0], f)
    else:
        make = lambda: gpu.MultiFrontend(iq.FS, [(iq.CF, iq.FREQS[:2]), (iq.CF, iq.FREQS[1:])])
        push = lambda fe, blocks, f=F.SFMT_CF32: fe.push_blocks_raw(blocks, f)
    ref_out, ref_pdus = reference_run(make, [[to_raw(y[b * N:(b + 1) * N], F.SFMT_CF32) for y, _, _ in fixed] for b in range(nblk)], push)
    fe = make()
    fe.iqbal_enable(ALPHA)
    for b in range(nblk):
        if b in (0, 2, 4):
            fe.blanker_enable(bf.THRESHOLD_DB if b in SWITCHED_ON else 0.0)
        push(fe, [r[b] for r in raws], fmt)
        assert same(taps(fe), ref_out[b]), b
        for r in range(nrx):
            assert same_estimate(fe.iqbal_stats(r), fixed[r][1][b]), (b, r)
    for r in range(nrx):
        st = fe.blanker_stats(r)
        print("receiver %d: %d samples blanked in %d blocks" % (r, st["samples_blanked"], st["blocks"]))
        assert st["samples_blanked"] == fixed[r][2]
    assert pdu_key(fe.poll_pdus()) == ref_pdus
    fe.close()


# ---------------------------------------------------------------- 5. decode

def device_pdus(gpu, x, alpha):
    fe = gpu.Frontend(iq.FS, iq.CF, iq.FREQS)
    if alpha:
        fe.iqbal_enable(alpha)
    for b in range(len(x) // N):
        fe.push_block(x[b * N:(b + 1) * N])
    out = sorted((p["freq"], bytes(p["octets"])) for p in fe.poll_pdus())
    st = fe.iqbal_stats() if alpha else None
    fe.close()
    return out, st


def test_decode_scenario_through_the_device(gpu, oracle):
    """with the corrector the device delivers what the oracle decodes from the model-corrected stream -- every frame sent; without it, at most 3"""
    s = iq.scenario()
    y, recs = iq.correct_stream(s["impaired"], N, ALPHA)
    want = iq.oracle_pdus(oracle, y)
    assert iq.delivered(want, s["sent"]) == len(s["sent"]) == 6
    on, st = device_pdus(gpu, s["impaired"], ALPHA)
    assert on == want
    assert (st["blocks"], st["refused"]) == (len(recs), 1) and abs(st["kappa"] - iq.KAPPA) < 0.02 * abs(iq.KAPPA)
    off, _ = device_pdus(gpu, s["impaired"], 0)
    print("delivered: %d with the corrector, %d without, of %d" % (iq.delivered(on, s["sent"]), iq.delivered(off, s["sent"]), len(s["sent"])))
    assert iq.delivered(off, s["sent"]) <= 3


# ---------------------------------------------------------------- 6. off is off

def test_off_is_off(gpu, small, host):
    """enable, two blocks, disable, three more: from the first block after the disable on, the taps equal those of a front end that never
    enabled anything and got the same stream with the first two blocks pre-corrected; enabled again, the estimate starts afresh"""
    case = small[F.SFMT_CF32]
    x, y = case["x"], case["y"]
    a = gpu.Frontend(iq.FS, iq.CF, iq.FREQS)
    b = gpu.Frontend(iq.FS, iq.CF, iq.FREQS)
    a.iqbal_enable(0.0)                                                  # off before it was ever on: nothing happens
    with pytest.raises(gpu.GpuError):
        a.iqbal_stats()
    a.iqbal_enable(ALPHA)
    for k in range(5):
        if k == 2:
            a.iqbal_enable(0.0)
        a.push_block(x[k * N:(k + 1) * N])
        b.push_block((y if k < 2 else x)[k * N:(k + 1) * N])
        assert same(taps(a), taps(b)), k
    st = a.iqbal_stats()
    assert (st["blocks"], st["refused"]) == (2, 1)
    assert not same(taps(a), case["ref"][0][4])                          # ... and those blocks do differ from the corrected ones
    a.iqbal_enable(ALPHA)                                                # on again: blocks 5, 6 are what a fresh enable makes of them
    again = host(np.concatenate([x[:N], x[N:2 * N]]), N)
    for k in range(2):
        a.push_block(x[k * N:(k + 1) * N])
        b.push_block(again[0][k * N:(k + 1) * N])
        assert same(taps(a), taps(b)), k
    st = a.iqbal_stats()
    assert (st["blocks"], st["refused"]) == (4, 2) and st["valid"]
    assert bits(np.array([st["kappa"]], np.complex64)).tolist() == bits(np.array([again[1][1]["kappa_re"], again[1][1]["kappa_im"]], np.float32)).tolist()
    a.close()
    b.close()


# ---------------------------------------------------------------- 7. hfdl_replay --iq-correct

def test_replay_iq_correct(gpu, oracle, tmp_path):
    """hfdl_replay --iq-correct 0.125 on a cs16 file of the scenario with interferers of rms 0.25, scaled to stay inside int16 (whole
    blocks): the PDUs the oracle decodes from the model-corrected samples of the file, and the stderr line"""
    s = iq.scenario(0.25)
    nblk = len(s["impaired"]) // N
    scaled = s["impaired"][:nblk * N] * np.float32(0.6)
    assert np.abs(scaled.view(np.float32)).max() < 1.0
    raw = to_raw(scaled, F.SFMT_CS16)
    y, recs = iq.correct_stream(bf.convert(raw, F.SFMT_CS16), N, ALPHA)
    want = sorted((f, o.hex()) for f, o in iq.oracle_pdus(oracle, y))
    assert len(want) == len(s["sent"])
    path = tmp_path / "iq.cs16"
    raw.tofile(path)
    exe = os.path.join(ROOT, "dumphfdl_amd", "hfdl_replay")
    cmd = [exe, "--iq-file", str(path), "--sample-rate", str(iq.FS), "--sample-format", "CS16", "--centerfreq", str(iq.CF / 1e3), "--iq-correct", "0.125"] + \
        ["%.3f" % (f / 1e3) for f in iq.FREQS]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = sorted((int(re.search(r"freq=(-?\d+)", l).group(1)), l.split()[-1]) for l in out.stdout.splitlines() if l.startswith("PDU "))
    assert got == want
    m = re.search(r"iq-correct: receiver 0: kappa ([-+][\d.]+)([-+][\d.]+)j \(image ([\d.]+) dB down\), dc \S+, (\d+) of (\d+) blocks refused", out.stderr)
    assert m, out.stderr
    assert abs(complex(float(m.group(1)), float(m.group(2))) - iq.KAPPA) < 0.03 * abs(iq.KAPPA) and int(m.group(4)) == 1 and int(m.group(5)) >= nblk
    assert "receiver 1" not in out.stderr
