"""GPU tests of the wideband impulse-noise blanker (hfdl_gpu_frontend_blanker_enable / _stats, hfdl_gpu_blank_block;
dumphfdl_amd/csrc/blanker_kernels.hip) against the float64 model of tests/blanker_f64.py.

Every input keeps the model's guard band (no sample's power within a relative 1e-3 of the threshold; asserted by the model's helpers),
so the device's mask must be the model's whatever the last bits of its block power.  Then:
  1. the stage alone: out == where(mask, 0, converted) bit for bit, the count is the mask's, P within 2 (d + 2) 2^-24 of float64 and
     equal, all 32 bits, to the host build of blanker.h's documented order;
  2. a front end with the blanker on, fed the impulsive input, equals -- HFDL_GPU_TAP_CHAN_OUT of every block and channel as uint32, the
     PDUs -- a front end that never enables it, fed where(mask, 0, converted) as cf32: every input path, both forms of the forward FFT's
     first pass, several receivers;
  3. the decode scenario through the device;  4. off is off;  5. hfdl_replay --blanker."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import blanker_f64 as bf
from dumphfdl_amd import frontend as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB = bf.THRESHOLD_DB
N = 28672                     # geometry.input_size at 250 ksps
TAP_SPECTRUM, TAP_CHAN_OUT = 1, 3
STAGE_SIZES = (1, 63, 64, 65, 1023, 4113, 28672)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def f32_bits(v):
    return int(np.array([v], np.float32).view(np.uint32)[0])


def to_raw(x, fmt):
    """a complex64 stream as the interleaved values of a sample format"""
    v = np.ascontiguousarray(x, dtype=np.complex64).view(np.float32)
    if fmt == F.SFMT_CS16:
        return np.clip(np.round(v * 32767.5), -32768, 32767).astype(np.int16)
    if fmt == F.SFMT_CU8:
        return np.clip(np.round(v * 127 + 63.5), 0, 255).astype(np.uint8)
    return v.copy()


# ---------------------------------------------------------------- 1. the stage alone

@pytest.fixture(scope="module")
def stage_input():
    """noise (sigma 0.01) with an impulse of amplitude 0.9 every 97 samples, the first at sample 0: 20 dB and more above the 14 dB threshold"""
    rng = np.random.default_rng(41)
    n = max(STAGE_SIZES)
    x = (0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    x[::97] += (0.9 * np.exp(2j * np.pi * rng.random(len(x[::97])))).astype(np.complex64)
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def host_power(tmp_path_factory, stage_input):
    """{(fmt, n): (depth, bits of P)} from the host build of blanker.h (tests/hostsim/blanker_sum_check.cpp)"""
    d = tmp_path_factory.mktemp("blank")
    exe = str(d / "blanker_sum_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "dumphfdl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "hostsim", "blanker_sum_check.cpp"), "-o", exe])
    out = {}
    for fmt in (F.SFMT_CF32, F.SFMT_CS16, F.SFMT_CU8):
        path = str(d / ("x%d.cf32" % fmt))
        bf.convert(to_raw(stage_input, fmt), fmt).tofile(path)
        lines = subprocess.run([exe, path] + [str(n) for n in STAGE_SIZES], capture_output=True, text=True, check=True).stdout.splitlines()
        for n, line in zip(STAGE_SIZES, lines):
            w = line.split()
            out[fmt, n] = (int(w[1]), int(w[2], 16))
    return out


@pytest.mark.parametrize("fmt", [F.SFMT_CF32, F.SFMT_CS16, F.SFMT_CU8])
@pytest.mark.parametrize("n", STAGE_SIZES)
def test_stage_alone(gpu, stage_input, host_power, n, fmt):
    raw = to_raw(stage_input[:n], fmt)
    x = bf.convert(raw, fmt)
    want, mask, P64 = bf.blank(x, DB)
    assert mask.any() and not mask.all() if n > 1 else not mask.any()      # (one sample is its own mean: never above k2 times it)
    out, P, cnt = gpu.blank_block(raw, fmt, DB)
    depth = F.blank_sum_depth(n)
    err = abs(float(P) - P64) / P64
    print("n %d fmt %d: blanked %d, |P - P64| / P64 = %.3g (bound %.3g, d = %d)" % (n, fmt, cnt, err, bf.power_bound(depth), depth))
    assert (bits(out) == bits(want)).all()
    assert cnt == int(mask.sum())
    assert err <= bf.power_bound(depth)
    assert host_power[fmt, n] == (depth, f32_bits(P))                     # the documented order IS the device's
    again = gpu.blank_block(raw, fmt, DB)
    assert f32_bits(again[1]) == f32_bits(P) and again[2] == cnt and (bits(again[0]) == bits(out)).all()


def test_stage_zeros_inf_nan_and_the_markov_share(gpu, stage_input):
    z = np.zeros(4113, np.complex64)
    out, P, cnt = gpu.blank_block(z, F.SFMT_CF32, DB)
    assert f32_bits(P) == 0 and cnt == 0 and not bits(out).any()
    for bad in (np.inf, np.nan):
        x = stage_input[:4113].copy()
        x[1234] = complex(bad, 0.0)
        out, P, cnt = gpu.blank_block(x, F.SFMT_CF32, DB)
        assert cnt == 0 and not np.isfinite(P) and (bits(out) == bits(x)).all(), bad
    # a 6 dB threshold on a block with one strong sample in 4: Markov's 25 % is reached, never passed
    x = np.full(4096, 0.01, np.complex64)
    x[::4] = 1.0
    want, mask, _ = bf.blank(x, 6.0)
    out, P, cnt = gpu.blank_block(x, F.SFMT_CF32, 6.0)
    assert cnt == 1024 == int(mask.sum()) and (bits(out) == bits(want)).all()


# ---------------------------------------------------------------- 2. pipeline == pre-blanked input

def chan_blocks(fe, back_max=0):
    """CHAN_OUT of every channel of the newest block (and up to back_max blocks before it) as uint32"""
    return [[bits(fe.read_tap(TAP_CHAN_OUT, c, back)) for c in range(fe.geometry.channels)] for back in range(back_max + 1)]


def same(a, b):
    return len(a) == len(b) and all(len(u) == len(v) and (u == v).all() for u, v in zip(a, b))


def pdu_key(pdus):
    return sorted((p["freq"], p["sample_index"], bytes(p["octets"])) for p in pdus)


def reference_run(make, blocks):
    """a front end that never enables the blanker, fed `blocks` (complex64) one by one with a sync after each:
    ([CHAN_OUT of every channel] per block, PDUs)"""
    fe = make()
    out = []
    for b in blocks:
        fe.push_block(b)
        out.append(chan_blocks(fe)[0])
    pdus = pdu_key(fe.poll_pdus())
    fe.close()
    return out, pdus


@pytest.fixture(scope="module")
def small(gpu):
    """the scenario's first five blocks at 250 ksps per sample format: converted input, the model's blanked blocks, counts and powers,
    and the never-enabled front end's outputs on the blanked blocks"""
    s = bf.scenario()
    nblk = 5
    out = {}
    for fmt in (F.SFMT_CF32, F.SFMT_CS16, F.SFMT_CU8):
        raw = to_raw(s["impulsive"][:nblk * N], fmt)
        x = bf.convert(raw, fmt)
        y, counts, powers = bf.blank_stream(x, N, DB)
        assert min(counts) > 0
        ref = reference_run(lambda: gpu.Frontend(bf.FS, bf.CF, bf.FREQS), [y[b * N:(b + 1) * N] for b in range(nblk)])
        out[fmt] = dict(raw=raw.reshape(nblk, -1), x=x, y=y, counts=counts, powers=powers, ref=ref)
    return out


def check_stats(fe, case, b, rx=0):
    st = fe.blanker_stats(rx)
    assert st["blocks"] == b + 1 and st["samples_blanked"] == sum(case["counts"][:b + 1]), (b, st)
    P64 = case["powers"][b]
    assert abs(float(st["last_power"]) - P64) / P64 <= bf.power_bound(F.blank_sum_depth(N)), (b, st, P64)
    assert f32_bits(st["last_threshold"]) == f32_bits(np.float32(bf.k2_of(DB)) * st["last_power"])


@pytest.mark.parametrize("fmt", [F.SFMT_CF32, F.SFMT_CS16, F.SFMT_CU8])
def test_pipeline_equals_preblanked_input_host_pushes(gpu, small, fmt):
    """raw pushes of every sample format (250 ksps: the LDS form of the first pass), a sync after every block; the record after every block"""
    case = small[fmt]
    fe = gpu.Frontend(bf.FS, bf.CF, bf.FREQS)
    assert fe.geometry.input_size == N and fe.geometry.fft_size < 1 << 18
    with pytest.raises(gpu.GpuError):
        fe.blanker_stats()                                               # never enabled
    for db in (-1.0, 5.9, 60.1, float("nan")):
        with pytest.raises(gpu.GpuError):
            fe.blanker_enable(db)
    fe.blanker_enable(DB)
    assert fe.blanker_stats() == dict(blocks=0, samples_blanked=0, last_power=0, last_threshold=0)
    for b, raw in enumerate(case["raw"]):
        fe.push_block_raw(raw, fmt)
        assert same(chan_blocks(fe)[0], case["ref"][0][b]), b
        check_stats(fe, case, b)
    assert pdu_key(fe.poll_pdus()) == case["ref"][1]
    fe.close()


def test_pipeline_device_resident_prefetched_and_channelize_only(gpu, small):
    """the other ways a cf32 block reaches the transform: where it lies in HBM (the forward FFT beside the fold, on the input stream), through
    a prefetch, and through channelize_block"""
    import torch
    case = small[F.SFMT_CF32]
    nblk = len(case["raw"])
    # one sample in front: every block starts 8 bytes off a 16-byte boundary, where a cf32 pair is two loads (staged host blocks take the one-load path)
    dev = torch.from_numpy(np.concatenate([np.zeros(1, np.complex64), case["x"]]).view(np.float32).copy()).cuda()
    torch.cuda.synchronize()
    assert (dev.data_ptr() + 8) % 16 == 8
    fe = gpu.Frontend(bf.FS, bf.CF, bf.FREQS)
    fe.blanker_enable(DB)
    for b in range(nblk):
        fe.push_block(dev.data_ptr() + 8 + 8 * b * N)
        assert same(chan_blocks(fe)[0], case["ref"][0][b]), b
        check_stats(fe, case, b)
    fe.close()
    del dev

    nbytes = case["x"].nbytes
    pinned = gpu.host_alloc(nbytes)
    try:
        ctypes.memmove(pinned, case["x"].ctypes.data, nbytes)
        fe = gpu.Frontend(bf.FS, bf.CF, bf.FREQS)
        fe.blanker_enable(DB)
        fe.prefetch_host_ptr(pinned)
        for b in range(nblk):
            if b + 1 < nblk:
                fe.prefetch_host_ptr(pinned + 8 * (b + 1) * N)          # the next block's copy is queued before this block is pushed
            fe.push_host_ptr(pinned + 8 * b * N)
            assert same(chan_blocks(fe)[0], case["ref"][0][b]), b
        check_stats(fe, case, nblk - 1)
        fe.close()
    finally:
        gpu.host_free(pinned)

    fe = gpu.Frontend(bf.FS, bf.CF, bf.FREQS)
    fe.blanker_enable(DB)
    for b in range(nblk):
        fe.channelize_block(case["x"][b * N:(b + 1) * N])
        assert same(chan_blocks(fe)[0], case["ref"][0][b]), b
    check_stats(fe, case, nblk - 1)
    fe.close()


def test_pipeline_eight_blocks_before_one_poll(gpu):
    """eight blocks queued before one poll against a sync after every push: the same record, the same PDUs, the same newest blocks"""
    s = bf.scenario()
    first = 20                                                           # blocks 20 .. 27: a frame ends inside them
    x = s["impulsive"][first * N:(first + 8) * N]
    y, counts, powers = bf.blank_stream(x, N, DB)
    ref_out, _ = reference_run(lambda: gpu.Frontend(bf.FS, bf.CF, bf.FREQS), [y[b * N:(b + 1) * N] for b in range(8)])
    got = {}
    for synced in (True, False):
        fe = gpu.Frontend(bf.FS, bf.CF, bf.FREQS)
        fe.blanker_enable(DB)
        for b in range(8):
            fe.push_block(x[b * N:(b + 1) * N])
            if synced:
                fe.sync()
        pdus = pdu_key(fe.poll_pdus())
        st = fe.blanker_stats()
        assert st["blocks"] == 8 and st["samples_blanked"] == sum(counts)
        assert same(chan_blocks(fe)[0], ref_out[7])
        got[synced] = (pdus, f32_bits(st["last_power"]))
        fe.close()
    assert got[True] == got[False]


@pytest.fixture(scope="module")
def big():
    """1.92 Msps, two channels: fft_size 2^18, the register-resident form of the first pass; four blocks"""
    import hfdl_synth as synth
    fs, cf, freqs, n = 1_920_000, 10_000_000, [9_600_000, 10_500_000], 229376
    rng = np.random.default_rng(1)
    bursts = [dict(freq=freqs[0], mode=1, octets=synth.make_pdu(rng, 1), t0=0.01, amp=0.005, cfo=3.0),
              dict(freq=freqs[1], mode=3, octets=synth.make_pdu(rng, 3), t0=0.02, amp=0.006, cfo=-5.0)]
    x = synth.synth_wideband(fs, cf, 4 * n, bursts, noise_sigma=0.01, seed=9)
    x, _ = bf.add_impulses(x, fs, 300, 8, 0.9, 5)
    return fs, cf, freqs, n, x


@pytest.mark.parametrize("fmt", [F.SFMT_CF32, F.SFMT_CS16])
def test_pipeline_register_resident_first_pass(gpu, big, fmt):
    fs, cf, freqs, n, x = big
    raw = to_raw(x, fmt)
    xc = bf.convert(raw, fmt)
    y, counts, powers = bf.blank_stream(xc, n, DB)
    assert min(counts) > 0
    make = lambda: gpu.Frontend(fs, cf, freqs)
    ref_out, ref_pdus = reference_run(make, [y[b * n:(b + 1) * n] for b in range(4)])
    fe = make()
    assert fe.geometry.fft_size >= 1 << 18 and fe.geometry.input_size == n
    fe.blanker_enable(DB)
    case = dict(counts=counts, powers=powers)
    for b in range(4):
        fe.push_block_raw(raw.reshape(4, -1)[b], fmt)
        assert same(chan_blocks(fe)[0], ref_out[b]), b
        st = fe.blanker_stats()
        assert st["blocks"] == b + 1 and st["samples_blanked"] == sum(counts[:b + 1])
        assert abs(float(st["last_power"]) - powers[b]) / powers[b] <= bf.power_bound(F.blank_sum_depth(n))
    assert pdu_key(fe.poll_pdus()) == ref_pdus
    fe.close()


def test_pipeline_three_receivers_each_with_its_own_power(gpu):
    """receiver 1 is receiver 0's stream x 100, receiver 2 another stretch of it: a block power shared between receivers would blank
    nothing of receiver 0 and 2"""
    s = bf.scenario()
    nblk = 4
    streams = [s["impulsive"][:nblk * N], (s["impulsive"][:nblk * N] * np.float32(100)).astype(np.complex64), s["impulsive"][7 * N:(7 + nblk) * N]]
    model = [bf.blank_stream(x, N, DB) for x in streams]
    assert model[0][1] == model[1][1] and model[0][1] != model[2][1]
    rx = [(bf.CF, bf.FREQS[:2]), (bf.CF, bf.FREQS[1:]), (bf.CF, bf.FREQS[:1])]
    ref = gpu.MultiFrontend(bf.FS, rx)
    fe = gpu.MultiFrontend(bf.FS, rx)
    fe.blanker_enable(DB)
    for b in range(nblk):
        ref.push_blocks([m[0][b * N:(b + 1) * N] for m in model])
        fe.push_blocks([x[b * N:(b + 1) * N] for x in streams])
        assert same(chan_blocks(fe)[0], chan_blocks(ref)[0]), b
        for r in range(3):
            st = fe.blanker_stats(r)
            P64 = model[r][2][b]
            assert st["blocks"] == b + 1 and st["samples_blanked"] == sum(model[r][1][:b + 1]), (b, r, st)
            assert abs(float(st["last_power"]) - P64) / P64 <= bf.power_bound(F.blank_sum_depth(N))
    with pytest.raises(gpu.GpuError):
        fe.blanker_stats(3)
    assert pdu_key(fe.poll_pdus()) == pdu_key(ref.poll_pdus())
    fe.close()
    ref.close()


# ---------------------------------------------------------------- 3. decode

def device_pdus(gpu, x, db):
    fe = gpu.Frontend(bf.FS, bf.CF, bf.FREQS)
    if db:
        fe.blanker_enable(db)
    for b in range(len(x) // N):
        fe.push_block(x[b * N:(b + 1) * N])
    out = sorted((p["freq"], bytes(p["octets"])) for p in fe.poll_pdus())
    st = fe.blanker_stats() if db else None
    fe.close()
    return out, st


def test_decode_scenario_through_the_device(gpu, oracle):
    """with the blanker the device delivers what the oracle decodes from the model-blanked stream -- every frame sent; without it, fewer"""
    s = bf.scenario()
    blanked, counts, _ = bf.blank_stream(s["impulsive"], N, DB)
    want = bf.oracle_pdus(oracle, blanked)
    assert bf.delivered(want, s["sent"]) == len(s["sent"])
    on, st = device_pdus(gpu, s["impulsive"], DB)
    assert on == want
    assert st["blocks"] == len(counts) and st["samples_blanked"] == sum(counts)
    off, _ = device_pdus(gpu, s["impulsive"], 0)
    print("delivered: %d with the blanker, %d without, of %d" % (bf.delivered(on, s["sent"]), bf.delivered(off, s["sent"]), len(s["sent"])))
    assert bf.delivered(off, s["sent"]) < bf.delivered(on, s["sent"]) == len(s["sent"])


# ---------------------------------------------------------------- 4. off is off

def test_off_is_off(gpu, small):
    """enable(14), two blocks, enable(0), three more: from the first block after the disable on, spectrum tap and CHAN_OUT equal a front
    end that never enabled anything and was fed the same stream with the first two blocks pre-blanked"""
    case = small[F.SFMT_CF32]
    x, y = case["x"], case["y"]
    a = gpu.Frontend(bf.FS, bf.CF, bf.FREQS)
    b = gpu.Frontend(bf.FS, bf.CF, bf.FREQS)
    a.blanker_enable(0.0)                                                # off before it was ever on: nothing happens
    with pytest.raises(gpu.GpuError):
        a.blanker_stats()
    a.blanker_enable(DB)
    for k in range(5):
        if k == 2:
            a.blanker_enable(0.0)
        a.push_block(x[k * N:(k + 1) * N])
        b.push_block((y if k < 2 else x)[k * N:(k + 1) * N])
        assert same(chan_blocks(a)[0], chan_blocks(b)[0]), k
        assert (bits(a.read_tap(TAP_SPECTRUM)) == bits(b.read_tap(TAP_SPECTRUM))).all(), k
    st = a.blanker_stats()
    assert st["blocks"] == 2 and st["samples_blanked"] == sum(case["counts"][:2])
    assert not same(chan_blocks(a)[0], case["ref"][0][4])                # ... and those blocks do differ from the blanked ones
    a.close()
    b.close()


# ---------------------------------------------------------------- 5. hfdl_replay --blanker

def test_replay_blanker(gpu, oracle, tmp_path):
    """hfdl_replay --blanker 14 on a cs16 file of the scenario (whole blocks): the PDUs the oracle decodes from the model-blanked
    samples of the file, and the stderr line with the model's count"""
    s = bf.scenario()
    nblk = len(s["impulsive"]) // N
    raw = to_raw(s["impulsive"][:nblk * N], F.SFMT_CS16)
    blanked, counts, _ = bf.blank_stream(bf.convert(raw, F.SFMT_CS16), N, DB)
    want = sorted((f, o.hex()) for f, o in bf.oracle_pdus(oracle, blanked))
    assert len(want) == len(s["sent"])
    path = tmp_path / "iq.cs16"
    raw.tofile(path)
    exe = os.path.join(ROOT, "dumphfdl_amd", "hfdl_replay")
    cmd = [exe, "--iq-file", str(path), "--sample-rate", str(bf.FS), "--sample-format", "CS16", "--centerfreq", str(bf.CF / 1e3), "--blanker", "14"] + \
        ["%.3f" % (f / 1e3) for f in bf.FREQS]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = sorted((int(re.search(r"freq=(-?\d+)", l).group(1)), l.split()[-1]) for l in out.stdout.splitlines() if l.startswith("PDU "))
    assert got == want
    m = re.search(r"blanker: receiver 0: (\d+) samples blanked in (\d+) blocks", out.stderr)
    assert m, out.stderr
    blocks = int(m.group(2))
    assert blocks >= nblk and int(m.group(1)) == sum(counts)
