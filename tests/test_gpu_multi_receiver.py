"""Several receivers' I/Q streams in ONE front end (hfdl_gpu_frontend_create_multi / push_blocks_raw, dumphfdl_amd.MultiFrontend):
every receiver's PDUs, channelizer output and spectrum equal those of a front end of its own, bit for bit where the fold runs the
same slices; PDUs stay with the receiver that sent them; the fold-bound shape against the oracle; every fold tiling equals the
FMA chain with receivers; call sequences and misuse change nothing."""
import os
import struct
import sys

import numpy as np
import pytest

from dumphfdl_amd import frontend as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

RMS_TOL = 1e-4


def rel_rms(a, b):
    a = np.asarray(a, np.complex128)
    b = np.asarray(b, np.complex128)
    return float(np.sqrt(np.mean(np.abs(a - b) ** 2) / max(np.mean(np.abs(b) ** 2), 1e-300)))


def fbits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def pdu_full_key(p):
    """Every field of a PDU but the (global) channel index, the float metadata by bit pattern."""
    return (p["freq"], p["sample_index"], p["mode"], p["bit_rate"], p["octets"], p["slot"], p["fcs_status"], p["pdu_kind"],
            p["hdr_len"], p["train_bits_bad"], p["train_bits_total"], tuple(p["lpdus"]),
            fbits(p["freq_err_hz"]), fbits(p["rssi_db"]), fbits(p["noise_floor_db"]))


def receiver_inputs(fs, centres, nchs, seeds, blocks, input_size, grid=15_000):
    """One synthetic stream per receiver (bench.make_input: a burst per channel + AWGN): (freqs per receiver, streams, bursts)."""
    freqs, xs, bursts = [], [], []
    for cf, nch, seed in zip(centres, nchs, seeds):
        w = dict(fs=fs, centerfreq=cf, nch=nch, grid=grid, blocks=blocks, seed=seed, noise=0.02)
        x, b = bench.make_input(w, input_size, 0, 1)
        freqs.append(bench.channel_plan(w))
        xs.append(x)
        bursts.append(b)
    return freqs, xs, bursts


def input_size_of(fs, cf=10_000_000):
    fe = F.Frontend(fs, cf, [cf + 1000])
    n = fe.input_size
    fe.close()
    return n


def as_raw(x, fmt):
    f = x.view(np.float32)
    if fmt == F.SFMT_CS16:
        return np.clip(np.round(f * 20000), -32768, 32767).astype(np.int16)
    if fmt == F.SFMT_CU8:
        return np.clip(np.round(f * 100 + 127.5), 0, 255).astype(np.uint8)
    return f


@pytest.mark.parametrize("feed", ["host_cf32", "device", "cs16", "cu8"])
def test_multi_receiver_is_bit_identical_to_one_front_end_per_receiver(gpu, feed):
    """Three receivers at 2.048 Msps, different centres and seeds, 1, 3 and 9 channels (each padded to its own octet: 1 -> 8, 3 -> 8,
    9 -> 16 slots).  With the same fold slices (16 everywhere here) every receiver's PDUs -- every field, the float metadata by bit
    pattern --, its channelizer output of the newest blocks and its spectrum equal those of a front end of its own fed the same blocks."""
    fs = 2_048_000
    centres, nchs, seeds = [10_000_000, 11_300_000, 8_950_000], [1, 3, 9], [21, 22, 23]
    n = input_size_of(fs)
    blocks = 30
    freqs, xs, _ = receiver_inputs(fs, centres, nchs, seeds, blocks, n)
    multi = gpu.MultiFrontend(fs, list(zip(centres, freqs)))
    singles = [gpu.Frontend(fs, cf, fr) for cf, fr in zip(centres, freqs)]
    assert multi.geometry.channels == sum(nchs) and multi.nrx == 3
    assert multi.geometry.fold_slices == 16 and all(s.geometry.fold_slices == 16 for s in singles)
    assert multi.geometry.fold_batch == singles[0].geometry.fold_batch and multi.geometry.demod_batch == singles[0].geometry.demod_batch
    dev = None
    if feed == "device":
        import torch
        dev = [torch.from_numpy(np.array(x.view(np.float32))).cuda() for x in xs]
        torch.cuda.synchronize()
    fmt = {"host_cf32": F.SFMT_CF32, "device": F.SFMT_CF32, "cs16": F.SFMT_CS16, "cu8": F.SFMT_CU8}[feed]
    raws = [as_raw(x, fmt) for x in xs]
    for b in range(blocks):
        if feed == "device":
            ptrs = [d.data_ptr() + 8 * b * n for d in dev]
            multi.push_blocks(ptrs)
            for s, p in zip(singles, ptrs):
                s.push_block(p)
        else:
            blk = [r[2 * b * n:2 * (b + 1) * n] for r in raws]
            multi.push_blocks_raw(blk, fmt)
            for s, r in zip(singles, blk):
                s.push_block_raw(r, fmt)
    mp = multi.poll_pdus()
    sp = [s.poll_pdus() for s in singles]
    assert sum(len(p) for p in sp) >= 8
    base = 0
    for r, (s, pr) in enumerate(zip(singles, sp)):
        mine = [p for p in mp if p["receiver"] == r]
        for p in mine:
            assert p["channel"] == base + freqs[r].index(p["freq"])
        assert sorted(pdu_full_key(p) for p in mine) == sorted(pdu_full_key(p) for p in pr), r
        for back in (0, 1):
            for c in range(nchs[r]):
                a = multi.read_tap(F.TAP_CHAN_OUT, base + c, back)
                e = s.read_tap(F.TAP_CHAN_OUT, c, back)
                assert len(a) == len(e) and a.tobytes() == e.tobytes(), (r, c, back)
            assert multi.read_tap(F.TAP_SPECTRUM, base, back).tobytes() == s.read_tap(F.TAP_SPECTRUM, 0, back).tobytes(), (r, back)
        assert multi.receiver_of(base) == (r, centres[r])
        base += nchs[r]
    multi.close()
    for s in singles:
        s.close()


def test_no_crosstalk_between_receivers(gpu):
    """Two receivers, six channels each at the same offsets from their centres: receiver 0 carries a burst per channel, receiver 1
    noise only.  Every PDU comes from receiver 0, is a payload it sent, and receiver 1 yields nothing: a workgroup that folded the
    wrong receiver's spectrum would put receiver 0's bursts on receiver 1's channels."""
    fs = 2_048_000
    n = input_size_of(fs)
    blocks = 30
    w = dict(fs=fs, centerfreq=10_000_000, nch=6, grid=60_000, blocks=blocks, seed=31, noise=0.02)
    x0, bursts = bench.make_input(w, n, 0, 1)
    f0 = bench.channel_plan(w)
    off = 2_500_000
    f1 = [f + off for f in f0]
    rng = np.random.default_rng(32)
    x1 = ((rng.standard_normal(len(x0)) + 1j * rng.standard_normal(len(x0))) * 0.02).astype(np.complex64)
    fe = gpu.MultiFrontend(fs, [(10_000_000, f0), (10_000_000 + off, f1)])
    for b in range(blocks):
        fe.push_blocks([x0[b * n:(b + 1) * n], x1[b * n:(b + 1) * n]])
    pdus = fe.poll_pdus()
    by_freq = {}
    for b in bursts:
        by_freq.setdefault(b["freq"], []).append(b)
    assert len(pdus) >= 5
    assert all(p["receiver"] == 0 and p["channel"] < 6 for p in pdus)
    assert all(bench.matches_sent(p, by_freq) for p in pdus)
    assert fe.counters()["pdus_dropped"] == 0
    fe.close()


def test_fold_bound_receivers_against_the_oracle(gpu, oracle):
    """Four cfg2-shaped receivers (8 Msps x 32 channels: 128 channels in all -- the fold-bound shape, 32-block halves, held-back
    demodulators), different centres and seeds, input resident in HBM.  Per receiver the PDUs equal the oracle's on the same stream
    (eight channels of each receiver run through the oracle), the channelizer output is within the suite's relative RMS, every PDU is a
    sent payload with a good device FCS and nothing is dropped."""
    import torch
    w0 = dict(bench.WORKLOADS["cfg2"])
    centres, seeds = [10_000_000, 13_000_000, 6_500_000, 17_200_000], [41, 42, 43, 44]
    fe = None
    ws = [dict(w0, seed=s, centerfreq=c) for s, c in zip(seeds, centres)]
    freqs = [bench.channel_plan(w) for w in ws]
    fe = gpu.MultiFrontend(w0["fs"], list(zip(centres, freqs)))
    g = fe.geometry
    assert g.channels == 128 and g.fold_batch == 32
    n = g.input_size
    streams = [bench.make_input(w, n, 0, 1) for w in ws]
    nblk = min(len(x) for x, _ in streams) // n
    sub = [0, 5, 9, 14, 18, 23, 27, 31]
    nthr = max(4, min(16, os.cpu_count() or 4))
    oras = [oracle.Frontend(w0["fs"], c, [fr[i] for i in sub], nthreads=nthr) for c, fr in zip(centres, freqs)]
    dev = [torch.from_numpy(np.array(x.view(np.float32))).cuda() for x, _ in streams]
    torch.cuda.synchronize()
    fe.enable_taps(False)
    worst = 0.0
    for b in range(nblk):
        fe.push_blocks([d.data_ptr() + 8 * b * n for d in dev])
        for (x, _), o in zip(streams, oras):
            o.push_block(x[b * n:(b + 1) * n], nthreads=nthr)
        if b in (0, nblk - 1):
            fe.sync()
            for r, o in enumerate(oras):
                for i, c in enumerate(sub):
                    worst = max(worst, rel_rms(fe.read_tap(F.TAP_CHAN_OUT, 32 * r + c), o.channel_view(i)["chan_out"]))
    pdus = fe.poll_pdus()
    assert worst < RMS_TOL, worst
    cnt = fe.counters()
    assert cnt["pdus_dropped"] == 0 and cnt["pdus_taken"] == len(pdus) and cnt["blocks"] == nblk
    key = lambda p: (p["freq"], p["sample_index"], p["mode"], p["octets"])
    total_sub = 0
    for r, ((x, bursts), o) in enumerate(zip(streams, oras)):
        by_freq = {}
        for b in bursts:
            by_freq.setdefault(b["freq"], []).append(b)
        mine = [p for p in pdus if p["receiver"] == r]
        assert all(bench.matches_sent(p, by_freq) and p["fcs_status"] == F.FCS_GOOD for p in mine)
        subset = sorted(key(p) for p in mine if p["channel"] - 32 * r in sub)
        assert subset == sorted(key(p) for p in o.pdus), r
        total_sub += len(subset)
        assert len(mine) >= 20, (r, len(mine))
    assert total_sub >= 16
    fe.close()


def test_every_fold_tiling_equals_the_fma_chain_with_receivers(gpu, monkeypatch):
    """Laboratory build: receivers of 70, 5 and 66 channels (full 64-channel workgroups, left-over octets and padding slots in each
    receiver) -- for the block counts of test_fold_mfma_equals_fma_chain every compiled tiling's partial sums equal the plain-VALU
    FMA-chain kernel's bit for bit (checksum over the bit patterns, the buffer poisoned before every kernel)."""
    lab = F.load_lab()
    fs = 2_048_000
    centres = [10_000_000, 11_500_000, 8_700_000]
    nchs = [70, 5, 66]
    recv = [(cf, [int(cf + (i - k // 2) * 14_000 + 3_000) for i in range(k)]) for cf, k in zip(centres, nchs)]
    monkeypatch.setenv("HFDL_GPU_FOLD_BATCH", "32")
    fe = gpu.MultiFrontend(fs, recv, lib=lab)
    assert fe.geometry.fold_batch == 32 and fe.geometry.channels == 141
    rng = np.random.default_rng(7)
    n = fe.input_size
    for b in range(32):
        fe.push_blocks([(rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64) * np.float32(0.1) for _ in recv])
    fe.sync()
    variants = F.fold_variants()
    ran = 0
    for nb in (1, 2, 3, 4, 5, 8, 11, 13, 16, 17, 21, 31, 32):
        ref = fe.fold_variant_probe(-1, nb, 1)[2]
        for v, (p, q, w, d, nbmax, layout) in enumerate(variants):
            if nb > nbmax or layout != 2:
                continue
            try:
                chk = fe.fold_variant_probe(v, nb, 1)[2]
            except gpu.GpuError:
                continue
            assert chk == ref, (nb, (p, q, w, d))
            ran += 1
    assert ran >= 13
    fe.close()


def _run_small(gpu, seq, fold_batch=None, monkeypatch=None):
    """Two receivers (3 + 2 channels, 2.048 Msps) through a call sequence: 'p' = push a step, 'P' = poll_pdus, 'R1' / 'R2' =
    poll_pdus_ready(.., 1 | 2), 'S' = sync.  Returns (sorted PDU keys, the channelizer output of the newest block per channel)."""
    if fold_batch is not None:
        monkeypatch.setenv("HFDL_GPU_FOLD_BATCH", str(fold_batch))
    fs = 2_048_000
    n = input_size_of(fs)
    centres, nchs = [10_000_000, 12_000_000], [3, 2]
    freqs, xs, _ = receiver_inputs(fs, centres, nchs, [51, 52], 24, n, grid=40_000)
    fe = gpu.MultiFrontend(fs, list(zip(centres, freqs)))
    if fold_batch is not None:
        monkeypatch.delenv("HFDL_GPU_FOLD_BATCH")
    pdus, b = [], 0
    for op in seq:
        if op == "p":
            fe.push_blocks([x[b * n:(b + 1) * n] for x in xs])
            b += 1
        elif op == "P":
            pdus += fe.poll_pdus()
        elif op in ("R1", "R2"):
            pdus += fe.poll_pdus(max_in_flight=int(op[1]))
        else:
            fe.sync()
    pdus += fe.poll_pdus()
    taps = [fe.read_tap(F.TAP_CHAN_OUT, c).tobytes() for c in range(sum(nchs))]
    fe.close()
    return sorted(pdu_full_key(p) + (p["receiver"],) for p in pdus), taps


def test_call_sequences_change_nothing(gpu, monkeypatch):
    """Random interleavings of pushes, polls, pipelined polls and syncs -- and HFDL_GPU_FOLD_BATCH=1 -- give the PDUs and taps of a
    poll after every step."""
    ref_pdus, ref_taps = _run_small(gpu, ["p", "P"] * 24)
    assert len(ref_pdus) >= 3
    rng = np.random.default_rng(5)
    seq = []
    for _ in range(24):
        seq.append("p")
        seq += list(rng.choice(["P", "R1", "R2", "S", "", ""], size=int(rng.integers(0, 3))))
    seq = [s for s in seq if s]
    assert _run_small(gpu, seq) == (ref_pdus, ref_taps)
    assert _run_small(gpu, ["p"] * 24, fold_batch=1, monkeypatch=monkeypatch) == (ref_pdus, ref_taps)
    assert _run_small(gpu, ["p"] * 24) == (ref_pdus, ref_taps)


def test_one_receiver_through_create_multi_is_create(gpu):
    """nrx = 1 through create_multi + push_blocks_raw is create + push_block_raw, bit for bit (PDUs, channelizer output, spectrum)."""
    fs = 2_048_000
    n = input_size_of(fs)
    freqs, xs, _ = receiver_inputs(fs, [10_000_000], [5], [61], 24, n, grid=50_000)
    raw = as_raw(xs[0], F.SFMT_CS16)
    a = gpu.MultiFrontend(fs, [(10_000_000, freqs[0])])
    b = gpu.Frontend(fs, 10_000_000, freqs[0])
    for k in range(24):
        blk = raw[2 * k * n:2 * (k + 1) * n]
        a.push_blocks_raw([blk], F.SFMT_CS16)
        b.push_block_raw(blk, F.SFMT_CS16)
    pa, pb = a.poll_pdus(), b.poll_pdus()
    assert len(pb) >= 2
    assert sorted(pdu_full_key(p) for p in pa) == sorted(pdu_full_key(p) for p in pb)
    assert all(p["receiver"] == 0 for p in pa)
    for c in range(5):
        assert a.read_tap(F.TAP_CHAN_OUT, c).tobytes() == b.read_tap(F.TAP_CHAN_OUT, c).tobytes()
    assert a.read_tap(F.TAP_SPECTRUM, 0).tobytes() == b.read_tap(F.TAP_SPECTRUM, 0).tobytes()
    ga, gb = a.geometry, b.geometry
    assert [getattr(ga, f) for f, _ in F.Geometry._fields_] == [getattr(gb, f) for f, _ in F.Geometry._fields_]
    a.close()
    b.close()


def test_misuse_and_the_memory_rule(gpu):
    """On nrx > 1 the one-stream entry points are EINVAL and enqueue nothing, a wrong block length is EINVAL; the next valid step
    after either gives what a run without the error gives.  Eight receivers at 40 Msps x 2 channels trip the memory rule
    (8 x 8 x 2^23 > 32 x 2^23): the reduced fold_batch / prefetch_depth are reported, and each receiver's channelizer output stays
    within the suite's relative RMS of its own front end (the slice counts differ: no bit identity)."""
    fs = 2_048_000
    n = input_size_of(fs)
    freqs, xs, _ = receiver_inputs(fs, [10_000_000, 12_000_000], [2, 3], [71, 72], 12, n, grid=40_000)
    recv = list(zip([10_000_000, 12_000_000], freqs))

    def run(with_errors):
        fe = gpu.MultiFrontend(fs, recv)
        L = fe._L
        for k in range(12):
            if with_errors and k in (3, 7):
                blk = np.ascontiguousarray(xs[0][k * n:(k + 1) * n])
                p = blk.ctypes.data
                assert L.hfdl_gpu_frontend_push_block(fe._h, p, n, 0) == -1
                assert L.hfdl_gpu_frontend_push_block_raw(fe._h, p, n, F.SFMT_CF32, 0) == -1
                assert L.hfdl_gpu_frontend_channelize_block(fe._h, p, n, 0) == -1
                assert L.hfdl_gpu_frontend_prefetch_block_raw(fe._h, p, n, F.SFMT_CF32) == -1
                assert L.hfdl_gpu_frontend_prefetch_cancel(fe._h) == -1
                assert b"receivers" in L.hfdl_gpu_last_error()
                with pytest.raises(gpu.GpuError):
                    fe.push_blocks_raw([x[k * n:(k + 1) * n].view(np.float32) for x in xs], F.SFMT_CF32, nsamples=n - 1)
                assert fe.counters()["blocks"] == k
            fe.push_blocks([x[k * n:(k + 1) * n] for x in xs])
        pd = sorted(pdu_full_key(p) for p in fe.poll_pdus())
        taps = [fe.read_tap(F.TAP_CHAN_OUT, c).tobytes() for c in range(5)] + [fe.read_tap(F.TAP_SPECTRUM, c).tobytes() for c in (0, 2)]
        fe.close()
        return pd, taps

    assert run(True) == run(False)

    # the memory rule: 8 receivers x 40 Msps x 2 channels
    fs, K = 40_000_000, 8
    centres = [8_000_000 + 3_000_000 * r for r in range(K)]
    recv = [(cf, [cf - 1_000_000 - 1440, cf + 2_000_000 - 1440]) for cf in centres]
    fe = gpu.MultiFrontend(fs, recv)
    g = fe.geometry
    one = gpu.Frontend(fs, centres[0], recv[0][1])
    g1 = one.geometry
    assert g.fft_size == 1 << 23 and g1.fold_batch == 8
    assert K * g.fold_batch * g.fft_size <= 32 << 23
    assert g.fold_batch == 4 and g.prefetch_depth < g1.prefetch_depth and g.demod_batch <= g.fold_batch
    rng = np.random.default_rng(9)
    n = g.input_size
    t = np.arange(n, dtype=np.float64)
    singles = [one] + [gpu.Frontend(fs, cf, fr) for cf, fr in recv[1:]]
    worst = 0.0
    for k in range(3):
        blocks = []
        for r, (cf, fr) in enumerate(recv):
            tone = 0.05 * np.exp(2j * np.pi * ((fr[r % 2] + 1440 + 300 - cf) / fs) * (t + k * n))
            blocks.append((tone + 0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64))
        fe.push_blocks(blocks)
        for s, blk in zip(singles, blocks):
            s.push_block(blk)
        fe.sync()
        for r, s in enumerate(singles):
            s.sync()
            for c in range(2):
                worst = max(worst, rel_rms(fe.read_tap(F.TAP_CHAN_OUT, 2 * r + c), s.read_tap(F.TAP_CHAN_OUT, c)))
    assert worst < RMS_TOL, worst
    fe.close()
    for s in singles:
        s.close()
