"""Device-resident blocks have their forward FFT on the input stream, beside the fold of the half before (planner.h FftOrder); uploaded
blocks keep theirs on the fold's stream.  Where a kernel runs changes nothing it computes: every case compares a run that pushes device
pointers (or a mix) with the SAME call sequence pushed from host memory -- the path the oracle tests pin -- in every field of every PDU,
the channelizer output as uint32 and every channel statistic."""
import ctypes

import numpy as np
import pytest

import hfdl_synth as synth
from dumphfdl_amd import frontend as F

pytestmark = pytest.mark.gpu

FS, CF = 250000, 10_000_000
FREQS = [9_915_000, 9_972_000, 10_026_000, 10_083_000, 10_101_000]
N_SMALL = 28672


def by_time(pdus):
    return sorted(pdus, key=lambda p: (p["freq"], p["sample_index"]))


def on_device(x):
    """The stream in HBM and one pointer per block of n samples (keep the tensor alive while the pointers are in use)."""
    import torch
    dev = torch.from_numpy(np.ascontiguousarray(x).view(np.float32).copy()).cuda()
    torch.cuda.synchronize()
    return dev, lambda b, n: dev.data_ptr() + 8 * b * n


@pytest.fixture(scope="module")
def dense():
    """250 ksps, 5 channels, 10 s of dense traffic (the stream of test_fft_stream_switch_changes_nothing): 87 blocks of 28 672 samples."""
    bursts = synth.plan_traffic(FREQS, 10.0, seed=61, dense=True, gap_s=0.12, amp=(0.02, 0.1))
    return synth.synth_wideband(FS, CF, int(10.0 * FS), bursts, noise_sigma=0.012, seed=61), bursts


def switch_sequence(gpu, x, block, poll_every_block=False):
    """The call sequence of the stream-switch test: a draining poll every 11th block, a lagging one every 5th, one channelize-only block."""
    fe = gpu.Frontend(FS, CF, FREQS)
    n, got, outs = fe.input_size, [], []
    assert n == N_SMALL
    for b in range(len(x) // n):
        if b == 20:
            fe.channelize_block(block(b, n))            # never demodulated
            outs.append(fe.read_tap(F.TAP_CHAN_OUT, 3).view(np.uint32).copy())
            continue
        fe.push_block(block(b, n))
        if poll_every_block:
            got += fe.poll_pdus()
        elif b % 11 == 4:
            got += fe.poll_pdus()                       # a draining poll: a ragged half
            outs.append(fe.read_tap(F.TAP_CHAN_OUT, 1).view(np.uint32).copy())
        elif b % 5 == 0:
            got += fe.poll_pdus(max_in_flight=1)
    got += fe.poll_pdus()
    outs.append(fe.read_tap(F.TAP_CHAN_OUT, 4).view(np.uint32).copy())
    stats = fe.all_channel_stats()
    fe.close()
    return by_time(got), outs, stats


def test_device_blocks_equal_host_blocks(gpu, dense):
    """Case 1: every block a device pointer -- full halves, ragged cuts, lagging collections, a channelize-only block -- against the
    host-pushed run, and against device pushes with a poll after every block (one block per launch of everything)."""
    x, bursts = dense
    ref, ref_outs, ref_stats = switch_sequence(gpu, x, lambda b, n: x[b * n:(b + 1) * n])
    dev, ptr = on_device(x)
    got, outs, stats = switch_sequence(gpu, x, ptr)
    assert len(ref) >= len(bursts) - 3 and got == ref and stats == ref_stats
    assert len(outs) == len(ref_outs) and all(np.array_equal(a, b) for a, b in zip(outs, ref_outs))
    got, outs, stats = switch_sequence(gpu, x, ptr, poll_every_block=True)
    assert got == ref and stats == ref_stats
    assert len(outs) == 2 and np.array_equal(outs[0], ref_outs[2]) and np.array_equal(outs[1], ref_outs[-1])      # the channelize-only block (behind the polls at blocks 4 and 15), the last block
    del dev


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_mixed_host_device_and_prefetched_blocks(gpu, dense, seed):
    """Case 2: each block at random a host array, a device pointer or a prefetched page-locked pointer (now and then two or three
    prefetches queued ahead), polls / syncs / statistics / tap reads at random behind each push: the forward FFTs change streams all the
    time, uploads queue behind device blocks' FFTs and the other way round."""
    x, _ = dense
    nblk = len(x) // N_SMALL
    rng = np.random.default_rng(seed)
    kinds, b = [], 0
    while b < nblk:
        k = str(rng.choice(["host", "dev", "dev", "pinned"]))
        run = int(rng.integers(2, 4)) if k == "pinned" and rng.random() < 0.5 else 1
        run = min(run, nblk - b)
        kinds += [(k, run - j) for j in range(run)]       # (kind, blocks of the prefetch run from here on)
        b += run
    acts = [str(rng.choice(["none", "none", "none", "lag", "lag", "drain", "sync", "stats", "tap"])) for _ in range(nblk)]
    dev, ptr = on_device(x)
    raw = np.ascontiguousarray(x[:nblk * N_SMALL]).view(np.float32)
    pinned = gpu.host_alloc(raw.nbytes)
    ctypes.memmove(pinned, raw.ctypes.data, raw.nbytes)

    def run(mixed):
        fe = gpu.Frontend(FS, CF, FREQS)
        n, got, outs, queued = fe.input_size, [], [], 0
        assert fe.geometry.prefetch_depth >= 3
        for b in range(nblk):
            kind, left = kinds[b] if mixed else ("host", 1)
            if kind == "host":
                fe.push_block(x[b * n:(b + 1) * n])
            elif kind == "dev":
                fe.push_block(ptr(b, n))
            else:
                if queued == 0:                          # the whole run is queued ahead of its first push
                    for j in range(left):
                        fe.prefetch_host_ptr(pinned + 8 * (b + j) * n)
                    queued = left
                fe.push_host_ptr(pinned + 8 * b * n)
                queued -= 1
            act = acts[b]
            if act == "lag":
                got += fe.poll_pdus(max_in_flight=1)
            elif act == "drain":
                got += fe.poll_pdus()
            elif act == "sync":
                fe.sync()
            elif act == "stats":
                fe.all_channel_stats()
            elif act == "tap":
                outs.append(fe.read_tap(F.TAP_CHAN_OUT, 1).view(np.uint32).copy())
        got += fe.poll_pdus()
        outs.append(fe.read_tap(F.TAP_CHAN_OUT, 2).view(np.uint32).copy())
        stats, cnt = fe.all_channel_stats(), fe.counters()
        fe.close()
        assert cnt["pdus_dropped"] == 0 and cnt["pdus_taken"] == len(got)
        return by_time(got), outs, stats

    try:
        ref, ref_outs, ref_stats = run(False)
        got, outs, stats = run(True)
    finally:
        gpu.host_free(pinned)
    assert {k for k, _ in kinds} == {"host", "dev", "pinned"} and any(r > 1 for _, r in kinds)
    assert len(ref) >= 8 and got == ref and stats == ref_stats
    assert len(outs) == len(ref_outs) and all(np.array_equal(a, b) for a, b in zip(outs, ref_outs))
    del dev


@pytest.fixture(scope="module")
def fold_bound(gpu):
    """Case 3's geometry and its reference.  128 channels at 1 Msps on a 7 kHz grid: decimation 128, N = 131 072, blocks of 114 688 samples,
    128 MiB of filter taps; the fold bounds the block (128 channels), a half holds 32 blocks and the first one after a drain 16.  Bursts on
    five channels.  68 blocks without a poll, then one: fold launches of 16, 32, 16 and 4 blocks."""
    fs, cf, nch, nblk = 1_000_000, 10_000_000, 128, 68
    freqs = [int(cf + (i - nch // 2) * 7_000 + 2_000) for i in range(nch)]
    rng = np.random.default_rng(16)
    bursts = [dict(freq=freqs[c], mode=int(rng.integers(0, 4)), octets=b"", t0=float(rng.uniform(0.2, 4.5)), amp=0.03, cfo=float(rng.uniform(-10, 10)))
              for c in (2, 41, 64, 99, 127)]
    for b in bursts:
        b["octets"] = synth.make_pdu(rng, b["mode"])
    n = 114688
    x = synth.synth_wideband(fs, cf, nblk * n, bursts, noise_sigma=0.01, seed=16)
    dev, ptr = on_device(x)

    def run(host_at):
        """Device pointers, but the blocks in `host_at` from host memory (None: every block from host memory)."""
        fe = gpu.Frontend(fs, cf, freqs)
        g = fe.geometry
        assert (g.channels, g.fft_size, g.input_size, g.fold_batch, g.decimation) == (nch, 131072, n, 32, 128)
        assert g.demod_batch >= 2
        fe.reset_timers(True)
        for b in range(nblk):
            fe.push_block(x[b * n:(b + 1) * n] if host_at is None or b in host_at else ptr(b, n))
        got = fe.poll_pdus()
        shapes, ffts = fe.fold_launch_shapes(), fe.stage_times()["fft"][1]
        fe.reset_timers(False)
        outs = [fe.read_tap(F.TAP_CHAN_OUT, c, back=k).view(np.uint32).copy() for c in (2, 64, 127) for k in (0, 3)]
        stats = fe.all_channel_stats()
        fe.close()
        return by_time(got), outs, stats, shapes, ffts

    ref = run(None)
    assert len(ref[0]) >= len(bursts) - 1 and ref[3] == {16: 2, 32: 1, 4: 1} and ref[4] == nblk
    yield run, ref
    del dev


@pytest.mark.parametrize("host_at", [(), (15,), (16,), (47,)], ids=["device", "host15", "host16", "host47"])
def test_fold_bound_halves_with_device_blocks(fold_bound, host_at):
    """Case 3: where the fold bounds the block, a half's demodulators are held back behind the next half's forward FFTs -- if those run
    in front of the fold.  Device blocks launch them at once; a host block as the last of the first half (15), the first of the second
    (16) and the last of the second (47) sits where the hold-back and the change of stream meet.  Same launches (16, 32, 16, 4; one timed
    forward FFT per block whichever stream it ran on), same PDUs, output and statistics."""
    run, (ref, ref_outs, ref_stats, ref_shapes, ref_ffts) = fold_bound
    got, outs, stats, shapes, ffts = run(set(host_at))
    assert shapes == {16: 2, 32: 1, 4: 1} and ffts == 68
    assert got == ref and stats == ref_stats
    assert all(len(a) and np.array_equal(a, b) for a, b in zip(outs, ref_outs))


def test_spectrum_monitor_with_device_blocks(gpu):
    """Case 4: the monitor's launch follows the forward FFT onto the input stream.  Band powers (mean and peak, as uint32) of device
    pushes equal those of host pushes at reads inside a half, across halves and after a drain; one receiver, and two receivers fed with
    push_blocks of device pointers."""
    from test_gpu_spectrum import stream_for, u32
    nblk, reads = 24, (0, 4, 9, 20, 23)

    def run(make, push_of, nrx):
        fe = make()
        push = push_of(fe)
        fe.spectrum_enable(64, hann=True, maxhold=True)
        out = []
        for b in range(nblk):
            push(b)
            if b == 12:
                fe.poll_pdus()
            if b in reads:
                for r in range(nrx):
                    s = fe.spectrum_read(r, reset=(b == 9))
                    out.append((s["blocks"], u32(s["mean"]).copy(), u32(s["peak"]).copy()))
        pdus = by_time(fe.poll_pdus())
        fe.close()
        return out, pdus

    def same(a, b):
        assert a[1] == b[1] and len(a[0]) == len(b[0])
        for (ta, ma, pa), (tb, mb, pb) in zip(a[0], b[0]):
            assert ta == tb and ma.any() and np.array_equal(ma, mb) and np.array_equal(pa, pb)

    fs, cf, freqs = 250_000, 10_000_000, [10_040_000]
    probe = gpu.Frontend(fs, cf, freqs)
    n = probe.input_size
    x = stream_for(probe, fs, cf, freqs[0], seed=161, nblk=nblk)
    probe.close()
    dev, ptr = on_device(x)
    one = lambda: gpu.Frontend(fs, cf, freqs)
    same(run(one, lambda fe: (lambda b: fe.push_block(ptr(b, n))), 1), run(one, lambda fe: (lambda b: fe.push_block(x[b * n:(b + 1) * n])), 1))

    fs2, centres = 2_048_000, [10_000_000, 11_300_000]
    freqs2 = [[c + 50_000 + 15_000 * i for i in range(k)] for c, k in zip(centres, (1, 2))]
    two = lambda: gpu.MultiFrontend(fs2, list(zip(centres, freqs2)))
    probe = two()
    n2 = probe.input_size
    xs = [stream_for(probe, fs2, c, fr[0], seed=162 + r, nblk=nblk) for r, (c, fr) in enumerate(zip(centres, freqs2))]
    probe.close()
    devs = [on_device(xr) for xr in xs]
    same(run(two, lambda fe: (lambda b: fe.push_blocks([p(b, n2) for _, p in devs])), 2),
         run(two, lambda fe: (lambda b: fe.push_blocks([xr[b * n2:(b + 1) * n2] for xr in xs])), 2))
    del dev, devs


def test_blocks_produced_on_the_frontend_stream(gpu, dense):
    """Case 5, the contract of hfdl_gpu_frontend_stream(): device input must be complete on, or ordered with, that stream.  Every block is
    produced ON it -- one device-side copy per block into a buffer that held zeros -- and pushed at once, without a host synchronisation
    between the copy and the push or between the blocks; a forward FFT that read its input early would transform zeros."""
    import torch
    x, _ = dense
    n = N_SMALL
    nblk = len(x) // n

    def run(produced):
        fe = gpu.Frontend(FS, CF, FREQS)
        assert fe.input_size == n
        if produced:
            src = torch.from_numpy(np.ascontiguousarray(x[:nblk * n]).view(np.float32).copy()).cuda().view(nblk, 2 * n)
            dst = torch.zeros_like(src)
            torch.cuda.synchronize()
            st = torch.cuda.ExternalStream(fe.stream())
            for b in range(nblk):
                with torch.cuda.stream(st):
                    dst[b].copy_(src[b], non_blocking=True)
                fe.push_block(dst.data_ptr() + 8 * b * n)
        else:
            for b in range(nblk):
                fe.push_block(x[b * n:(b + 1) * n])
        got = by_time(fe.poll_pdus())
        outs = [fe.read_tap(F.TAP_CHAN_OUT, c, back=k).view(np.uint32).copy() for c in (0, 4) for k in (0, 2)]
        stats = fe.all_channel_stats()
        fe.close()
        return got, outs, stats

    ref, ref_outs, ref_stats = run(False)
    got, outs, stats = run(True)
    assert len(ref) >= 8 and got == ref and stats == ref_stats
    assert all(len(a) and np.array_equal(a, b) for a, b in zip(outs, ref_outs))
