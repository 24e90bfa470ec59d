"""GPU tests of the channel baseband export (hfdl_gpu_frontend_export_enable / _read; export_pack_kernel in
dumphfdl_amd/csrc/spectrum_kernels.hip; include/hfdl_gpu.h "Channel baseband export").

What an exported row must be: the very words HFDL_GPU_TAP_CHAN_OUT reads for that block and channel, then +0.0 up to P -- so every
comparison of samples is on uint32 --, however the blocks were pushed, polled or batched.  The CS16 words and the clip count equal
tests/export_f64.py's conversion exactly; the row power equals its fp32 emulation bit for bit and lies within
(ceil(P / 256) + 8 + 3) 2^-23 relative of the float64 mean: one rounding per sequential add of a thread, eight tree levels, three for
the term and the division, all terms non-negative (derived, not measured).

250 ksps x 4 channels (N = 2^15), white noise plus one HFDL burst (hfdl_synth); a front end that starts fresh gives block k the same
words whatever else differs, so one reference pass (a sync after every push) is shared by the cases below."""
import os
import subprocess

import numpy as np
import pytest

import export_f64 as E
import hfdl_synth as synth
from dumphfdl_amd import frontend as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS, CF = 250_000, 10_000_000
FREQS = [9_930_000, 9_958_000, 10_037_000, 10_081_500]
SEL = [3, 1]                   # two of the four channels, in reversed order
NBLK, NALL = 21, 30            # blocks exported and compared; blocks of the whole stream (the burst ends behind block 21)
NTAP = 6


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def pdu_key(p):
    return (p["freq"], p["sample_index"], p["mode"], p["octets"], p["slot"], p["fcs_status"])


class Reference:
    """The stream, and the export of its first NBLK blocks collected one block at a time with a sync after every push (the taps of the
    first NTAP of them read at the same moment)."""

    def __init__(self, gpu):
        fe = gpu.Frontend(FS, CF, FREQS)
        g = fe.geometry
        self.n, self.P = g.input_size, g.max_outputs_per_block
        rng = np.random.default_rng(11)
        bursts = [dict(freq=FREQS[1], mode=1, octets=synth.make_pdu(rng, 1), t0=0.15, amp=0.1, cfo=6.0)]
        self.x = synth.synth_wideband(FS, CF, NALL * self.n, bursts, noise_sigma=0.004, seed=5).astype(np.complex64)
        fe.export_enable(SEL, ring_blocks=8)
        self.first = fe.counters()["blocks"]
        self.per_push, self.taps = [], []
        nxt = 0
        for b in range(NBLK):
            self.push(fe, b)
            fe.sync()
            got = fe.export_read(nxt, wait=True)
            nxt = got[5]
            self.per_push.append(got)
            if b < NTAP:
                self.taps.append([fe.read_tap(F.TAP_CHAN_OUT, c) for c in SEL])
        fe.poll_pdus()
        fe.close()
        self.samples = np.concatenate([g[0] for g in self.per_push])
        self.counts = np.concatenate([g[1] for g in self.per_push])
        self.power = np.concatenate([g[2] for g in self.per_push])
        self.clipped = np.concatenate([g[3] for g in self.per_push])

    def push(self, fe, b):
        fe.push_block(self.x[b * self.n:(b + 1) * self.n])

    def same(self, got, blocks):
        """got = an export_read tuple holding exactly `blocks` of the reference pass, word for word"""
        blocks = list(blocks)
        return (got[4] == blocks and np.array_equal(u32(got[0]), u32(self.samples[blocks])) and np.array_equal(got[1], self.counts[blocks])
                and np.array_equal(u32(got[2]), u32(self.power[blocks])) and np.array_equal(got[3], self.clipped[blocks]))


@pytest.fixture(scope="module")
def ref(gpu):
    return Reference(gpu)


def test_export_equals_the_tap_bit_for_bit(ref):
    """Case 1: after each push and sync, export_read(wait=True) returns that block; its rows are the taps' words, counts the taps'
    lengths, the padding up to P is +0.0; CF32 never clips."""
    for b, got in enumerate(ref.per_push):
        samples, counts, power, clipped, blocks, nxt = got
        assert blocks == [ref.first + b] and nxt == ref.first + b + 1 and samples.shape == (1, len(SEL), ref.P) and samples.dtype == np.complex64
        assert (clipped == 0).all() and (counts > 0).all() and (counts <= ref.P).all()
        for s in range(len(SEL)):
            k = counts[0, s]
            assert not u32(samples[0, s, k:]).any()
            if b < NTAP:
                tap = ref.taps[b][s]
                assert len(tap) == k and np.array_equal(u32(samples[0, s, :k]), u32(tap)), (b, s)
    # the two rows are different channels, and the burst is in one of them
    assert ref.power[:, 1].max() > 10 * ref.power[:, 0].max()


def test_batching_changes_nothing(gpu, ref, monkeypatch):
    """Case 2: the same 21 blocks pushed without a poll into halves of 16 (fold launches of 16 and 5, one export launch each) export the
    same bytes; and the PDUs of the whole stream are the same with the export on and off."""
    monkeypatch.setenv("HFDL_GPU_FOLD_BATCH", "16")
    pdus = {}
    for on in (True, False):
        fe = gpu.Frontend(FS, CF, FREQS)
        assert fe.geometry.fold_batch == 16
        fe.reset_timers(True)
        if on:
            fe.export_enable(SEL, ring_blocks=32)
        for b in range(NBLK):
            ref.push(fe, b)
        if on:
            early = fe.export_read(0, wait=True)                # closes nothing: the half of 16 at most, never the 5 still waiting
            assert early[4] == list(range(16)) and ref.same(early, range(16))
        fe.sync()
        assert fe.fold_launch_shapes() == {16: 1, 5: 1}
        if on:
            got = fe.export_read(0, wait=False)                 # after a sync everything has run: nothing to wait for
            assert got[5] == NBLK and ref.same(got, range(NBLK))
        for b in range(NBLK, NALL):
            ref.push(fe, b)
        pdus[on] = [pdu_key(p) for p in fe.poll_pdus()]
        fe.close()
    assert len(pdus[False]) >= 1 and pdus[True] == pdus[False]


def test_ring_wrap_and_loss(gpu, ref, monkeypatch):
    """Case 3: R = 4, ten blocks pushed one by one and nothing read: from_block = 0 returns blocks 6 .. 9; a half of 5 blocks into R = 4
    keeps its blocks 1 .. 4."""
    fe = gpu.Frontend(FS, CF, FREQS)
    fe.export_enable(SEL, ring_blocks=4)
    for b in range(10):
        ref.push(fe, b)
        fe.sync()
    got = fe.export_read(0)
    assert got[4][0] == 6 and got[5] == 10 and ref.same(got, range(6, 10))
    assert ref.same(fe.export_read(8, max_blocks=1), [8])
    none = fe.export_read(0, max_blocks=0)
    assert none[4] == [] and none[5] == 6 and none[0].shape == (0, len(SEL), ref.P)
    fe.close()
    monkeypatch.setenv("HFDL_GPU_FOLD_BATCH", "16")
    fe = gpu.Frontend(FS, CF, FREQS)
    fe.reset_timers(True)
    fe.export_enable(SEL, ring_blocks=4)
    for b in range(5):
        ref.push(fe, b)
    assert fe.fold_launch_shapes() == {5: 1} and fe.counters()["blocks"] == 5        # (reading the shapes syncs)
    got = fe.export_read(0, wait=True)
    assert got[5] == 5 and ref.same(got, range(1, 5))
    fe.close()


def test_collecting_without_waiting(gpu, ref):
    """Case 4: wait=False after every push, one wait=True after the final sync: every block exactly once, in order, the reference's
    words; no call returns a block that has not been pushed."""
    fe = gpu.Frontend(FS, CF, FREQS)
    fe.export_enable(SEL, ring_blocks=32)
    parts, nxt = [], 0
    for b in range(NBLK):
        ref.push(fe, b)
        got = fe.export_read(nxt, wait=False)
        assert all(k < fe.counters()["blocks"] for k in got[4]) and got[5] <= fe.counters()["blocks"]
        nxt = got[5]
        parts.append(got)
    fe.sync()
    parts.append(fe.export_read(nxt, wait=True))
    assert parts[-1][5] == NBLK
    whole = tuple(np.concatenate([p[i] for p in parts]) for i in range(4)) + (sum((p[4] for p in parts), []), NBLK)
    assert ref.same(whole, range(NBLK))
    fe.poll_pdus()
    fe.close()


def test_enable_boundary(gpu, ref):
    """Case 5: two blocks pushed and still waiting in the open half, enable, two more, sync: exactly the last two are exported.
    Enabling again with another selection starts over with an empty ring at the current block count."""
    fe = gpu.Frontend(FS, CF, FREQS)
    ref.push(fe, 0)
    ref.push(fe, 1)
    fe.export_enable(SEL, ring_blocks=8)
    none = fe.export_read(0, wait=True)
    assert none[4] == [] and none[5] == 2
    ref.push(fe, 2)
    ref.push(fe, 3)
    fe.sync()
    got = fe.export_read(0, wait=True)
    assert got[5] == 4 and ref.same(got, [2, 3])
    fe.export_enable([0, 2, 1], ring_blocks=2)
    got = fe.export_read(0, wait=True)
    assert got[4] == [] and got[5] == 4 == fe.counters()["blocks"] and got[0].shape == (0, 3, ref.P)
    ref.push(fe, 4)
    fe.sync()
    got = fe.export_read(0)
    assert got[4] == [4] and np.array_equal(u32(got[0][0, 2]), u32(ref.samples[4, 1]))          # channel 1 is row 2 now, row 1 of the reference
    with pytest.raises(F.GpuError):
        fe.export_enable([0, 0], ring_blocks=8)
    with pytest.raises(F.GpuError):
        fe.export_enable([4], ring_blocks=8)
    with pytest.raises(F.GpuError):
        fe.export_enable([0], fmt="cs16", scale=float("inf"), ring_blocks=8)
    with pytest.raises(F.GpuError):
        fe.export_enable([0], ring_blocks=F.EXPORT_RING_MAX + 1)
    assert fe.export_read(0)[4] == [4]                          # a refused call leaves the export as it was
    fe.export_enable([])
    with pytest.raises(F.GpuError):
        fe.export_read(0)
    fe.poll_pdus()
    fe.close()


def test_cs16(gpu, ref):
    """Case 6: the int16 words and the clip counts are the numpy definition's, exactly, with a scale at which some but not all
    components clip (32767 / the 99th percentile of |component| of the CF32 export); at scale 1.0 nothing clips."""
    comp = np.abs(ref.samples.view(np.float32))
    scale = float(np.float32(32767.0 / np.percentile(comp[comp > 0], 99)))
    for sc in (scale, 1.0):
        fe = gpu.Frontend(FS, CF, FREQS)
        fe.export_enable(SEL, fmt="cs16", scale=sc, ring_blocks=32)
        for b in range(NBLK):
            ref.push(fe, b)
        fe.sync()
        samples, counts, power, clipped, blocks, nxt = fe.export_read(0, wait=True)
        fe.poll_pdus()
        fe.close()
        want, nclip = E.cs16(ref.samples, sc)
        assert blocks == list(range(NBLK)) and samples.dtype == np.int16 and samples.shape == (NBLK, len(SEL), ref.P, 2)
        assert np.array_equal(samples, want) and np.array_equal(clipped, nclip)
        assert np.array_equal(counts, ref.counts) and np.array_equal(u32(power), u32(ref.power))       # the power is of the fp32 samples
        print("cs16 scale %g: %d of %d components clipped" % (sc, int(clipped.sum()), 2 * int(counts.sum())))
        if sc == 1.0:
            assert (clipped == 0).all()
        else:
            assert 0 < clipped.sum() < 2 * counts.sum() and (np.abs(samples) == 32767).any()


def test_power(gpu, ref):
    """Case 7: every exported row's power is the fp32 emulation's word and lies within the derived gate of the float64 mean (measured on
    an MI355X: worst |error| / gate 0.078 at P = 896); a block of exact zeros gives 0.0."""
    gate = E.power_gate(ref.P)
    worst = 0.0
    for b in range(NBLK):
        for s in range(len(SEL)):
            row = ref.samples[b, s, :ref.counts[b, s]]
            emu, p64 = E.power_f32(row), E.power_f64(row)
            assert ref.power[b, s].view(np.uint32) == emu.view(np.uint32), (b, s, float(ref.power[b, s]), float(emu))
            worst = max(worst, abs(float(ref.power[b, s]) - p64) / (gate * p64))
    print("power: worst |error| / gate %.3f (gate %.3g relative, P = %d)" % (worst, gate, ref.P))
    assert worst <= 1.0
    fe = gpu.Frontend(FS, CF, FREQS)
    fe.export_enable(SEL, ring_blocks=4)
    for _ in range(2):
        fe.push_block(np.zeros(ref.n, np.complex64))
    fe.sync()
    samples, counts, power, clipped, blocks, nxt = fe.export_read(0, wait=True)
    assert blocks == [0, 1] and (counts > 0).all() and not u32(power).any() and not (samples != 0).any()
    fe.poll_pdus()
    fe.close()


def test_two_receivers(gpu, ref):
    """Case 8: MultiFrontend, 2 receivers x 2 channels; one channel of each selected (global indices): both rows equal their taps."""
    centres = [CF, 11_300_000]
    freqs = [[9_958_000, 10_037_000], [11_262_000, 11_348_000]]
    fe = gpu.MultiFrontend(FS, list(zip(centres, freqs)))
    sel = [2, 1]
    fe.export_enable(sel, ring_blocks=4)
    y = np.roll(ref.x, 12345) * np.complex64(0.5)
    nxt = 0
    for b in range(3):
        fe.push_blocks([ref.x[b * ref.n:(b + 1) * ref.n], y[b * ref.n:(b + 1) * ref.n]])
        fe.sync()
        samples, counts, power, clipped, blocks, nxt = fe.export_read(nxt, wait=True)
        assert blocks == [b]
        for s, c in enumerate(sel):
            tap = fe.read_tap(F.TAP_CHAN_OUT, c)
            assert counts[0, s] == len(tap) and np.array_equal(u32(samples[0, s, :len(tap)]), u32(tap)) and not u32(samples[0, s, len(tap):]).any()
            assert power[0, s].view(np.uint32) == E.power_f32(tap).view(np.uint32)
    fe.poll_pdus()
    fe.close()


def test_replay_writes_channel_files(gpu, tmp_path):
    """Case 9: hfdl_replay --iq-export-dir on a cs16 recording: each <freq>.cf32 is the concatenation of the channel's tap over the same
    blocks of a Python run over the same file, byte for byte (a .cs16 likewise, through the definition); the PDUs on stdout are those of
    a run without the option.  The Python run reads the newest block's tap after every push (read_tap, which is read_tap_block with
    back = 0; the read syncs, so it makes one block per half) where the program batches its halves: the same words either way."""
    freqs = FREQS[:3]
    probe = gpu.Frontend(FS, CF, freqs)
    n = probe.input_size
    nblk = 29
    rng = np.random.default_rng(4)
    bursts = [dict(freq=freqs[1], mode=1, octets=synth.make_pdu(rng, 1), t0=0.15, amp=0.1, cfo=6.0)]
    x = synth.synth_wideband(FS, CF, nblk * n + n // 3, bursts, noise_sigma=0.004, seed=9)          # the last third of a block is never pushed
    raw = np.clip(np.round(x.astype(np.complex64).view(np.float32) * 20000), -32768, 32767).astype(np.int16)
    want = [[] for _ in freqs]
    for b in range(nblk):
        probe.push_block_raw(raw[2 * b * n:2 * (b + 1) * n], F.SFMT_CS16)
        for c in range(len(freqs)):
            want[c].append(probe.read_tap(F.TAP_CHAN_OUT, c))
    probe.poll_pdus()
    probe.close()
    want = [np.concatenate(w) for w in want]
    path = tmp_path / "iq.cs16"
    raw.tofile(path)
    exe = os.path.join(ROOT, "dumphfdl_amd", "hfdl_replay")
    base = [exe, "--iq-file", str(path), "--sample-rate", str(FS), "--sample-format", "CS16", "--centerfreq", str(CF / 1e3)]
    chans = ["%.3f" % (f / 1e3) for f in freqs]

    def pdus(out):        # every field but the wall-clock timestamp
        return sorted(" ".join(t for t in l.split() if not t.startswith("ts=")) for l in out.splitlines() if l.startswith("PDU "))
    plain = subprocess.run(base + chans, capture_output=True, text=True, timeout=300)
    d32, d16 = tmp_path / "cf32", tmp_path / "cs16"
    d32.mkdir()
    d16.mkdir()
    exp = subprocess.run(base + ["--iq-export-dir", str(d32)] + chans, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and exp.returncode == 0, exp.stderr
    assert len(pdus(plain.stdout)) >= 1 and pdus(plain.stdout) == pdus(exp.stdout)
    assert sorted(os.listdir(d32)) == sorted("%d.cf32" % f for f in freqs)
    for c, f in enumerate(freqs):
        got = np.fromfile(d32 / ("%d.cf32" % f), np.complex64)
        assert len(got) == len(want[c]) and np.array_equal(u32(got), u32(want[c])), f
    scale = 20000.0
    exp = subprocess.run(base + ["--iq-export-dir", str(d16), "--iq-export-format", "cs16", "--iq-export-scale", str(scale)] + chans,
                         capture_output=True, text=True, timeout=300)
    assert exp.returncode == 0 and pdus(plain.stdout) == pdus(exp.stdout), exp.stderr
    for c, f in enumerate(freqs):
        got = np.fromfile(d16 / ("%d.cs16" % f), np.int16).reshape(-1, 2)
        assert np.array_equal(got, E.cs16(want[c], scale)[0]), f
