"""GPU tests of retuning a channel of a running front end (hfdl_gpu_frontend_retune_channel; retune_channelizer_kernel in
dumphfdl_amd/csrc/fft_kernels.hip, retune_demod_kernel and retune_freq_kernel in demod_kernels.hip).

What a retune must be: blocks pushed before the call run on the old frequency, blocks pushed after it on the new one, where the
channel is a freshly created channel -- so everything here is compared as uint32 words or as whole PDUs, never within a tolerance.

250 ksps x 4 channels (N = 2^15), channel C = 1 moves from F_OLD to F_NEW at block K.  The stream: blocks 0 .. K - 2 white noise with
an HFDL burst on F_OLD that ends inside them, block K - 1 all zeros (the overlap history at the boundary is then what a front end
starts with), from block K on noise with a burst on F_NEW (hfdl_synth, amplitude 0.1, sigma 0.004; both bursts decode alone in the
oracle at these seeds).  Three passes are made once and shared: A (retune at K, a sync after every push), B (created with F_NEW,
blocks K .. end only) and A' (no retune)."""
import os
import subprocess

import numpy as np
import pytest

import hfdl_synth as synth
from dumphfdl_amd import frontend as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FS, CF = 250_000, 10_000_000
FREQS = [9_930_000, 9_958_000, 10_037_000, 10_081_500]
CH = 1
F_OLD, F_NEW = FREQS[CH], 10_003_300           # F_NEW: inside +-fs/2, on no other channel's grid
K, NALL = 25, 50                               # the boundary (odd: a multiple of no batch size); blocks of the whole stream
EINVAL = -1


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def pdu_key(p):
    return (p["freq"], p["sample_index"], p["mode"], p["octets"], p["slot"], p["fcs_status"])


def with_freq(freqs, c, f):
    out = list(freqs)
    out[c] = f
    return out


def make_stream(n, k, nall, bursts_before, bursts_after, seed):
    """blocks 0 .. k - 2: noise + bursts_before; block k - 1: zeros; blocks k ..: noise + bursts_after (their t0 counts from block k)"""
    head = synth.synth_wideband(FS, CF, (k - 1) * n, bursts_before, noise_sigma=0.004, seed=seed).astype(np.complex64)
    tail = synth.synth_wideband(FS, CF, (nall - k) * n, bursts_after, noise_sigma=0.004, seed=seed + 1).astype(np.complex64)
    return np.concatenate([head, np.zeros(n, np.complex64), tail])


def the_stream(n):
    rng = np.random.default_rng(23)
    before = [dict(freq=F_OLD, mode=1, octets=synth.make_pdu(rng, 1), t0=0.12, amp=0.1, cfo=6.0)]
    after = [dict(freq=F_NEW, mode=3, octets=synth.make_pdu(rng, 3), t0=0.12, amp=0.1, cfo=-9.0)]
    return make_stream(n, K, NALL, before, after, seed=5)


class Pass:
    """One run over blocks [first, last) of x: retunes = {block: (channel, freq)} applied before that block is pushed.  Every channel's
    TAP_CHAN_OUT words of every block come from the export (a ring as long as the stream); `taps`: also read TAP_CHAN_OUT and TAP_NCO_PHASORS of
    channel CH after every block (needs sync_each)."""

    def __init__(self, gpu, x, freqs, first, last, retunes=None, sync_each=False, taps=False, on_device=False, fe=None, push=None):
        retunes = retunes or {}
        fe = fe or gpu.Frontend(FS, CF, freqs)
        n = fe.input_size
        nch = fe.geometry.channels
        fe.export_enable(list(range(nch)), ring_blocks=max(64, last - first))
        self.filters_before = self.filters_after = None
        self.boundary_cnt = {}
        self.chan_out, self.phasors = [], []
        dev = None
        if on_device:
            import torch
            dev = torch.from_numpy(np.ascontiguousarray(x).view(np.float32).copy()).cuda()
            torch.cuda.synchronize()
        for b in range(first, last):
            if b in retunes:
                c, f = retunes[b]
                if taps:
                    self.filters_before = [fe.read_tap(F.TAP_FILTER, i) for i in range(nch)]
                    self.boundary_cnt[b] = fe.channel_stats(c)["sample_cnt"]
                fe.retune(c, f)
                if taps:
                    fe.sync()
                    self.filters_after = [fe.read_tap(F.TAP_FILTER, i) for i in range(nch)]
                    assert fe.channel_stats(c)["freq"] == f
            if push:
                push(fe, b)
            elif on_device:
                fe.push_block(dev.data_ptr() + 8 * b * n)
            else:
                fe.push_block(x[b * n:(b + 1) * n])
            if sync_each:
                fe.sync()
            if taps:
                self.chan_out.append(fe.read_tap(F.TAP_CHAN_OUT, CH))
                self.phasors.append(fe.read_tap(F.TAP_NCO_PHASORS, CH))
        self.pdus = fe.poll_pdus()
        samples, counts, _, _, blocks, _ = fe.export_read(0, wait=True)
        assert blocks == list(range(last - first))
        self.words, self.counts = u32(samples), counts       # [block][channel][P]
        self.stats = fe.all_channel_stats()
        self.fe = fe

    def close(self):
        self.fe.close()


class Shared:
    def __init__(self, gpu):
        probe = gpu.Frontend(FS, CF, FREQS)
        self.n = probe.input_size
        self.create_filters = [probe.read_tap(F.TAP_FILTER, i) for i in range(len(FREQS))]
        probe.close()
        self.x = the_stream(self.n)
        self.A = Pass(gpu, self.x, FREQS, 0, NALL, {K: (CH, F_NEW)}, sync_each=True, taps=True)
        self.B = Pass(gpu, self.x, with_freq(FREQS, CH, F_NEW), K, NALL, sync_each=True, taps=True)
        self.B_filters = [self.B.fe.read_tap(F.TAP_FILTER, i) for i in range(len(FREQS))]
        self.A1 = Pass(gpu, self.x, FREQS, 0, NALL, sync_each=True)
        for p in (self.A, self.B, self.A1):
            p.close()


@pytest.fixture(scope="module")
def sh(gpu):
    return Shared(gpu)


def test_taps_are_a_fresh_creates(sh):
    """1: after retune + sync the filter of the retuned channel equals, as uint32, that of a front end created with F_NEW in its place;
    every other channel's equals what it was before the retune (and at create)."""
    A = sh.A
    assert np.array_equal(u32(A.filters_after[CH]), u32(sh.B_filters[CH]))
    assert not np.array_equal(u32(A.filters_after[CH]), u32(A.filters_before[CH]))
    for c in range(len(FREQS)):
        assert np.array_equal(u32(A.filters_before[c]), u32(sh.create_filters[c]))
        if c != CH:
            assert np.array_equal(u32(A.filters_after[c]), u32(A.filters_before[c])), c
            assert np.array_equal(u32(A.filters_after[c]), u32(sh.B_filters[c])), c


def test_a_fresh_channel_bit_for_bit(sh):
    """2: from the boundary on, channel CH of A is channel CH of B (created with F_NEW, pushed blocks K .. end only): channelizer output,
    its count and the NCO phasors of every block as uint32; every PDU field except sample_index, which differs by exactly A's
    sample_cnt at the boundary.  At least one PDU with a good FCS on each side of the boundary."""
    A, B = sh.A, sh.B
    for j in range(K, NALL):
        assert len(A.chan_out[j]) == len(B.chan_out[j - K]) > 0
        assert np.array_equal(u32(A.chan_out[j]), u32(B.chan_out[j - K])), j
        assert np.array_equal(u32(A.phasors[j]), u32(B.phasors[j - K])), j
        assert A.counts[j, CH] == B.counts[j - K, CH] and np.array_equal(A.words[j, CH], B.words[j - K, CH]), j
    cnt = A.boundary_cnt[K]
    assert cnt > 0
    a_old = [p for p in A.pdus if p["channel"] == CH and p["freq"] == F_OLD]
    a_new = [p for p in A.pdus if p["channel"] == CH and p["freq"] == F_NEW]
    b_new = [p for p in B.pdus if p["channel"] == CH]
    assert len(a_old) + len(a_new) == len([p for p in A.pdus if p["channel"] == CH])
    assert any(p["fcs_status"] == F.FCS_GOOD for p in a_old) and any(p["fcs_status"] == F.FCS_GOOD for p in a_new)
    assert all(p["sample_index"] < cnt for p in a_old) and all(p["sample_index"] >= cnt for p in a_new)
    assert len(a_new) == len(b_new) >= 1
    for pa, pb in zip(a_new, b_new):
        assert pa["sample_index"] - pb["sample_index"] == cnt
        assert {k: v for k, v in pa.items() if k != "sample_index"} == {k: v for k, v in pb.items() if k != "sample_index"}
    # the restarted counters: what B counted, not what A had before the boundary plus that
    for k in ("frames", "a1_found", "a2_found", "m1_found", "symbol_cnt", "train_bits_total"):
        assert A.stats[CH][k] == B.stats[CH][k], k
    assert A.stats[CH]["sample_cnt"] == B.stats[CH]["sample_cnt"] + cnt and A.stats[CH]["freq"] == F_NEW


def test_nobody_else_notices(sh):
    """3: against A' (the same stream, no retune): every other channel's words and PDUs are the same for every block; channel CH's are
    the same before the boundary, its PDUs there labelled F_OLD."""
    A, A1 = sh.A, sh.A1
    for c in range(len(FREQS)):
        last = NALL if c != CH else K
        assert np.array_equal(A.counts[:last, c], A1.counts[:last, c]) and np.array_equal(A.words[:last, c], A1.words[:last, c]), c
    others = lambda ps: [pdu_key(p) for p in ps if p["channel"] != CH]
    assert others(A.pdus) == others(A1.pdus)
    cnt = A.boundary_cnt[K]
    before = lambda ps: [pdu_key(p) for p in ps if p["channel"] == CH and p["sample_index"] < cnt]
    assert before(A.pdus) == before(A1.pdus) and len(before(A.pdus)) >= 1
    assert all(k[0] == F_OLD for k in before(A.pdus))
    assert not np.array_equal(A.words[K:, CH], A1.words[K:, CH])


@pytest.mark.parametrize("cut", ["one_sync", "mid_half", "fold_batch_1", "on_device"])
def test_the_cut_changes_nothing(gpu, sh, monkeypatch, cut):
    """4: A pushed (ii) all at once with one sync at the end, (iii) with halves of 6 blocks and demodulator launches of 3 -- the boundary
    K = 25 falls inside a half and inside a launch --, (iv) with HFDL_GPU_FOLD_BATCH=1, (v) every block from device memory (a torch
    tensor: the forward FFTs run on the input stream, beside the fold) gives the words of every channel and block and the PDU list of
    (i), the pass with a sync after every push."""
    if cut == "mid_half":
        monkeypatch.setenv("HFDL_GPU_FOLD_BATCH", "6")
        monkeypatch.setenv("HFDL_GPU_DEMOD_BATCH", "3")
    if cut == "fold_batch_1":
        monkeypatch.setenv("HFDL_GPU_FOLD_BATCH", "1")
    fe = gpu.Frontend(FS, CF, FREQS)
    g = fe.geometry
    if cut == "mid_half":
        assert (g.fold_batch, g.demod_batch) == (6, 3)
    if cut != "fold_batch_1":
        assert K % g.fold_batch and K % g.demod_batch
    p = Pass(gpu, sh.x, FREQS, 0, NALL, {K: (CH, F_NEW)}, on_device=cut == "on_device", fe=fe)
    p.close()
    assert np.array_equal(p.counts, sh.A.counts) and np.array_equal(p.words, sh.A.words)
    assert len(p.pdus) >= 2 and p.pdus == sh.A.pdus


def test_slot_is_not_channel(gpu, sh):
    """5: receivers of 3 and 2 channels; global channel 3 is receiver 1's first channel, tap slot 8 (each receiver pads its channels to
    an octet of slots: planner.h plan_receiver_slots, tests/hostsim/rx_layout_check.cpp -- the slot number is not visible through
    the interface; what is, is that the filter read for channel 3 and the words the fold makes with it change, and nothing else
    does).  Its retuned filter is a fresh create's, the other four channels' filters, words and PDUs are those of the run without the retune, and a frequency outside
    receiver 1's span (but inside receiver 0's) is refused."""
    n, nblk, k5 = sh.n, 30, 7
    cf1 = CF + 100_000
    recv = [(CF, FREQS[:3]), (cf1, [10_081_500, 10_120_000])]
    f_new = 10_150_700
    y = synth.synth_wideband(FS, cf1, nblk * n, [], noise_sigma=0.004, seed=9).astype(np.complex64)
    x = sh.x[:nblk * n]
    push = lambda fe, b: fe.push_blocks([x[b * n:(b + 1) * n], y[b * n:(b + 1) * n]])
    runs = {}
    for name, ret in (("retuned", {k5: (3, f_new)}), ("plain", None)):
        fe = gpu.MultiFrontend(FS, recv)
        if ret:
            with pytest.raises(gpu.GpuError, match="outside"):
                fe.retune(3, 9_930_500)                 # inside receiver 0's +-125 kHz, outside receiver 1's
        runs[name] = Pass(gpu, None, None, 0, nblk, ret, sync_each=True, taps=bool(ret), fe=fe, push=push)
    fresh = gpu.MultiFrontend(FS, [recv[0], (cf1, [f_new, 10_120_000])])
    fresh_filters = [fresh.read_tap(F.TAP_FILTER, i) for i in range(5)]
    fresh.close()
    R, P = runs["retuned"], runs["plain"]
    R.close()
    P.close()
    assert np.array_equal(u32(R.filters_after[3]), u32(fresh_filters[3])) and not np.array_equal(u32(R.filters_after[3]), u32(R.filters_before[3]))
    for c in (0, 1, 2, 4):
        assert np.array_equal(u32(R.filters_after[c]), u32(R.filters_before[c])) and np.array_equal(u32(R.filters_after[c]), u32(fresh_filters[c])), c
        assert np.array_equal(R.counts[:, c], P.counts[:, c]) and np.array_equal(R.words[:, c], P.words[:, c]), c
    assert np.array_equal(R.words[:k5, 3], P.words[:k5, 3]) and not np.array_equal(R.words[k5:, 3], P.words[k5:, 3])
    others = lambda ps: [pdu_key(p) for p in ps if p["channel"] != 3]
    assert others(R.pdus) == others(P.pdus) and len(others(R.pdus)) >= 1
    assert R.stats[3]["freq"] == f_new


def test_twice_and_back(gpu, sh):
    """6: F_OLD -> F_NEW -> F_OLD at two boundaries, a burst in each of the three stretches (everything pushed at once: the boundaries
    fall inside halves).  After the second retune the filter equals the original create's bit for bit, and no frame is lost to the
    carried data_slot toggle: three PDUs with a good FCS, labelled F_OLD, F_NEW, F_OLD in that order."""
    n = sh.n
    rng = np.random.default_rng(31)
    third = synth.synth_wideband(FS, CF, (NALL - K) * n, [dict(freq=F_OLD, mode=2, octets=synth.make_pdu(rng, 2), t0=0.12, amp=0.1, cfo=3.0)],
                                 noise_sigma=0.004, seed=41).astype(np.complex64)
    x = np.concatenate([sh.x, third])
    fe = gpu.Frontend(FS, CF, FREQS)
    p = Pass(gpu, x, FREQS, 0, len(x) // n, {K: (CH, F_NEW), NALL: (CH, F_OLD)}, fe=fe)
    filt = [fe.read_tap(F.TAP_FILTER, i) for i in range(len(FREQS))]
    p.close()
    for c in range(len(FREQS)):
        assert np.array_equal(u32(filt[c]), u32(sh.create_filters[c])), c
    mine = [p_ for p_ in p.pdus if p_["channel"] == CH]
    assert [(q["freq"], q["fcs_status"]) for q in mine] == [(F_OLD, F.FCS_GOOD), (F_NEW, F.FCS_GOOD), (F_OLD, F.FCS_GOOD)]
    assert p.stats[CH]["frames"] == 1           # the counters restarted at the second boundary


def test_four_retunes_and_statistics_that_never_show_the_old_counters(gpu, sh):
    """F_OLD -> F_NEW -> F_OLD -> F_NEW on one front end with nothing waited for in between: the third and fourth call reuse the two
    page-locked tap buffers (the call's one designed wait), and the filter at the end is a fresh create's on F_NEW, every other
    channel's untouched.  And the statistics read that waits for nothing: straight after a retune the channel's counters are a fresh
    channel's -- never the old ones, although the device's own reset is still queued -- while sample_cnt goes on and the other
    channels keep theirs."""
    n = sh.n
    fe = gpu.Frontend(FS, CF, FREQS)
    for b in range(K):
        fe.push_block(sh.x[b * n:(b + 1) * n])
    before = fe.all_channel_stats()                  # (no wait: the last blocks may still be running)
    fe.sync()
    done = fe.all_channel_stats()
    assert done[CH]["frames"] == 1 and done[CH]["a2_found"] >= 1
    fe.push_block(sh.x[K * n:(K + 1) * n])           # something in flight in front of the reset
    for i, f in enumerate((F_NEW, F_OLD, F_NEW)):
        fe.retune(CH, f)
        now = fe.all_channel_stats()
        assert now[CH]["freq"] == f
        for k in ("frames", "a1_found", "a2_found", "m1_found", "m1_not_found", "train_bits_total"):
            assert now[CH][k] == 0, (i, k)
        assert now[CH]["sample_cnt"] >= done[CH]["sample_cnt"]
        for c in range(len(FREQS)):
            if c != CH:
                assert now[c]["frames"] >= before[c]["frames"] and now[c]["freq"] == FREQS[c]
    fe.retune(CH, F_OLD)
    fe.retune(CH, F_NEW)                              # back to back: nothing pushed between the fourth and the fifth
    fe.push_block(sh.x[(K + 1) * n:(K + 2) * n])
    fe.sync()
    filt = [fe.read_tap(F.TAP_FILTER, i) for i in range(len(FREQS))]
    fe.close()
    assert np.array_equal(u32(filt[CH]), u32(sh.B_filters[CH]))
    for c in range(len(FREQS)):
        if c != CH:
            assert np.array_equal(u32(filt[c]), u32(sh.create_filters[c])), c


def test_refusals_change_nothing(gpu, sh, monkeypatch):
    """7: every refusal the interface can be made to give -- null handle, channel out of range, a frequency fs/2 or more from the
    centre, a frequency another channel listens on, a front end created with HFDL_GPU_FOLD_PRUNE -- returns HFDL_GPU_EINVAL with its
    text, and the block pushed after each gives the words of the run that was never asked.  (The planner's refusal of a shift cannot be
    reached through the interface: inside +-fs/2 plan_block() always succeeds.)"""
    L = gpu.load()
    assert L.hfdl_gpu_frontend_retune_channel(None, 0, F_NEW) == EINVAL and b"null" in L.hfdl_gpu_last_error()
    n = sh.n
    fe = gpu.Frontend(FS, CF, FREQS)
    fe.export_enable(list(range(len(FREQS))), ring_blocks=8)
    cases = [((-1, F_NEW), "out of range"), ((len(FREQS), F_NEW), "out of range"), ((CH, CF + FS // 2), "outside"),
             ((CH, CF - FS // 2 - 7), "outside"), ((CH, FREQS[2]), "already listens")]
    for b, ((c, f), text) in enumerate(cases):
        with pytest.raises(gpu.GpuError, match=text):
            fe.retune(c, f)
        assert fe.freqs == FREQS
        fe.push_block(sh.x[b * n:(b + 1) * n])
        fe.sync()
        samples, counts, _, _, blocks, _ = fe.export_read(b, wait=True)
        assert blocks == [b] and np.array_equal(counts[0], sh.A1.counts[b]) and np.array_equal(u32(samples)[0], sh.A1.words[b]), text
        assert fe.channel_stats(CH)["freq"] == F_OLD
    fe.close()
    monkeypatch.setenv("HFDL_GPU_FOLD_PRUNE", "1e-6")
    words = []
    for ask in (True, False):
        fe = gpu.Frontend(FS, CF, FREQS)
        fe.export_enable(list(range(len(FREQS))), ring_blocks=8)
        fe.push_block(sh.x[:n])
        if ask:
            with pytest.raises(gpu.GpuError, match="HFDL_GPU_FOLD_PRUNE"):
                fe.retune(CH, F_NEW)
        fe.push_block(sh.x[n:2 * n])
        fe.sync()
        words.append(u32(fe.export_read(0, wait=True)[0]))
        fe.close()
    assert words[0].shape[0] == 2 and np.array_equal(words[0], words[1])


def test_replay_retunes_through_the_c_host_program(sh, tmp_path):
    """hfdl_replay --retune over libhfdl_host.so and the real libhfdl_gpu.so (the weak reference to the entry point resolves): the stream
    as a cf32 file, the request timed into block K - 1 so that it is applied before block K.  The printed PDUs are A's: the same
    frequencies in the same order, the same octets."""
    path = tmp_path / "in.cf32"
    sh.x.tofile(path)
    khz = lambda f: "%.1f" % (f / 1e3)
    when = "%.6f" % ((K - 0.5) * sh.n / FS)
    out = subprocess.run([os.path.join(ROOT, "dumphfdl_amd", "hfdl_replay"), "--iq-file", str(path), "--sample-rate", str(FS), "--sample-format", "CF32",
                          "--centerfreq", khz(CF), "--retune", ":".join((when, khz(F_OLD), khz(F_NEW)))] + [khz(f) for f in FREQS],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "refused" not in out.stderr and "GPU front end" not in out.stderr, out.stderr[-2000:]
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("PDU ")]
    got = [(int(w[1][len("freq="):]), bytes.fromhex(w[-1])) for w in lines]
    assert got == [(p["freq"], p["octets"]) for p in sh.A.pdus] and [f for f, _ in got] == [F_OLD, F_NEW]
