"""GPU tests of the spectrum monitor's history of interval rows (hfdl_gpu_frontend_spectrum_history / _row_close / _rows; the second
target of spectrum_bands in dumphfdl_amd/csrc/spectrum_kernels.hip).

What a row must be: the very 32-bit words hfdl_gpu_frontend_spectrum_read(rx, reset = 1) returns for the same blocks -- the same Kahan
sequence on the device, the same division on the host -- so every comparison between the two paths, between runs and with the fp32
emulation of tests/spectrum_f64.py is on uint32.  Against the float64 model a row sits inside the monitor's own gate
((log2 G + 8) 2^-23 per band, derived in tests/test_gpu_spectrum.py), checked by that file's check_against_model.  Shapes are the
smallest that reach both epilogues of the kernel (a band per workgroup, G > 512, and the tile path down to a band of 8 threads), both
windows, more than one receiver, the ring's wrap, and N = 2^23."""
import numpy as np
import pytest

import spectrum_f64 as S
from dumphfdl_amd import frontend as F
from test_gpu_spectrum import check_against_model, pdu_key, stream_for, traffic, u32

pytestmark = pytest.mark.gpu

FS, CF, FREQ = 250_000, 10_000_000, 10_040_000
NBLK = 9
CLOSES = (1, 3, 4, 9)          # rows of 1, 2, 1 and 5 blocks


def same(a, b):
    return a is not None and b is not None and a.shape == b.shape and bool(np.array_equal(u32(a), u32(b)))


class OneReceiver:
    """One 250 ksps front end and its NBLK-block stream; spec[b] = the device's own spectrum of block b pushed behind block b - 1
    (block 0 behind block NBLK - 1), computed once and shared by the tests below, which all push the blocks in that order."""

    def __init__(self, gpu):
        self.fe = gpu.Frontend(FS, CF, [FREQ])
        g = self.fe.geometry
        self.N, self.n = g.fft_size, g.input_size
        self.x = S.make_signal(self.N, NBLK * self.n, seed=77).astype(np.complex64)
        self.push(NBLK - 1)
        self.spec = []
        for b in range(NBLK):
            self.push(b)
            self.spec.append(self.fe.read_tap(F.TAP_SPECTRUM))
        self.fe.poll_pdus()

    def push(self, b, fe=None):
        (fe or self.fe).push_block(self.x[b * self.n:(b + 1) * self.n])

    def start(self, bins, hann=True, fe=None):
        """monitor off, block NBLK - 1 as the history of block 0, monitor on: the next block pushed is block 0 of the shared pass"""
        fe = fe or self.fe
        fe.spectrum_enable(0)
        self.push(NBLK - 1, fe)
        fe.poll_pdus()
        fe.spectrum_enable(bins, hann=hann, maxhold=True)


@pytest.fixture(scope="module")
def one(gpu):
    o = OneReceiver(gpu)
    yield o
    o.fe.close()


def run_rows(o, rows, closes, interval=0, resets=(), fe=None, nblk=NBLK):
    """push blocks 0 .. nblk - 1; a spectrum_read with reset after the blocks in `resets`, a row_close after those in `closes`.
    Returns (the reads, the indices row_close returned, spectrum_rows(wait=True))."""
    fe = fe or o.fe
    fe.spectrum_history(rows, interval)
    reads, closed = {}, []
    for b in range(nblk):
        o.push(b, fe)
        if b + 1 in resets:
            reads[b + 1] = fe.spectrum_read(0, reset=True)
        if b + 1 in closes:
            closed.append(fe.spectrum_row_close())
    got = fe.spectrum_rows(0, wait=True)
    fe.poll_pdus()
    return reads, closed, got


@pytest.mark.parametrize("hann", [False, True])
@pytest.mark.parametrize("bins", [16, 256, -16])
def test_rows_equal_read_with_reset(one, bins, hann):
    """Case 1: rows of 1, 2, 1 and 5 blocks against spectrum_read(reset) at the same boundaries, the fp32 emulation and the float64 model."""
    o = one
    bins = o.N // 16 if bins < 0 else bins
    G = o.N // bins
    o.start(bins, hann)
    base = o.fe.counters()["blocks"]
    reads, closed, got = run_rows(o, 8, CLOSES, resets=CLOSES)
    assert closed == [0, 1, 2, 3]
    assert got["row"] == [0, 1, 2, 3] and got["next_row"] == 4 and got["mean"].shape == (4, bins) and got["peak"].shape == (4, bins)
    p64 = np.array([S.band_powers(X, bins, hann) for X in o.spec])
    ref = np.array([S.hann_ref(X, bins) for X in o.spec]) if hann else p64
    first = 0
    for i, end in enumerate(CLOSES):
        rd = reads[end]
        assert (got["blocks"][i], got["first_block"][i]) == (end - first, base + first) == (rd["blocks"], rd["first_block"])
        assert same(got["mean"][i], rd["mean"]) and same(got["peak"][i], rd["peak"]), (bins, hann, i)
        acc = S.Accumulator()
        for t in range(first, end):
            acc.add(S.emulate_block(o.spec[t], bins, hann))
        row = dict(mean=got["mean"][i], peak=got["peak"][i], blocks=got["blocks"][i])
        check_against_model("row %d bins=%d %s" % (i, bins, "HANN" if hann else "RECT"), row, p64[first:end], ref[first:end], acc.read(), G, end - first)
        first = end


def test_rows_and_reads_are_independent(gpu, one):
    """Case 2: closing rows does not touch the read's accumulators (a second front end without the history reads the same words), and a
    read's reset does not touch the open row (rows closed at 1, 3, 4, 9 are the same words with reads-with-reset at 2, 5, 7)."""
    o = one
    plain = gpu.Frontend(FS, CF, [FREQ])
    bins = 256
    o.start(bins)
    o.start(bins, fe=plain)
    _, _, rows_a = run_rows(o, 8, CLOSES)
    for b in range(NBLK):
        o.push(b, plain)
    ra, rp = o.fe.spectrum_read(0), plain.spectrum_read(0)
    assert ra["blocks"] == rp["blocks"] == NBLK and same(ra["mean"], rp["mean"]) and same(ra["peak"], rp["peak"])
    plain.poll_pdus()
    # reads with reset at other blocks than the closes, on both
    o.start(bins)
    o.start(bins, fe=plain)
    reads_h, _, rows_b = run_rows(o, 8, CLOSES, resets=(2, 5, 7))
    reads_p = {}
    for b in range(NBLK):
        o.push(b, plain)
        if b + 1 in (2, 5, 7):
            reads_p[b + 1] = plain.spectrum_read(0, reset=True)
    assert rows_a["row"] == rows_b["row"] == [0, 1, 2, 3] and rows_a["blocks"] == rows_b["blocks"] == [1, 2, 1, 5]
    assert same(rows_a["mean"], rows_b["mean"]) and same(rows_a["peak"], rows_b["peak"])
    for k in (2, 5, 7):
        assert reads_h[k]["blocks"] == reads_p[k]["blocks"] == {2: 2, 5: 3, 7: 2}[k]
        assert same(reads_h[k]["mean"], reads_p[k]["mean"]) and same(reads_h[k]["peak"], reads_p[k]["peak"])
    ra, rp = o.fe.spectrum_read(0), plain.spectrum_read(0)
    assert ra["blocks"] == rp["blocks"] == 2 and same(ra["mean"], rp["mean"]) and same(ra["peak"], rp["peak"])
    plain.poll_pdus()
    plain.close()


def test_three_receivers_rows_close_by_themselves(gpu):
    """Case 3: interval_blocks = 2, five blocks: rows 0 and 1, the fifth block in open row 2 (not returned); receiver r's rows = those of
    a front end of its own fed receiver r's samples; info identical across receivers."""
    fs = 2_048_000
    centres, nchs = [10_000_000, 11_300_000, 8_950_000], [1, 3, 2]
    freqs = [[c + 50_000 + 15_000 * i for i in range(k)] for c, k in zip(centres, nchs)]
    multi = gpu.MultiFrontend(fs, list(zip(centres, freqs)))
    singles = [gpu.Frontend(fs, c, fr) for c, fr in zip(centres, freqs)]
    n, nblk = multi.input_size, 5
    xs = [stream_for(multi, fs, c, fr[0], seed=400 + r, nblk=nblk) for r, (c, fr) in enumerate(zip(centres, freqs))]
    for fe in [multi] + singles:
        fe.spectrum_enable(1024, hann=True, maxhold=True)
        fe.spectrum_history(4, 2)
    for b in range(nblk):
        multi.push_blocks([x[b * n:(b + 1) * n] for x in xs])
        for s, x in zip(singles, xs):
            s.push_block(x[b * n:(b + 1) * n])
    info0 = None
    for r, s in enumerate(singles):
        gm, gs = multi.spectrum_rows(r, wait=True), s.spectrum_rows(0, wait=True)
        info = (gm["row"], gm["first_block"], gm["blocks"], gm["next_row"])
        assert info == ([0, 1], [0, 2], [2, 2], 2) == (gs["row"], gs["first_block"], gs["blocks"], gs["next_row"])
        info0 = info0 or info
        assert info == info0
        assert same(gm["mean"], gs["mean"]) and same(gm["peak"], gs["peak"]), r
    # the rows differ between receivers (different content), so a receiver stride gone wrong cannot hide
    assert not same(multi.spectrum_rows(0, wait=True)["mean"], multi.spectrum_rows(1, wait=True)["mean"])
    assert multi.spectrum_row_close() == 2                       # the fifth block's row was open
    assert multi.spectrum_rows(2, from_row=2, wait=True)["blocks"] == [1]
    for fe in [multi] + singles:
        fe.poll_pdus()
        fe.close()


def test_ring_wrap_and_loss(one):
    """Case 4: rows = 2 and seven one-block rows keep rows 5 and 6 (the values a ring of 8 holds for them); paging with max_rows = 1."""
    o = one
    every = tuple(range(1, 8))
    o.start(256)
    _, closed, full = run_rows(o, 8, every, nblk=7)
    assert closed == list(range(7)) and full["row"] == list(range(7)) and full["blocks"] == [1] * 7
    o.start(256)
    base = o.fe.counters()["blocks"]
    _, closed, got = run_rows(o, 2, every, nblk=7)
    assert closed == list(range(7))
    assert got["row"] == [5, 6] and got["next_row"] == 7 and got["first_block"] == [base + 5, base + 6] and got["blocks"] == [1, 1]
    assert same(got["mean"], full["mean"][5:]) and same(got["peak"], full["peak"][5:])
    assert not same(full["mean"][5], full["mean"][6])
    again = o.fe.spectrum_rows(0, from_row=got["next_row"], wait=True)
    assert again["row"] == [] and again["next_row"] == 7 and again["mean"].shape == (0, 256)
    nxt, seen = 0, []
    for _ in range(3):
        page = o.fe.spectrum_rows(0, from_row=nxt, max_rows=1, wait=True)
        seen += page["row"]
        if page["row"]:
            assert same(page["mean"][0], full["mean"][page["row"][0]])
        nxt = page["next_row"]
    assert seen == [5, 6] and nxt == 7
    z = o.fe.spectrum_rows(0, from_row=0, max_rows=0)
    assert z["row"] == [] and z["next_row"] == 5


def test_collecting_without_waiting_changes_nothing(gpu):
    """Case 5: the traffic of test_monitor_moves_nothing_else; spectrum_rows(wait=False) after every push and a close every 3 blocks.
    PDUs and fold launch shapes equal the run without the history; the rows gathered on the way plus a final wait=True call are every
    row exactly once, in order, never an unclosed one, and the words of a run that only collects at the end."""
    fs, cf = 250_000, 10_000_000
    freqs = [9_915_000, 9_972_000, 10_026_000, 10_083_000, 10_101_000]
    x = traffic(fs, cf, freqs, 9.0, 31)

    def run(history, collect):
        fe = gpu.Frontend(fs, cf, freqs)
        n, nblk = fe.input_size, len(x) // fe.input_size
        fe.reset_timers(True)
        fe.spectrum_enable(256, hann=True, maxhold=True)
        if history:
            fe.spectrum_history(64)
        rows, nxt, closed = [], 0, 0
        for b in range(nblk):
            fe.push_block(x[b * n:(b + 1) * n])
            if history and b % 3 == 2:
                assert fe.spectrum_row_close() == closed
                closed += 1
            if collect:
                got = fe.spectrum_rows(0, from_row=nxt, wait=False)
                assert all(r < closed for r in got["row"]) and got["next_row"] == nxt + len(got["row"])
                rows += list(zip(got["row"], got["blocks"], got["first_block"], got["mean"], got["peak"]))
                nxt = got["next_row"]
        if history:
            got = fe.spectrum_rows(0, from_row=nxt, wait=True)
            rows += list(zip(got["row"], got["blocks"], got["first_block"], got["mean"], got["peak"]))
            assert got["next_row"] == closed
        shapes = fe.fold_launch_shapes()
        pdus = fe.poll_pdus()
        fe.close()
        return sorted(pdu_key(p) for p in pdus), shapes, rows, closed

    plain, late, live = run(False, False), run(True, False), run(True, True)
    assert len(plain[0]) >= 5 and plain[0] == live[0] == late[0]
    assert plain[1] == live[1] == late[1] and sum(plain[1].values()) >= 2
    assert live[3] == late[3] >= 3
    assert [r[0] for r in live[2]] == [r[0] for r in late[2]] == list(range(live[3]))
    for a, b in zip(live[2], late[2]):
        assert a[1:3] == b[1:3] == (3, 3 * a[0]) and same(a[3], b[3]) and same(a[4], b[4])


def test_semantics(one):
    """Case 6: a close without a block makes no row; spectrum_enable drops the history; rows = 0 frees it and reads go on; a new
    spectrum_history starts over at row 0."""
    o = one
    fe = o.fe
    o.start(64)
    with pytest.raises(F.GpuError):
        fe.spectrum_rows(0)                                      # history not on yet
    with pytest.raises(F.GpuError):
        fe.spectrum_row_close()
    for bad in ((1, 0), (-1, 0), (F.SPECTRUM_ROWS_MAX + 1, 0), (4, -1)):
        with pytest.raises(F.GpuError):
            fe.spectrum_history(*bad)
    fe.spectrum_history(4)
    assert fe.spectrum_row_close() == 0 and fe.spectrum_row_close() == 0      # nothing pushed: row 0 stays open
    assert fe.spectrum_rows(0, wait=True)["row"] == []
    o.push(0)
    assert fe.spectrum_rows(0, wait=True)["row"] == []                       # open, not closed
    assert fe.spectrum_row_close() == 0
    assert fe.spectrum_row_close() == 1 and fe.spectrum_row_close() == 1      # row 1 is open and empty
    o.push(1)
    o.push(2)
    assert fe.spectrum_row_close() == 1
    got = fe.spectrum_rows(0, wait=True)
    assert (got["row"], got["blocks"], got["next_row"]) == ([0, 1], [1, 2], 2)
    with pytest.raises(F.GpuError):
        fe.spectrum_rows(1)                                      # one receiver
    with pytest.raises(F.GpuError):
        fe.spectrum_rows(0, max_rows=-1)
    # numbering starts over, the read's accumulators are untouched by it
    fe.spectrum_history(4)
    o.push(3)
    assert fe.spectrum_row_close() == 0
    again = fe.spectrum_rows(0, wait=True)
    assert (again["row"], again["blocks"]) == ([0], [1]) and not same(again["mean"][0], got["mean"][0])
    rd = fe.spectrum_read(0)
    assert rd["blocks"] == 4
    # rows = 0: off, reads go on
    fe.spectrum_history(0)
    with pytest.raises(F.GpuError):
        fe.spectrum_rows(0)
    o.push(4)
    rd = fe.spectrum_read(0)
    assert rd["blocks"] == 5
    # without MAXHOLD a row has no peak, and the C entry point refuses to be asked for one
    fe.spectrum_history(2)
    fe.spectrum_enable(64)                                       # again: the history is gone
    with pytest.raises(F.GpuError):
        fe.spectrum_rows(0)
    fe.spectrum_history(2)
    o.push(5)
    fe.spectrum_row_close()
    got = fe.spectrum_rows(0, wait=True)
    assert got["peak"] is None and got["row"] == [0] and same(got["mean"][0], fe.spectrum_read(0)["mean"])
    import ctypes as C
    buf = np.zeros(64, np.float32)
    info, n, nxt = F.SpectrumRow(), C.c_int32(0), C.c_uint64(0)
    assert fe._L.hfdl_gpu_frontend_spectrum_rows(fe._h, 0, 0, 1, buf.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p), C.byref(info), C.byref(n), C.byref(nxt), 1) == -1
    fe.spectrum_enable(0)
    with pytest.raises(F.GpuError):
        fe.spectrum_history(4)                                   # monitor off
    fe.poll_pdus()


def test_rows_at_40_msps(gpu):
    """Case 7: N = 2^23, 4096 Hann bands with max-hold, rows of 1 and 2 blocks against read-with-reset."""
    fs, cf = 40_000_000, 8_000_000
    fe = gpu.Frontend(fs, cf, [8_927_000])
    g = fe.geometry
    assert g.fft_size == 1 << 23
    x = S.make_signal(g.fft_size, 2 * g.input_size, seed=41).astype(np.complex64)
    blocks = [x[:g.input_size], x[g.input_size:], x[:g.input_size]]
    fe.spectrum_enable(4096, hann=True, maxhold=True)
    fe.spectrum_history(2)
    reads = []
    for b, blk in enumerate(blocks):
        fe.push_block(blk)
        if b in (0, 2):
            reads.append(fe.spectrum_read(0, reset=True))
            fe.spectrum_row_close()
    got = fe.spectrum_rows(0, wait=True)
    fe.poll_pdus()
    assert (got["row"], got["blocks"], got["first_block"]) == ([0, 1], [1, 2], [0, 1])
    for i, rd in enumerate(reads):
        assert rd["blocks"] == got["blocks"][i] and same(got["mean"][i], rd["mean"]) and same(got["peak"][i], rd["peak"])
    assert not same(got["mean"][0], got["mean"][1])
    fe.close()
