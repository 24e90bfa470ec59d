"""GPU tests of the spectrum monitor at every band width (spectrum_bands in dumphfdl_amd/csrc/spectrum_kernels.hip) against the float64
model and the fp32 emulation of tests/spectrum_f64.py.

The kernel reduces a band of G = N / bins bins along a path that depends on G alone:
    G = 16, 32, 64   the xor butterfly stops inside a wave, several bands share a wave
    G = 128          one wave per band, no LDS
    G = 256          wsum[wave & ~1] + wsum[wave | 1]: two bands share a workgroup's wsum
    G = 512          (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]): one band per tile
    G = 1024, 2048   a workgroup owns the band and walks it in 2 and 4 tiles: a per-thread Kahan sum, then the tree of G = 512
N = 2^15 (250 ksps) reaches all eight with bins = N / 16 ... 16; N = 2048 (12 ksps, four workgroups) reaches G = 16 ... 128.

Gates: those of tests/test_gpu_spectrum.py, through the same check_against_model -- per band (log2 G + 8) 2^-23 of the reference against the
float64 model of the device's own spectra (HFDL_GPU_TAP_SPECTRUM), AND the very words of the fp32 emulation, for the mean, the peak
and the interval rows; end to end (RECT, T = 1) the forward FFT's 3e-6 of the whole spectrum plus the same gate.  Every band of every
read of every receiver is compared.

A front end is created once per module and its blocks' spectra are read once; a case pushes the same five blocks behind the same
history twice (reads without reset and self-closing rows; then reads with reset at the rows' ends) and the three tests of a case
share the result."""
import numpy as np
import pytest

import spectrum_f64 as S
from dumphfdl_amd import frontend as F
from spectrum_f64 import check_against_model
from test_gpu_spectrum import stream_for
from test_gpu_spectrum_history import same

pytestmark = pytest.mark.gpu

WIDTHS = (16, 32, 64, 128, 256, 512, 1024, 2048)
NBLK = 5
ROW_BLOCKS = 2                 # spectrum_history(interval_blocks): rows of blocks 0-1 and 2-3 close by themselves, block 4 stays in the open row


def window_name(hann):
    return "HANN" if hann else "RECT"


class Sweep:
    """A front end, its receivers' streams of NBLK blocks and spec[r][b] = the device's own spectrum of receiver r's block b pushed
    behind block b - 1 (block 0 behind block NBLK - 1).  run(G, hann) pushes the blocks in that order again and keeps what the device
    returned; every case's blocks therefore have the windows, and the spectra, of the reference pass."""

    def __init__(self, fe, xs, chan_of_rx, t_reads):
        self.fe, self.xs, self.chan_of_rx, self.t_reads = fe, xs, chan_of_rx, t_reads
        g = fe.geometry
        self.N, self.n, self.ov, self.nrx = g.fft_size, g.input_size, g.overlap_length, len(xs)
        self.push(NBLK - 1)
        fe.poll_pdus()
        self.spec = [[] for _ in xs]
        for b in range(NBLK):
            self.push(b)
            for r in range(self.nrx):
                self.spec[r].append(fe.read_tap(F.TAP_SPECTRUM, chan_of_rx[r]))
        fe.poll_pdus()
        self.results, self.models = {}, {}

    def push(self, b):
        blk = [x[b * self.n:(b + 1) * self.n] for x in self.xs]
        if self.nrx == 1:
            self.fe.push_block(blk[0])
        else:
            self.fe.push_blocks(blk)

    def start(self, bins, hann):
        """monitor off, block NBLK - 1 as the history of block 0, monitor on: the next block pushed is block 0"""
        self.fe.spectrum_enable(0)
        self.push(NBLK - 1)
        self.fe.poll_pdus()
        self.fe.spectrum_enable(bins, hann=hann, maxhold=True)

    def model(self, G, hann):
        """per receiver: float64 band powers p64[t], the gate's reference ref[t], the fp32 emulation emu[t] of every block"""
        if (G, hann) not in self.models:
            bins = self.N // G
            out = []
            for r in range(self.nrx):
                p64 = np.array([S.band_powers(X, bins, hann) for X in self.spec[r]])
                ref = np.array([S.hann_ref(X, bins) for X in self.spec[r]]) if hann else p64
                out.append((p64, ref, [S.emulate_block(X, bins, hann) for X in self.spec[r]]))
            self.models[G, hann] = out
        return self.models[G, hann]

    def run(self, G, hann):
        if (G, hann) in self.results:
            return self.results[G, hann]
        fe, bins = self.fe, self.N // G
        assert bins * G == self.N and 16 <= bins <= self.N // 16
        res = dict(reads={}, resets={})
        # reads without reset after the blocks of t_reads (the first: the `fresh` path; later: the Kahan step and fmaxf), rows closing by themselves
        self.start(bins, hann)
        fe.spectrum_history(4, ROW_BLOCKS)
        res["base"] = fe.counters()["blocks"]
        for b in range(NBLK):
            self.push(b)
            if b + 1 in self.t_reads:
                res["reads"][b + 1] = [fe.spectrum_read(r) for r in range(self.nrx)]
        res["rows"] = [fe.spectrum_rows(r, wait=True) for r in range(self.nrx)]
        res["tap"] = [fe.read_tap(F.TAP_SPECTRUM, c) for c in self.chan_of_rx]
        fe.poll_pdus()
        # the rows' blocks again, with a read-with-reset where each row ended
        self.start(bins, hann)
        for b in range(2 * ROW_BLOCKS):
            self.push(b)
            if (b + 1) % ROW_BLOCKS == 0:
                res["resets"][b + 1] = [fe.spectrum_read(r, reset=True) for r in range(self.nrx)]
        fe.poll_pdus()
        fe.spectrum_enable(0)
        self.results[G, hann] = res
        return res

    # ---- the three checks of a case, every receiver

    def check_stage(self, tag, G, hann):
        res, model = self.run(G, hann), self.model(G, hann)
        for r in range(self.nrx):
            # the spectra of this pass are those of the reference pass: the newest block's, bit for bit
            assert np.array_equal(res["tap"][r].view(np.uint32), self.spec[r][NBLK - 1].view(np.uint32))
            p64, ref, emu = model[r]
            acc = S.Accumulator()
            for t in range(max(self.t_reads)):
                acc.add(emu[t])
                if t + 1 in self.t_reads:
                    got = res["reads"][t + 1][r]
                    assert got["first_block"] == res["base"] and got["mean"].shape == (self.N // G,)
                    check_against_model("%s rx%d G=%d %s" % (tag, r, G, window_name(hann)), got, p64, ref, acc.read(), G, t + 1)

    def check_end_to_end(self, tag, G):
        """RECT, T = 1: the device's mean against float64 np.fft of the [history, new] window of block 0 (tests/test_gpu_spectrum.py)"""
        res, bins = self.run(G, False), self.N // G
        for r in range(self.nrx):
            x = self.xs[r].astype(np.complex128)
            w = S.windows(x[:self.n], self.N, self.ov, [0], history=x[(NBLK - 1) * self.n:])[0]
            got = res["reads"][1][r]
            assert got["blocks"] == 1
            m64 = S.band_powers_from_samples(w, bins)
            err = np.abs(np.sqrt(got["mean"].astype(np.float64)) - np.sqrt(m64))
            lim = 3e-6 * np.sqrt(m64.sum()) + S.gate(G) * np.sqrt(m64)
            print("%s rx%d end to end G=%d: worst error / bound %.3f" % (tag, r, G, (err / lim).max()))
            assert (err <= lim).all(), (tag, r, G, float((err / lim).max()))

    def check_rows(self, tag, G, hann):
        """the two closed rows: the words of the emulation over their own blocks (and the model's gate), and of a read-with-reset over them"""
        res, model, bins = self.run(G, hann), self.model(G, hann), self.N // G
        for r in range(self.nrx):
            got = res["rows"][r]
            assert (got["row"], got["blocks"], got["next_row"]) == ([0, 1], [ROW_BLOCKS] * 2, 2)
            assert got["first_block"] == [res["base"], res["base"] + ROW_BLOCKS]
            assert got["mean"].shape == (2, bins) and got["peak"].shape == (2, bins)
            p64, ref, emu = model[r]
            for i in range(2):
                first, end = i * ROW_BLOCKS, (i + 1) * ROW_BLOCKS
                acc = S.Accumulator()
                for t in range(first, end):
                    acc.add(emu[t])
                row = dict(mean=got["mean"][i], peak=got["peak"][i], blocks=got["blocks"][i])
                check_against_model("%s rx%d row %d G=%d %s" % (tag, r, i, G, window_name(hann)), row, p64[first:end], ref[first:end], acc.read(), G, ROW_BLOCKS)
                rd = res["resets"][end][r]
                assert rd["blocks"] == ROW_BLOCKS
                assert same(got["mean"][i], rd["mean"]) and same(got["peak"][i], rd["peak"]), (tag, r, i, G, hann)
            assert not same(got["mean"][0], got["mean"][1])


# ---------------------------------------------------------------- 1. every width at N = 2^15

FS, CF, FREQ = 250_000, 10_000_000, 10_040_000


@pytest.fixture(scope="module")
def wide(gpu):
    fe = gpu.Frontend(FS, CF, [FREQ])
    assert fe.geometry.fft_size == 1 << 15
    x = stream_for(fe, FS, CF, FREQ, seed=501, nblk=NBLK)
    yield Sweep(fe, [x], [0], t_reads=(1, 4))
    fe.close()


@pytest.mark.parametrize("hann", [False, True], ids=window_name)
@pytest.mark.parametrize("G", WIDTHS)
def test_mean_and_peak_at_every_width(wide, G, hann):
    """after one block (the `fresh` stores) and after four (three Kahan steps, fmaxf), read without reset"""
    wide.check_stage("250 ksps", G, hann)


@pytest.mark.parametrize("G", WIDTHS)
def test_end_to_end_at_every_width(wide, G):
    wide.check_end_to_end("250 ksps", G)


@pytest.mark.parametrize("hann", [False, True], ids=window_name)
@pytest.mark.parametrize("G", WIDTHS)
def test_rows_at_every_width(wide, G, hann):
    wide.check_rows("250 ksps", G, hann)


# ---------------------------------------------------------------- 2. two receivers through the inter-wave paths

@pytest.fixture(scope="module")
def pair(gpu):
    centres, freqs = [10_000_000, 11_300_000], [[10_040_000], [11_262_000]]
    fe = gpu.MultiFrontend(FS, list(zip(centres, freqs)))
    assert fe.geometry.fft_size == 1 << 15
    xs = [stream_for(fe, FS, c, fr[0], seed=520 + r, nblk=NBLK) for r, (c, fr) in enumerate(zip(centres, freqs))]
    yield Sweep(fe, xs, [0, 1], t_reads=(1, 4))
    fe.close()


@pytest.mark.parametrize("G", [256, 512])
def test_two_receivers_where_waves_meet_through_lds(pair, G):
    """Two receivers of different content, HANN and max-hold: each receiver's mean, peak and rows against the model of ITS spectra.  At
    G = 256 two bands share a workgroup's wsum, and blockIdx.y selects the receiver: a slip mixes bands or receivers."""
    pair.check_stage("2 x 250 ksps", G, True)
    pair.check_rows("2 x 250 ksps", G, True)
    reads = pair.run(G, True)["reads"][4]
    assert not same(reads[0]["mean"], reads[1]["mean"]) and not same(reads[0]["peak"], reads[1]["peak"])
    # one receiver's result is not inside the other's gate either: band for band the two differ by more than the gate allows
    p0, ref0, _ = pair.model(G, True)[0]
    assert (np.abs(reads[1]["mean"] - p0[:4].mean(axis=0)) > S.gate(G) * ref0[:4].mean(axis=0)).mean() > 0.9


# ---------------------------------------------------------------- 3. the halo, made visible

TONE_AMP = 0.1


@pytest.mark.parametrize("G", [16, 2048])
@pytest.mark.parametrize("side", ["below", "above"])
def test_halo_with_on_bin_tones(wide, side, G):
    """HANN on a stream that is four on-bin tones and nothing else, one on the same side of each boundary of S.HALO_EDGES: the circular
    wrap, a wave boundary inside a tile (127 | 128), a tile boundary (511 | 512), a tile boundary inside an owner's walk at G = 2048
    (1023 | 1024).  A tone leaves 2/3 of its power in its bin and 1/6 in each neighbour (tests/test_spectrum_cpu.py), so a neighbour
    that is missing, doubled or not taken round the ends moves a band by a sixth of a tone.  The two sides of a boundary are two
    cases, not one stream: tones on adjacent bins add up coherently under the three taps and their shares are no longer sixths.

    Every band under the stage gate and as the emulation's words (T = 1, 2); then, T = 1, against the shares written down without a
    transform: |got - want| <= gate ref + E (2 sqrt(want) + E), the stage gate plus what the spectrum itself may be off by as an
    amplitude, E = (3e-6 + 2^-24) sqrt(sum want / 0.375) -- the forward FFT's 3e-6 of the whole spectrum's RMS
    and the rounding of the samples to fp32, through three taps of absolute sum 1 and the division by sqrt(0.375)."""
    fe, N, n = wide.fe, wide.N, wide.n
    bins = N // G
    pos = S.halo_tones(N, side)
    x = S.tone_stream(N, 3 * n, pos, TONE_AMP).astype(np.complex64)
    fe.spectrum_enable(0)
    fe.push_block(x[:n])                           # the history of block 1: the stream runs through without a seam from here on
    fe.poll_pdus()
    fe.spectrum_enable(bins, hann=True, maxhold=True)
    reads, spec = [], []
    for t in (1, 2):
        fe.push_block(x[t * n:(t + 1) * n])
        reads.append(fe.spectrum_read(0))
        spec.append(fe.read_tap(F.TAP_SPECTRUM))
        fe.poll_pdus()
    fe.spectrum_enable(0)
    p64, ref = np.array([S.band_powers(X, bins, True) for X in spec]), np.array([S.hann_ref(X, bins) for X in spec])
    # first the readable statement, T = 1: the bands next to every boundary in sixths of a tone, and every band against the shares
    want = S.tone_band_powers(N, pos, TONE_AMP, bins)
    mean = reads[0]["mean"].astype(np.float64)
    E = (3e-6 + S.U) * np.sqrt(want.sum() / 0.375)
    tol = S.gate(G) * ref[0] + E * (2 * np.sqrt(want) + E)
    near = sorted({((e - 1) % N) // G for e in S.HALO_EDGES} | {e // G for e in S.HALO_EDGES})
    sixth = TONE_AMP ** 2 / 6
    for b in near:
        print("tones %s G=%d band %d: device %.6f, model %.6f, shares %.6f sixths of a tone (tolerance %.2g)"
              % (side, G, b, mean[b] / sixth, p64[0][b] / sixth, want[b] / sixth, tol[b] / sixth))
    assert tol.max() < 1e-3 * sixth
    off = np.flatnonzero(np.abs(mean - want) > tol)
    assert len(off) == 0, (side, G, "band, device, shares in sixths of a tone", [(int(b), round(float(mean[b] / sixth), 4), round(float(want[b] / sixth), 4)) for b in off[:8]])
    assert abs(mean.sum() - want.sum()) <= tol.sum()
    assert abs(mean.sum() - p64[0].sum()) <= S.gate(G) * ref[0].sum()
    # then the stage check, every band, T = 1 and 2
    acc = S.Accumulator()
    for t, X in enumerate(spec):
        acc.add(S.emulate_block(X, bins, True))
        check_against_model("tones %s G=%d" % (side, G), reads[t], p64, ref, acc.read(), G, t + 1)


# ---------------------------------------------------------------- 4. the smallest FFT

@pytest.fixture(scope="module")
def small(gpu):
    fs, cf = 12_000, 10_000_000
    fe = gpu.Frontend(fs, cf, [cf - 2_000])
    g = fe.geometry
    assert g.fft_size == 2048               # four monitor workgroups; bins = 16 is the widest band the interface allows
    x = S.make_signal(g.fft_size, NBLK * g.input_size, seed=540).astype(np.complex64)
    yield Sweep(fe, [x], [0], t_reads=(1, 3))
    fe.close()


@pytest.mark.parametrize("hann", [False, True], ids=window_name)
@pytest.mark.parametrize("G", [16, 32, 64, 128])
def test_smallest_fft(small, G, hann):
    """N = 2048 at 12 ksps, bins = 128 ... 16: mean and peak after one and three blocks, the rows, and with RECT end to end"""
    assert small.fe.geometry.fft_size == 2048
    small.check_stage("12 ksps", G, hann)
    small.check_rows("12 ksps", G, hann)
    if not hann:
        small.check_end_to_end("12 ksps", G)
    with pytest.raises(F.GpuError):
        small.fe.spectrum_enable(2048 // 8)        # a band of 8 bins is not offered
