"""A float64 statement of what the channelizer computes, written from the definition (numpy only; a helper module, not a test).

The overlap-and-scrap channelizer keeps, of every block's circular convolution, only samples that no wrap-around has touched, so
outside block 0's zero history it IS a linear convolution, and its bin shift is a plain time-domain mixer.  With

    N = fft_size, overlap = taps_length - 1 = N / v, input_size = N - overlap, pre = pre_decimation, scrap = overlap / pre,
    x[n]   the whole input stream (x[n] = 0 for n < 0: block 0 sees a zero history),
    h[t]   the channel's complex band-pass taps, t = 0 .. overlap,
    y[n]   = sum_t h[t] x[n - t]                                   (linear convolution),

block k holds the samples n0 .. n0 + N - 1 with n0 = k * input_size - overlap.  Sample p of its size-M inverse transform
(M = N / pre) is the circular convolution at local index pre * p; for p >= scrap that index is >= overlap, no tap reaches across the
wrap, and the value is y[n0 + pre * p].  The circular bin shift moves spectrum bin b to bin b - offsetbin before the inverse
transform (the channel centre, bin offsetbin of the unshifted spectrum, lands on DC), and

    (1/N) sum_b Y[b] exp(+2 pi j (b - offsetbin) i / N) = y[i] * exp(-2 pi j offsetbin i / N)

so the shift is the factor exp(-2 pi j * offsetbin * n / N): NEGATIVE sign, a down-mix by offsetbin bins.  Written with the
absolute index n instead of the block-local i the factor changes by exp(-2 pi j offsetbin n0 / N); n0 is a multiple of overlap
= N / v and offsetbin a multiple of v, so that is exactly 1: the mixer is phase-continuous across blocks and no per-block or fitted
phase exists.  The unity gain follows from the 1 / (pre * M) = 1 / N normalisation.  Block k therefore hands

    z_k[j] = y[n] * exp(-2 pi j offsetbin n / N),   n = k * input_size - overlap + pre * (scrap + j),   j = 0 .. post_input_size - 1

to the NCO and the decimator: counting the z samples of all blocks g = k * post_input_size + j, every g that is a multiple of
post_decimation is kept and output number K = g / post is multiplied by exp(+j phi_K), phi_K = pi * nco_rate * K (the planner's
`nco_rate` = 2 * post_shift * post, the residual shift below one bin step).

Two NCO modes:
  * default: phi_K in float64 from the planner's fp32 `nco_rate`.  The fp32 phase accumulation and phasor recurrence of the code
    under test are then part of its measured error.  tests/test_channelizer_f64_cpu.py gates the oracle in this mode.
  * nco_phasors=[per-block complex64 tables]: the phasors that really multiplied each block (the device's tap 9, bit-exact against
    the reference recurrence) replace exp(j phi_K), so the recurrence's drift is not charged to the fold.
    tests/test_gpu_channelizer_f64.py measures the device in this mode (the oracle, its calibrating side, in the default mode) and
    bounds the tables against phi_K separately.

Nothing is fitted and nothing is skipped: block 0 is compared too (its history is zero on both sides).
"""
import math

import numpy as np


def _pow2_at_least(n):
    p = 1
    while p < n:
        p *= 2
    return p


class Stream:
    """The input stream cut into the segments the linear convolution of each block needs, with their float64 spectra cached (they
    are shared by every channel).  Segment k = x[n0 .. n0 + N - 1], zero-padded to L >= N + overlap so that the FFT product is the
    LINEAR convolution of the segment (no wrap reaches any index)."""

    def __init__(self, x, plan):
        self.x = np.asarray(x)
        self.N, self.overlap, self.input_size = int(plan.fft_size), int(plan.overlap_length), int(plan.input_size)
        assert self.N == self.overlap + self.input_size
        assert len(self.x) % self.input_size == 0
        self.nblk = len(self.x) // self.input_size
        self.L = _pow2_at_least(self.N + self.overlap)
        self._spec = {}

    def segment(self, k):
        seg = np.zeros(self.L, np.complex128)
        lo = k * self.input_size - self.overlap
        a = max(lo, 0)
        seg[a - lo:self.N] = self.x[a:lo + self.N]
        return seg

    def spectrum(self, k, keep=True):
        if k in self._spec:
            return self._spec[k]
        s = np.fft.fft(self.segment(k))
        if keep:
            self._spec[k] = s
        return s

    def forget(self, k):
        self._spec.pop(k, None)


def taps_spectrum(taps, L):
    h = np.zeros(L, np.complex128)
    h[:len(taps)] = np.asarray(taps, np.complex128)
    return np.fft.fft(h)


def nco_phase(plan, K):
    """phi_K of the default mode, float64."""
    return np.pi * float(plan.nco_rate) * np.asarray(K, np.float64)


def ddc_reference(x, taps, plan, nco_phasors=None, blocks=None, fast=False, taps_fft=None):
    """Per-block channelizer outputs (a list of complex128 arrays, one per block of `blocks`, default all) of the stream `x` (an array
    of whole blocks, or a Stream) through the channel whose time-domain taps are `taps` and whose planner record is `plan` (fft_size,
    overlap_length, input_size, pre_decimation, post_decimation, scrap, post_input_size, offsetbin, nco_rate).

    fast=False: the definition as it stands -- the whole linear convolution of the segment, mixed, every pre-th sample picked.
    fast=True: the same numbers from a size L / pre inverse transform (decimating y by `pre` aliases its spectrum: summing the pre
    slices of the length-L product first and inverting the short sum is an identity of the DFT); the CPU suite pins it to the
    definition at 1e-12 and the large geometries use it.
    taps_fft: taps_spectrum(taps, stream.L) computed before (one per channel, reused over calls)."""
    st = x if isinstance(x, Stream) else Stream(x, plan)
    N, overlap, pre, post = st.N, st.overlap, int(plan.pre_decimation), int(plan.post_decimation)
    scrap, P, off = int(plan.scrap), int(plan.post_input_size), int(plan.offsetbin)
    assert pre * scrap == overlap and len(taps) == overlap + 1 and st.L % pre == 0
    H = taps_spectrum(taps, st.L) if taps_fft is None else taps_fft
    outs = []
    for k in (range(st.nblk) if blocks is None else blocks):
        prod = st.spectrum(k) * H
        i = pre * (scrap + np.arange(P, dtype=np.int64))              # segment-local index of z_k[j]; i >= overlap: no zero padding, no wrap
        if fast:
            y = np.fft.ifft(prod.reshape(pre, st.L // pre).sum(axis=0))[scrap:scrap + P] / pre
        else:
            y = np.fft.ifft(prod)[i]
        n = k * st.input_size - overlap + i                           # absolute sample index
        z = y * np.exp(-2j * np.pi * ((off * n) % N) / N)             # the bin shift (integer phase reduced exactly)
        g = k * P + np.arange(P, dtype=np.int64)
        keep = (g % post) == 0
        K = g[keep] // post
        if nco_phasors is None:
            ph = np.exp(1j * nco_phase(plan, K))
        else:
            ph = np.asarray(nco_phasors[len(outs)], np.complex128)
            assert len(ph) == len(K)
        outs.append(z[keep] * ph)
    return outs


def half_rate_sign(g):
    """(-1)^g for stream output indices g: what the reference's bin arithmetic leaves on the output of a receiver with
    pre_decimation = post_decimation = 1 (below 10 800 sps; oracle/PINNING.md section 3).  The model above does not contain it:
    the tests of those rates multiply it in, and say so."""
    return 1.0 - 2.0 * (np.asarray(g, np.int64) & 1)


def errors(got, want):
    """(relative RMS error, worst element error / RMS of the model output) of one block."""
    got = np.asarray(got, np.complex128)
    want = np.asarray(want, np.complex128)
    rms = max(float(np.sqrt(np.mean(np.abs(want) ** 2))), 1e-300)
    d = np.abs(got - want)
    return float(np.sqrt(np.mean(d ** 2))) / rms, float(d.max()) / rms


# ---------------------------------------------------------------- the channel's plan and taps, and the test signal

def channel_offsets(fs, overlap):
    """Channel centres (Hz from the receiver centre, before the 1440 Hz of the carrier): one within 1 kHz of +fs / 2, one exactly on
    a bin that is a multiple of v (f0 = j fs / overlap an integer number of Hz; 0 where no other exists inside the band), one ordinary."""
    step = fs // math.gcd(fs, overlap)
    on_bin = step * max(1, int(0.21 * fs) // step) if step < fs // 2 else 0
    return [fs // 2 - 600, on_bin, -int(0.3137 * fs)]


def channel_plan(oracle, fs, cf, freq):
    """(planner record, time-domain band-pass taps as complex128) of one channel: the oracle's planner and tap design with the
    arguments orc_channel_create uses (the product's taps are bit-equal: test_tap_design_matches_oracle_bit_for_bit)."""
    L = oracle.lib()
    dec = L.orc_compute_fft_decimation_rate(fs, 5400)
    tbw = L.orc_transition_bw(fs, 250)
    shift = np.float32(cf - (freq + 1440)) / np.float32(fs)
    d = oracle.fastddc_init(tbw, dec, float(shift))
    hb = np.float32(0.5) / np.float32(dec)
    taps = np.zeros(d.taps_length, np.complex64)
    L.orc_firdes_bandpass_c(taps.ctypes.data, d.taps_length, float(-shift - hb), float(-shift + hb))
    return d, taps.astype(np.complex128)


def channel_plan_f64(fs, cf, freq):
    """The same pair with nothing borrowed: the record and the taps of tests/ddc_design_f64.py, written from the definition (the taps in
    the form that carries the reference's fp32 phase register and normalising sum; `nco_rate` is the fp32 word, as in channel_plan)."""
    import ddc_design_f64 as D
    plan = D.channel(fs, cf, freq)
    plan.nco_rate = plan.nco_rate32
    return plan, D.channel_taps(fs, cf, freq)["phase32+sum32"]


def alias_tone_offset(fs, cf, freq, all_freqs, pre, margin=0.3):
    """A frequency (Hz from the receiver's centre) on an alias of the channel centre, f0 + k fs / pre with k != 0, inside +-fs / 2 and at
    least margin * fs / pre away from every channel's centre (a channel's pass band is +-fs / (4 pre) wide), or None if pre == 1."""
    if pre < 2:
        return None
    f0 = freq + 1440 - cf
    step = fs / pre
    centres = np.asarray(all_freqs, np.float64) + 1440 - cf
    for k in sorted(range(-pre, pre + 1), key=lambda k: (abs(k), k)):
        f = f0 + k * step
        if k == 0 or abs(f) >= 0.5 * fs - 1:
            continue
        if np.min(np.abs(centres - f)) >= margin * step:
            return f
    return None


def make_signal(fs, cf, freqs, strong_for, nsamples, seed, dec, pre, level=1e-3, chunk=1 << 18):
    """White noise at level / 4 per component, wide-band noise 60 dB above the in-band level everywhere outside the pass bands of the
    channels of `strong_for` (wideband_outside), and for every channel of `strong_for`: two in-band tones at known amplitudes
    (level, 0.7 level at +400 / -700 Hz), one tone at the pass-band edge (the middle of the transition band) and one tone 60 dB above
    the in-band level on an alias of the channel's centre.  complex64; the model is fed these very samples, so a tone only has to be
    continuous to rounding: it is a table of one chunk times the exact phasor of the chunk's first sample."""
    rng = np.random.default_rng(seed)
    x = np.empty(nsamples, np.complex64)
    tones = []
    for i, f in enumerate(strong_for):
        f0 = f + 1440 - cf
        tones += [(f0 + 400.0, level, float(i)), (f0 - 700.0, 0.7 * level, float(i))]
        if dec > 1:
            tones.append((f0 + 0.5 * fs / dec, level, 0.0))
        fa = alias_tone_offset(fs, cf, f, freqs, pre)
        if fa is not None:
            tones.append((fa, 1000.0 * level, 0.5 * i))
    wide = wideband_outside(fs, cf, strong_for, nsamples, seed, pre, 1000.0 * level) if pre > 1 else None
    t = np.arange(min(chunk, nsamples), dtype=np.float64)
    tables = [(a * np.exp(2j * np.pi * ((f / fs * t) % 1.0) + 1j * ph)).astype(np.complex64) for f, a, ph in tones]
    for lo in range(0, nsamples, chunk):
        n = min(chunk, nsamples - lo)
        acc = np.empty(n, np.complex64)
        acc.real = rng.standard_normal(n, dtype=np.float32)
        acc.imag = rng.standard_normal(n, dtype=np.float32)
        acc *= np.float32(level / 4)
        for (f, a, ph), tab in zip(tones, tables):
            acc += tab[:n] * np.complex64(np.exp(2j * np.pi * ((f * lo / fs) % 1.0)))
        if wide is not None:
            acc += wide[lo:lo + n]
        x[lo:lo + n] = acc
    return x


def wideband_outside(fs, cf, strong_for, nsamples, seed, pre, rms, piece=1 << 22):
    """White noise of the given RMS (60 dB above the in-band level) with a notch of +-0.3 fs / pre around the centre of every channel
    of `strong_for` (its pass band is +-0.25 fs / pre wide): every alias row of those channels' filters holds its share of the input
    -- how much of a row then shows in the output is the filter's own depth, measured per row by
    tests/test_channelizer_f64_cpu.py::test_every_alias_row_is_excited_as_far_as_its_taps_reach (oracle/PINNING.md section 3) -- and
    none in their pass bands.  Made in pieces of up to 2^22 samples, each notched in its own DFT; what the cuts between pieces leak
    into the notches lies some 45 dB below the noise, beside the in-band tones.  complex64."""
    rng = np.random.default_rng(seed + 7919)
    out = np.empty(nsamples, np.complex64)
    for lo in range(0, nsamples, piece):
        n = min(piece, nsamples - lo)
        w = np.empty(n, np.complex64)
        w.real = rng.standard_normal(n, dtype=np.float32)
        w.imag = rng.standard_normal(n, dtype=np.float32)
        W = np.fft.fft(w)
        f = np.fft.fftfreq(n) * fs
        for ch in strong_for:
            d = (f - (ch + 1440 - cf) + fs / 2) % fs - fs / 2
            W[np.abs(d) <= 0.3 * fs / pre] = 0
        out[lo:lo + n] = np.fft.ifft(W) * (rms / np.sqrt(2))
    return out
