"""Float64 model of the spectrum monitor (include/hfdl_gpu.h, "Spectrum monitor") and an fp32 emulation of the device's summation
order (dumphfdl_amd/csrc/spectrum_kernels.hip).  numpy only: shared by the CPU and the GPU tests.

For an fftshifted spectrum X[0 .. N-1] of one block, B bands of G = N / B bins:
    RECT: Xw = X, wpow = 1;   HANN: Xw[s] = 0.5 X[s] - 0.25 X[s-1] - 0.25 X[s+1] (indices mod N), wpow = 0.375
    p[b] = sum_{s = bG}^{(b+1)G-1} |Xw[s]|^2 / (N^2 wpow)
mean = average of p over the blocks, peak = maximum."""
import numpy as np

U = 2.0 ** -24                 # unit round-off of fp32
TILE, THREADS = 512, 256       # spectrum.h SPECMON_TILE / SPECMON_THREADS


def gate(G):
    """Relative error bound per band of the device's fp32 result against the float64 model: |X|^2 <= 2u, a reduction tree of depth
    log2 G <= log2 G u (bands longer than a tile: a compensated per-thread sum ~2u + a tree of depth 8 instead, which is no more),
    the normalisation u, the compensated accumulation over blocks ~2u, the read-back's division u: (log2 G + 8) * 2^-23."""
    return (np.log2(G) + 8) * 2.0 ** -23


def windows(x, fft_size, overlap, blocks, history=None):
    """The overlap-and-scrap windows [history, new] of the given blocks of stream x (history before block 0: zeros, or `history`)."""
    n = fft_size - overlap
    h = np.zeros(overlap, np.complex128) if history is None else np.asarray(history, np.complex128)[-overlap:]
    xp = np.concatenate([h, np.asarray(x, np.complex128)])
    return [xp[t * n:t * n + fft_size] for t in blocks]


def hann_window(N):
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)


def spectrum_of(window, hann=False):
    """fftshifted float64 spectrum of a window of samples; hann: of w * x (the time-domain definition)."""
    w = np.asarray(window, np.complex128)
    if hann:
        w = w * hann_window(len(w))
    return np.fft.fftshift(np.fft.fft(w))


def band_powers(X, bins, hann=False):
    """p[b] of one block from its fftshifted spectrum X (the three-tap form of the Hann window), float64."""
    X = np.asarray(X, np.complex128)
    N = len(X)
    G = N // bins
    assert G * bins == N
    if hann:
        X = 0.5 * X - 0.25 * np.roll(X, 1) - 0.25 * np.roll(X, -1)
    pw = X.real ** 2 + X.imag ** 2
    return pw.reshape(bins, G).sum(axis=1) / (float(N) ** 2 * (0.375 if hann else 1.0))


def band_powers_from_samples(window, bins, hann=False):
    """p[b] from the window's samples: np.fft.fft of w * x, no three-tap identity."""
    X = spectrum_of(window, hann)
    N = len(X)
    pw = X.real ** 2 + X.imag ** 2
    return pw.reshape(bins, N // bins).sum(axis=1) / (float(N) ** 2 * (0.375 if hann else 1.0))


def hann_ref(X, bins):
    """What the HANN gate is relative to: the RECT power of the band widened by one bin on each side (circular), / 0.375 -- by
    Cauchy-Schwarz on the weights 0.5, 0.25, 0.25 an upper bound of what the cancelling three-term sum was made from."""
    X = np.asarray(X, np.complex128)
    N = len(X)
    G = N // bins
    pw = (X.real ** 2 + X.imag ** 2) / float(N) ** 2
    inner = pw.reshape(bins, G).sum(axis=1)
    left = np.roll(pw, 1)[::G]            # the bin before each band's first
    right = np.roll(pw, -1)[G - 1::G]     # the bin after each band's last
    return (inner + left + right) / 0.375


def band_edges(centerfreq, sample_rate, fft_size, bins):
    """(low, high) edge in Hz of every band: centerfreq + (bG - N/2 - 0.5) fs/N and G fs/N above that."""
    G = fft_size // bins
    lo = centerfreq + (np.arange(bins, dtype=np.float64) * G - fft_size / 2 - 0.5) * (sample_rate / fft_size)
    return lo, lo + G * (sample_rate / fft_size)


# ---------------------------------------------------------------- fp32 emulation of the device order

def _tree(a):
    """binary tree over adjacent elements of the last axis (a power of two long), fp32"""
    while a.shape[-1] > 1:
        a = a[..., 0::2] + a[..., 1::2]
    return a[..., 0]


def emulate_block(X32, bins, hann=False):
    """The device's band sums of one block in fp32, operation by operation (no fused multiply-add: the kernel is compiled without
    contraction): X32 = complex64 fftshifted spectrum.  Returns float32 p[b], already scaled."""
    X32 = np.asarray(X32, np.complex64)
    N = len(X32)
    G = N // bins
    re, im = X32.real.astype(np.float32), X32.imag.astype(np.float32)
    h, q = np.float32(0.5), np.float32(0.25)
    if hann:
        re, im = h * re - q * (np.roll(re, 1) + np.roll(re, -1)), h * im - q * (np.roll(im, 1) + np.roll(im, -1))
    pw = re * re + im * im
    term = pw[0::2] + pw[1::2]                       # a thread's two bins
    assert term.dtype == np.float32
    if G <= TILE:
        s = _tree(term.reshape(bins, G // 2))
    else:
        t = term.reshape(bins, G // TILE, THREADS)   # a thread's terms lie a tile apart
        acc, c = np.zeros((bins, THREADS), np.float32), np.zeros((bins, THREADS), np.float32)
        for i in range(t.shape[1]):                  # Kahan per thread
            y = t[:, i] - c
            u = acc + y
            c = (u - acc) - y
            acc = u
        s = _tree(acc)
    scale = np.float32(1.0 / (float(N) * float(N) * (0.375 if hann else 1.0)))
    return s * scale


class Accumulator:
    """The device accumulator: a Kahan sum per band in fp32 and a running maximum; read() as hfdl_gpu_frontend_spectrum_read."""

    def __init__(self):
        self.T = 0

    def add(self, p):
        p = np.asarray(p, np.float32)
        if self.T == 0:
            self.s, self.c, self.peak = p.copy(), np.zeros_like(p), p.copy()
        else:
            y = p - self.c
            u = self.s + y
            self.c = (u - self.s) - y
            self.s = u
            self.peak = np.maximum(self.peak, p)
        self.T += 1

    def read(self):
        return ((self.s.astype(np.float64) - self.c.astype(np.float64)) / self.T).astype(np.float32), self.peak


# ---------------------------------------------------------------- the stage check of the GPU tests

def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def over(err, lim):
    """err / lim per band for a statement err <= lim: where the bound is zero (a band whose spectrum is exact zeros: on-bin tones on
    even bins leave such) an error of zero is 0, inside it, and any other is inf."""
    err, lim = np.asarray(err, np.float64), np.asarray(lim, np.float64)
    return np.divide(err, lim, out=np.where(err > 0, np.inf, 0.0), where=lim > 0)


def check_against_model(tag, got, p64, ref, emu, G, T):
    """got = spectrum_read dict; p64 / ref [T][bins] float64 per-block powers and gate references; emu = (mean, peak) of the fp32 emulation."""
    g = gate(G)
    mean64, peak64 = np.mean(p64[:T], axis=0), np.max(p64[:T], axis=0)
    e_mean = over(np.abs(got["mean"] - mean64), g * np.mean(ref[:T], axis=0))
    e_peak = over(np.abs(got["peak"] - peak64), g * np.max(ref[:T], axis=0))
    same = bool(np.array_equal(u32(got["mean"]), u32(emu[0])) and np.array_equal(u32(got["peak"]), u32(emu[1])))
    print("%s T=%d: worst |mean error| / gate %.3f, |peak error| / gate %.3f, bit-identical to the fp32 emulation: %s" % (tag, T, e_mean.max(), e_peak.max(), same))
    assert got["blocks"] == T
    assert e_mean.max() <= 1.0 and e_peak.max() <= 1.0, (tag, T, float(e_mean.max()), float(e_peak.max()))
    assert same, (tag, T, int((u32(got["mean"]) != u32(emu[0])).sum()), int((u32(got["peak"]) != u32(emu[1])).sum()))


# ---------------------------------------------------------------- the tests' input

TONE_BIN = 1000.37            # the 0 dBFS tone, in FFT bins above the centre: between two bins
WEAK_BIN = TONE_BIN + 3 * 64 + 5      # the -70 dBFS tone: three 64-bin bands and five bins further up


def make_signal(fft_size, nsamples, seed, burst=None):
    """complex128 stream: white noise at -60 dBFS in total, a 0 dBFS tone TONE_BIN bins above the centre, a -70 dBFS tone at WEAK_BIN,
    plus `burst` (an array to add: one HFDL burst from hfdl_synth where the caller has a channel for it)."""
    rng = np.random.default_rng(seed)
    n = np.arange(nsamples, dtype=np.float64)
    x = (rng.standard_normal(nsamples) + 1j * rng.standard_normal(nsamples)) * np.sqrt(0.5e-6)
    x += np.exp(2j * np.pi * (TONE_BIN / fft_size) * n)
    x += 10 ** (-70 / 20) * np.exp(2j * np.pi * ((WEAK_BIN / fft_size) * n + 0.123))
    if burst is not None:
        x += burst
    return x


# ---------------------------------------------------------------- on-bin tones: the Hann halo made visible

HALO_EDGES = (0, 128, 512, 1024)      # boundaries e - 1 | e between fftshifted bins (mod N): the circular wrap, a wave boundary inside a
                                      # tile, a tile boundary, and a tile boundary inside an owner's walk at G = 2048


def halo_tones(N, side):
    """fftshifted positions of the tones on one side of every edge of HALO_EDGES: "below" = e - 1 (mod N), "above" = e.  Tones of one
    side lie more than two bins apart, so no two of them share a bin under the three-tap window."""
    return [(e - 1) % N if side == "below" else e for e in HALO_EDGES]


def tone_stream(N, nsamples, positions, amp):
    """complex128 stream: a sum of exponentials of amplitude `amp` exactly on the fftshifted bins `positions` of an N-point transform, and
    nothing else.  On a bin a tone is continuous from block to block: every [history, new] window holds whole cycles of it."""
    m = np.arange(nsamples, dtype=np.float64)
    x = np.zeros(nsamples, np.complex128)
    for s in positions:
        x += amp * np.exp(2j * np.pi * (((s - N // 2) * m) % N) / N)
    return x


def tone_band_powers(N, positions, amp, bins, hann=True):
    """Band powers of a window of tone_stream from the window's weights alone, no transform: RECT, a tone is amp^2 in its bin; HANN,
    0.5^2 / 0.375 = 2/3 of it in bin s and 0.25^2 / 0.375 = 1/6 in each of s - 1 and s + 1 (mod N)."""
    d = np.diff(np.sort(np.concatenate([np.asarray(positions), [min(positions) + N]])))
    assert d.min() >= 3, "tones whose three-tap footprints overlap add up coherently: not the sum of their shares"
    pw = np.zeros(N)
    for s in positions:
        for k, share in ((-1, 1 / 6), (0, 2 / 3), (1, 1 / 6)) if hann else ((0, 1.0),):
            pw[(s + k) % N] += share * amp * amp
    return pw.reshape(bins, N // bins).sum(axis=1)
