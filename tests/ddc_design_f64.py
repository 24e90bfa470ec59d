"""What a channel IS, stated from the definition: the block geometry of a sample rate, a channel's bin shift and residual NCO rate, and
its band-pass taps (numpy and `fractions` only; a helper module, not a test; nothing imported from the product, from oracle/ or from
hfdl_synth).  Written from src/fastddc.c:46-80, src/libcsdr.c:62-144, src/libcsdr_gpl.c:26-39 and src/hfdl.c:476.

Integers and the fp32 words the reference hands from one function to the next are exact here: a C `float` is a rational number, and
`f32()` rounds a Fraction to the nearest one (ties to even) without any floating-point arithmetic of its own.  Everything else --
window, sinc, sums, phases -- is float64.

Geometry of a sample rate fs (integer logic):
    decimation       the largest power of two not above fs / 5400
    transition       250 / fs as an fp32 word; taps_min_length = floor(4 / transition), made odd
    pre, post        post = decimation, pre = 1; while post is even and post / 2 != 1: post /= 2, pre *= 2   (post ends as 1 or 2)
    taps_length      (smallest power of two ABOVE taps_min_length rounded up to a multiple of pre) + 1
    N                the smallest power of two above 4 taps_length, at least pre
    overlap = taps_length - 1, input_size = N - overlap, M = N / pre, v = N / overlap, scrap = overlap / pre, post_input_size = M - scrap

A channel at `freq` Hz of a receiver centred on `centre`:
    fc               (freq + 1440 - centre) / fs cycles per sample, the carrier 1440 Hz above the channel frequency (a Fraction)
    shift            the fp32 word of (float)(centre - (freq + 1440)) / (float)fs = -fc after two roundings
    offsetbin        startbin = trunc(f32(N/2 + N/2 * (-shift) * 2)), rounded to a multiple of v with ties away from zero, minus N/2
    nco_rate         2 post pre (shift + offsetbin / N): what the bin shift left over, turned back by the NCO after decimation.  The sum
                     is exact in float64; its fp32 word is the reference's `rate`, sin / cos of pi * rate its `sindelta` / `cosdelta`
    cut-offs         f32(-shift -+ 0.5 / decimation), the two fp32 numbers the tap design is handed; inside it their half difference
                     and half sum (fp32 again) are the low-pass cut-off and the centre
The down-mix as a whole, offsetbin / N - nco_rate / (2 pre post), is fc up to those roundings.  A carrier beyond +fs/2 (freq passes
the span check |freq - centre| < fs/2, freq + 1440 does not) gives offsetbin > N/2: nothing here reduces modulo fs, the bin shift
exp(-2 pi j offsetbin n / N) and the taps' exp(2 pi j center n) do that by themselves.

Taps, length L = taps_length, mid = L // 2, i = |n - mid|, in three forms:
    definition       t[n] = sin(2 pi cutoff i) / i * (0.54 + 0.46 cos(pi i / mid))   (2 pi cutoff at i = 0: a Hamming-windowed sinc),
                     h[n] = t[n] / sum(t) * exp(2 pi j center n)
    phase32          the phase of tap n is not 2 pi center n but the reference's fp32 register: phase = f32(phase + 2 pi center) after
                     every tap, then wrapped into [0, 2 pi] by steps of f32(phase -+ 2 pi).  The register drifts linearly: at 2^20 taps
                     it ends some 0.05 rad off, which is the whole distance between the reference's taps and the definition
    phase32 + sum32  additionally sum(t) is taken over the taps rounded to fp32, in index order in an fp32 register (at 2^20 taps that
                     sum is 1.5e-5 off the float64 one)
"""
import math
from array import array
from fractions import Fraction
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

CARRIER_HZ = 1440           # src/hfdl.c:46,476
CHANNEL_RATE = 5400         # the rate the decimation aims at
TRANSITION_HZ = 250


def f32(q):
    """The fp32 number nearest the rational q (ties to even), as a Fraction.  Normal range only."""
    q = Fraction(q)
    if q == 0:
        return q
    s, a = (-1 if q < 0 else 1), abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()          # 2^(e-1) < a < 2^(e+1)
    if a < Fraction(2) ** e:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1) and -126 <= e <= 127
    ulp = Fraction(2) ** (e - 23)
    k, r = divmod(a, ulp)
    k = int(k)
    if r > ulp / 2 or (r == ulp / 2 and k % 2 == 1):
        k += 1
    return s * k * ulp


def pow2_above(x):
    p = 1
    while p <= x:
        p *= 2
    return p


def geometry(fs):
    """The block geometry every channel of a receiver at fs samples per second shares."""
    dec = 1
    while 2 * dec * CHANNEL_RATE <= fs:
        dec *= 2
    tbw = f32(Fraction(TRANSITION_HZ, fs))
    q = 4 / tbw                                                 # the reference divides in double: the same integer part unless q is
    tl = q.numerator // q.denominator                           # within 2^-52 of an integer from below, which it is nowhere near
    assert q == tl or min(q - tl, tl + 1 - q) > q * Fraction(2) ** -40
    taps_min = tl + 1 if tl % 2 == 0 else tl
    pre, post = 1, dec
    while post % 2 == 0 and post // 2 != 1:
        post //= 2
        pre *= 2
    taps_length = pow2_above(-(-taps_min // pre) * pre) + 1
    n = pow2_above(4 * taps_length)
    while n < pre:
        n *= 2
    overlap = taps_length - 1
    m = n // pre
    scrap = overlap // pre
    return SimpleNamespace(sample_rate=fs, decimation=dec, transition_bw=tbw, pre_decimation=pre, post_decimation=post, taps_min_length=taps_min,
                           taps_length=taps_length, fft_size=n, overlap_length=overlap, input_size=n - overlap, fft_inv_size=m, v=n // overlap,
                           scrap=scrap, post_input_size=m - scrap)


def channel(fs, centre, freq, g=None):
    """The channel's record: the geometry's fields plus fc, shift, startbin, offsetbin, post_shift, nco_rate (float64), the fp32 values
    nco_rate32 / sindelta / cosdelta / post_shift32 (as Python floats holding fp32 numbers), lowcut, highcut, cutoff, center."""
    g = g or geometry(fs)
    n, v, pre, post = g.fft_size, g.v, g.pre_decimation, g.post_decimation
    fc = Fraction(freq + CARRIER_HZ - centre, fs)
    shift = f32(f32(centre - (freq + CARRIER_HZ)) / f32(fs))
    mid = n // 2
    sb = f32(mid + f32(f32(mid * -shift) * 2))
    startbin = int(sb) if sb >= 0 else -int(-sb)                # truncation
    q = f32(f32(startbin) / v)
    r = int(abs(q) + Fraction(1, 2)) * (1 if q >= 0 else -1)    # ties away from zero
    startbin = v * r
    offsetbin = startbin - mid
    resid = shift + Fraction(offsetbin, n)                      # exact; also exactly a float64
    post_shift32 = pre * f32(f32(shift) + f32(f32(offsetbin) / n))
    rate32 = f32(f32(post_shift32 * post) * 2)
    hb = Fraction(1, 2 * g.decimation)
    lowcut, highcut = f32(-shift - hb), f32(-shift + hb)
    c = SimpleNamespace(**vars(g))
    c.centre, c.freq, c.fc, c.shift = centre, freq, fc, shift
    c.startbin, c.offsetbin = startbin, offsetbin
    c.nco_rate = float(2 * post * pre * resid)
    assert Fraction(c.nco_rate) == 2 * post * pre * resid
    c.post_shift32, c.nco_rate32 = float(post_shift32), float(rate32)
    c.sindelta, c.cosdelta = float(np.float32(math.sin(c.nco_rate32 * math.pi))), float(np.float32(math.cos(c.nco_rate32 * math.pi)))
    c.lowcut, c.highcut = lowcut, highcut
    c.cutoff, c.center = f32(highcut - lowcut) / 2, f32(highcut + lowcut) / 2
    return c


def downmix_error_hz(c, rate=None):
    """(offsetbin / N - rate / (2 pre post) - fc) * fs in Hz, exact: how far the centre of the whole down-mix lies from the carrier.
    rate: the NCO rate in use (default: the fp32 word)."""
    rate = Fraction(c.nco_rate32 if rate is None else rate)
    return float((Fraction(c.offsetbin, c.fft_size) - rate / (2 * c.pre_decimation * c.post_decimation) - c.fc) * c.sample_rate)


def downmix_bound_hz(c):
    """Three fp32 roundings lie between fc and the rate word -- (float)(centre - carrier), the division by fs, the sum with
    offsetbin / N -- each at most 2^-24 of a number no larger than max(|shift|, |offsetbin / N|)."""
    return float(3 * Fraction(2) ** -24 * max(abs(c.shift), abs(Fraction(c.offsetbin, c.fft_size))) * c.sample_rate)


# ---------------------------------------------------------------- taps

def lowpass_unnormalised(length, cutoff):
    """t[n]: the Hamming-windowed sinc before normalisation, float64."""
    mid = length // 2
    i = np.arange(1, mid + 1, dtype=np.float64)
    half = np.sin(2 * np.pi * float(cutoff) * i) / i * (0.54 + 0.46 * np.cos(np.pi * i / mid))
    return np.concatenate([half[::-1], [2 * np.pi * float(cutoff)], half])


def sum32(t):
    """The sum of the taps rounded to fp32, in index order in an fp32 register (numpy's accumulate over float32 is that loop:
    tests/test_ddc_design_f64_cpu.py checks it against the loop written out)."""
    return float(np.add.accumulate(np.asarray(t, np.float64).astype(np.float32), dtype=np.float32)[-1])


def phase_register(length, center):
    """phase[n] of the reference's fp32 register, float64 array.  A plain loop; the value goes through an array('f') cell, which is
    C's (float) conversion."""
    two_pi = 2 * math.pi
    step = two_pi * float(center)
    cell = array("f", [0.0])
    out = np.empty(length, np.float64)
    ph = 0.0
    for n in range(length):
        out[n] = ph
        cell[0] = ph + step
        ph = cell[0]
        while ph > two_pi:
            cell[0] = ph - two_pi
            ph = cell[0]
        while ph < 0:
            cell[0] = ph + two_pi
            ph = cell[0]
    return out


FORMS = ("definition", "phase32", "phase32+sum32")


def taps(length, cutoff, center, form="phase32+sum32", _phase=None):
    """complex128 taps of the band-pass centred on `center` (cycles per sample) with the low-pass cut-off `cutoff`, in one of FORMS."""
    assert form in FORMS and length % 2 == 1
    t = lowpass_unnormalised(length, cutoff)
    t = t / (sum32(t) if form == "phase32+sum32" else math.fsum(t))
    if form == "definition":
        n = np.arange(length, dtype=np.float64)
        ph = 2 * np.pi * ((float(center) * n) % 1.0)            # the product is exact to 2^-53 of up to 2^21 turns: 5e-10 rad
    else:
        ph = phase_register(length, center) if _phase is None else _phase
    return t * np.exp(1j * ph)


@lru_cache(maxsize=64)
def channel_taps(fs, centre, freq):
    """{form: taps} of one channel (the register is walked once), read-only arrays."""
    c = channel(fs, centre, freq)
    ph = phase_register(c.taps_length, c.center)
    out = {f: taps(c.taps_length, c.cutoff, c.center, f, ph) for f in FORMS}
    for a in out.values():
        a.setflags(write=False)
    return out


def phase_drift(length, center):
    """The register's last value minus 2 pi center (length - 1), reduced to (-pi, pi]."""
    last = phase_register(length, center)[-1]
    exact = 2 * math.pi * float((Fraction(center) * (length - 1)) % 1)
    return (last - exact + math.pi) % (2 * math.pi) - math.pi


def tap_errors(got, want):
    """(relative RMS error, worst tap error / largest tap) of a set of taps against a model's."""
    got, want = np.asarray(got, np.complex128), np.asarray(want, np.complex128)
    d = np.abs(got - want)
    return float(np.sqrt(np.sum(d ** 2) / np.sum(np.abs(want) ** 2))), float(d.max() / np.abs(want).max())


def spectrum(h, n):
    """The taps' frequency response on N bins, bin b = b / N cycles per sample (float64, not shifted)."""
    p = np.zeros(n, np.complex128)
    p[:len(h)] = h
    return np.fft.fft(p)


def response_at(h, f):
    """|H(f)| at one frequency (cycles per sample), by the sum itself."""
    n = np.arange(len(h), dtype=np.float64)
    return float(abs(np.sum(np.asarray(h, np.complex128) * np.exp(-2j * np.pi * ((float(f) * n) % 1.0)))))
