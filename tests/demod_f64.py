"""A float64 statement of the demodulator's per-sample front: arbitrary resampler, AGC, matched filter (numpy only; a helper module,
not a test).  It imports nothing from the product and nothing from oracle/.

Design (with no tables given): Kaiser low-pass h[i] = sinc(2 fc t) I0(beta sqrt(1 - (2 t / n)^2)) / I0(beta), t = i - (n - 1) / 2,
n = 2 * 7 * 256 + 1, fc = min(0.515 rate, 0.49) / 256, beta = 0.1102 (60 - 8.7), scaled to a sum of 256; branch b, tap k is h[b + 256 k];
step = round(2^24 / rate) with `rate` the fp32 value.

Resampler: output k of the WHOLE stream sits at t = k step (phase 0 at the start), i = t >> 24, branch = (t & 0xFFFFFF) >> 16,
y = sum_{j < 14} h[branch][j] x[i - j], zeros before sample 0.  A launch of n_in inputs yields the outputs with t < (inputs so far) 2^24
that were not produced yet -- possibly none.

AGC: alpha = float32(0.01), g = 1, y2 = 1; per sample y = x g; y2 = (1 - alpha) y2 + alpha |y|^2; if y2 > 1e-6: g *= y2^(-alpha / 2);
g = min(g, 1e6); level = 1 / g.

Matched filter: out[k] = sum_{t < 19} mf[t] y[k - t], zeros before sample 0; mf = tests/golden/hfdl_constants.json rounded to fp32.

Besides the values every stage reports the magnitude sums sum |h_j| |x_{i-j}| per real component, which the forward error bound of an
fp32 dot product is stated in (tests/test_gpu_demod_front_f64.py)."""
import json
import math
import os

import numpy as np

NPFB, RS_TAPS, MF_TAPS = 256, 14, 19
ALPHA = float(np.float32(0.01))
G_MAX, Y2_MIN = 1e6, 1e-6
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def design(rate):
    """(h[256][14] float64, step) of the resampler for the fp32 rate."""
    rate = float(np.float32(rate))
    n = 2 * 7 * NPFB + 1
    fc = min(0.515 * rate, 0.49) / NPFB
    beta = 0.1102 * (60.0 - 8.7)
    t = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    h = np.sinc(2.0 * fc * t) * np.i0(beta * np.sqrt(1.0 - (2.0 * t / n) ** 2)) / np.i0(beta)
    h *= NPFB / h.sum()
    return np.ascontiguousarray(h[:NPFB * RS_TAPS].reshape(RS_TAPS, NPFB).T), int(round(float(1 << 24) / rate))


def matched_filter_taps():
    K = json.load(open(os.path.join(GOLD, "hfdl_constants.json")))
    return np.array(K["matched_filter"], np.float64).astype(np.float32).astype(np.float64)


def fir(taps, x, hist):
    """out[k] = sum_t taps[t] x[k - t] over the launch x with `hist` = the len(taps) - 1 samples in front of it (oldest first).
    Returns (out, magnitude sums of the real parts, of the imaginary parts, new hist)."""
    n = len(taps)
    z = np.concatenate([hist, np.asarray(x, np.complex128)])
    if len(x) == 0:
        return np.zeros(0, np.complex128), np.zeros(0), np.zeros(0), z
    w = np.lib.stride_tricks.sliding_window_view(z, n)[:, ::-1]             # w[k][t] = x[k - t]
    a = np.abs(taps)
    return w @ taps, np.abs(w.real) @ a, np.abs(w.imag) @ a, z[len(z) - (n - 1):]


class DemodFrontF64:
    """One channel.  tables = (rs_h[256 * 14], rs_step, mf[19]) as read back from the side under test (fp32 values), or None: the float64
    design for `rate`."""

    def __init__(self, rate=None, tables=None):
        if tables is None:
            self.h, self.step = design(rate)
            self.mf = matched_filter_taps()
        else:
            self.h = np.asarray(tables[0], np.float64).reshape(NPFB, RS_TAPS)
            self.step = int(tables[1])
            self.mf = np.asarray(tables[2], np.float64)
        self.n_in = 0                                   # input samples so far
        self.k = 0                                      # outputs so far
        self.rs_hist = np.zeros(RS_TAPS - 1, np.complex128)
        self.g, self.y2 = 1.0, 1.0
        self.mf_hist = np.zeros(MF_TAPS - 1, np.complex128)
        self.rs_mag = self.mf_mag = None                # magnitude sums (re, im) of the last launch
        self.t = np.zeros(0, np.int64)                  # phase t_k of the last launch's outputs
        self.g_trace, self.y2_trace = [], []            # after every sample of the stream

    def resample(self, x):
        x = np.asarray(x, np.complex128)
        z = np.concatenate([self.rs_hist, x])           # z[m] = stream sample self.n_in - 13 + m
        first = self.n_in
        self.n_in += len(x)
        k_end = ((self.n_in << 24) + self.step - 1) // self.step          # outputs with k step < n_in 2^24
        t = np.arange(self.k, max(k_end, self.k), dtype=np.int64) * self.step
        self.k += len(t)
        self.t = t
        self.rs_hist = z[len(z) - (RS_TAPS - 1):]
        if len(t) == 0:
            self.rs_mag = (np.zeros(0), np.zeros(0))
            return np.zeros(0, np.complex128)
        i = (t >> 24) - first + (RS_TAPS - 1)           # index of x[i] in z
        h = self.h[(t & 0xFFFFFF) >> 16]
        w = z[i[:, None] - np.arange(RS_TAPS)[None, :]]
        self.rs_mag = ((np.abs(h) * np.abs(w.real)).sum(1), (np.abs(h) * np.abs(w.imag)).sum(1))
        return (h * w).sum(1)

    def agc(self, x):
        """(gained samples, level after each)"""
        y = np.zeros(len(x), np.complex128)
        lvl = np.zeros(len(x))
        g, y2 = self.g, self.y2
        for k, v in enumerate(np.asarray(x, np.complex128)):
            o = complex(v) * g
            y2 = (1.0 - ALPHA) * y2 + ALPHA * (o.real * o.real + o.imag * o.imag)
            if y2 > Y2_MIN:
                g *= math.exp(-0.5 * ALPHA * math.log(y2))
            g = min(g, G_MAX)
            y[k] = o
            lvl[k] = 1.0 / g if g > 0.0 else math.inf
            self.g_trace.append(g)
            self.y2_trace.append(y2)
        self.g, self.y2 = g, y2
        return y, lvl

    def matched(self, y):
        out, mr, mi, self.mf_hist = fir(self.mf, y, self.mf_hist)
        self.mf_mag = (mr, mi)
        return out

    def push(self, x):
        """One launch of input samples -> (resampled, agc_out, level, mf_out)."""
        r = self.resample(x)
        y, lvl = self.agc(r)
        return r, y, lvl, self.matched(y)


# ---------------------------------------------------------------- the edge stream of the tests

def psk_like(rng, n, sps, offset):
    """Random 8-PSK symbols of `sps` samples each (fractional), smoothed over one symbol, turning by `offset` cycles per sample."""
    sym = np.exp(2j * np.pi * rng.integers(0, 8, int(n / sps) + 3) / 8.0)
    x = sym[(np.arange(n) / sps).astype(np.int64)]
    w = np.hanning(int(round(sps)) + 2)[1:-1]
    x = np.convolve(x, w / w.sum(), mode="same")
    return x * np.exp(2j * np.pi * offset * np.arange(n))


def edge_stream(seed, rate, outputs=6000, zeros=1300, onset=1e-3, tone=True):
    """cf32 channelizer output of one channel, lengths given in 5400-sps OUTPUT samples (input samples = outputs / rate): an 8-PSK-like
    burst at 0.05 with 30 Hz offset on noise of sigma 0.003 over the first quarter; `zeros` exact zeros; an onset of the same burst at
    amplitude `onset` (its noise scaled alike) to the end; over the last third a tone 40 dB above the burst at 0.45 cycles per input
    sample, in the resampler's transition band."""
    rng = np.random.default_rng(seed)
    rate = float(np.float32(rate))
    fs_in = 5400.0 / rate
    n = int(math.ceil(outputs / rate))
    a, b = int(outputs / 4 / rate), int((outputs / 4 + zeros) / rate)
    sig = psk_like(rng, n, fs_in / 1800.0, 30.0 / fs_in)
    noise = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.003
    x = 0.05 * sig + noise
    x[b:] *= onset / 0.05
    x[a:b] = 0.0
    if tone:
        c = 2 * n // 3
        x[c:] += 0.05 * 100.0 * np.exp(2j * np.pi * 0.45 * np.arange(n - c))
    return x.astype(np.complex64)


def rel_rms(got, want):
    got, want = np.asarray(got, np.complex128), np.asarray(want, np.complex128)
    return float(np.sqrt(np.mean(np.abs(got - want) ** 2) / np.mean(np.abs(want) ** 2)))


def worst_over_rms(got, want):
    got, want = np.asarray(got, np.complex128), np.asarray(want, np.complex128)
    return float(np.abs(got - want).max() / np.sqrt(np.mean(np.abs(want) ** 2)))


def level_errors(got, want):
    """(relative RMS, worst sample) of the AGC level: the error of every sample relative to that sample's level (the level spans twelve
    decades over the edge stream; an RMS relative to the stream's RMS would see its loudest stretch only)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    e = np.abs(got - want) / want
    return float(np.sqrt(np.mean(e ** 2))), float(e.max())
