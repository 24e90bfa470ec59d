"""The wideband I/Q imbalance and DC corrector's rule in float64 (dumphfdl_amd/csrc/iqbal.h), the error bounds of its fp32 form, and the
decode scenario the corrector is judged on.  numpy only: shared by the CPU and the GPU tests.

Rule, per receiver, block by block, on the fp32-converted samples x of a block of n:
    B = (mean x, mean x^2, mean |x|^2)                 A <- A + g (B - A),  g = max(alpha, 1 / (k + 1)),  A = (m, c2, p2)
    C = c2 - m^2,  P = p2 - |m|^2,  kappa = C / (P + sqrt(P^2 - |C|^2))
    no estimate: no block yet, P not finite or not positive, P^2 - |C|^2 < 0, |C|^2 > 0.25 P^2
    block b enters the transform as d - kappa conj(d), d = x - m, with the estimate from the blocks before b; without one: as it is.
The model is x = s + kappa conj(s) + m with proper s (E s^2 = 0): E (x - m)^2 = 2 kappa sigma^2, E |x - m|^2 = (1 + |kappa|^2) sigma^2, and the
formula gives kappa back exactly (test_iqbal_cpu.py checks it to 1e-9).

Bounds of the fp32 form (u = 2^-24, d = blank_sum_depth(n), eps = 2 (d + 2) u):
  sums    Each of the five sums is added up in blanker.h's order, whose longest path has d additions, from terms that carry at most two
          roundings of their own (a product and a sum of products).  The terms are signed, so the error is relative to the sum of the
          terms' MAGNITUDES T: |S32 - S64| <= ((1 + u)^(d + 2) - 1) T <= eps T, the factor 2 covering the second-order terms as in
          blanker_f64.power_bound.  (sum_bound)
  m       mean re, mean im: |dm_re| <= eps mean |re| <= eps sqrt(p2) (Cauchy-Schwarz), so |dm| <= sqrt(2) eps sqrt(p2).  The averages
          are convex combinations of block means, so the bound holds for A with the largest p2 of the blocks seen; each update adds three
          roundings of quantities no larger than the means themselves: 4 u |m| covers them.  (m_bound)
  kappa   |dc2| <= sqrt(2) eps p2 (each component's terms are at most |x|^2), |dp2| <= eps p2.  C = c2 - m^2 and |m| <= sqrt(p2):
          |dC| <= |dc2| + 2 |m| |dm| <= 3 sqrt(2) eps p2;  |dP| <= |dp2| + 2 |m| |dm| <= (1 + 2 sqrt(2)) eps p2.
          With den = P + sqrt(P^2 - |C|^2) and |C| <= 0.5 P (an estimate exists): den >= 1.866 P, |C| / den <= 0.268,
          |d den| <= |dP| (1 + 1 / 0.866) + |dC| 0.5 / 0.866, and to first order
          |dkappa| <= (|dC| + 0.268 |d den|) / den <= (1.155 |dC| + 0.578 |dP|) / (1.866 P) <= 3.83 eps p2 / P.
          kappa_bound = 4 eps p2 / P + 32 u: the 32 u for the twenty-odd roundings of the estimate's own arithmetic, each relative to
          quantities of magnitude at most 1 here (|kappa| <= 0.268).  p2 / P = 1 + |m|^2 / P: a DC offset far above the signal costs accuracy.
What is measured on top (tests/test_iqbal_cpu.py prints it, DESIGN.md section 4.15 records it): the largest |kappa32 - kappa64| and
|m32 - m64| over the test's sizes, against the float64 model -- never against the device."""
import numpy as np

import blanker_f64 as bf

U = 2.0 ** -24
ALPHA = 0.125
ALPHA_MIN, KAPPA_MAX = 2.0 ** -10, 0.25


def terms64(x):
    """the five terms of every sample of x (complex64) in float64: [5][n]"""
    x = np.asarray(x, np.complex64)
    re, im = x.real.astype(np.float64), x.imag.astype(np.float64)
    return np.stack([re, im, re * re - im * im, 2 * re * im, re * re + im * im])


def sum_bound(depth):
    return 2.0 * (depth + 2) * U


def m_bound(depth, p2, m):
    return np.sqrt(2.0) * sum_bound(depth) * np.sqrt(p2) + 4 * U * abs(m)


def kappa_bound(depth, p2, P):
    return 4.0 * sum_bound(depth) * p2 / P + 32 * U


def estimate(m, c2, p2):
    """(valid, kappa, P) of the averages"""
    with np.errstate(all="ignore"):
        C = c2 - m * m
        P = p2 - (m.real * m.real + m.imag * m.imag)
        if not (np.isfinite(P) and P > 0):
            return False, 0j, P
        D = P * P - abs(C) ** 2
        if not D >= 0 or abs(C) ** 2 > 0.25 * P * P:
            return False, 0j, P
        return True, C / (P + np.sqrt(D)), P


class Model:
    """one receiver's corrector from a fresh enable; step(block) -> (the block as it enters the transform, record)"""

    def __init__(self, alpha=ALPHA, seed=None, hold=False):
        self.alpha = float(np.float32(alpha))
        self.k, self.A, self.prev = 0, None, None
        self.fixed = None                       # (kappa, m, hold): a seed not yet weighed, or a hold
        self.blocks = self.refused = 0
        self.p2max = 0.0
        if seed is not None:
            self.fixed = (complex(np.complex64(seed[0])), complex(np.complex64(seed[1])), bool(hold))
            self.k = 1

    def _update(self, B):
        if self.fixed is not None:
            kappa, m, _ = self.fixed
            PB = B[2] - abs(B[0]) ** 2
            if not PB > 0:
                return
            self.A = np.array([m, 2 * kappa / (1 + abs(kappa) ** 2) * PB + m * m, PB + abs(m) ** 2], complex)
            self.fixed = None
        if self.A is None:
            self.A = np.zeros(3, complex)
        g = max(self.alpha, 1.0 / (self.k + 1))
        self.A = self.A + g * (B - self.A)
        self.k += 1

    def step(self, x):
        x = np.asarray(x, np.complex64)
        if self.prev is not None and not (self.fixed is not None and self.fixed[2]):
            B = self.prev
            if np.isfinite(B.real).all() and np.isfinite(B.imag).all():
                self.p2max = max(self.p2max, B[2].real)
                self._update(B)
        if self.fixed is not None:
            valid, kappa, m, P = True, self.fixed[0], self.fixed[1], 0.0
        elif self.k == 0:
            valid, kappa, m, P = False, 0j, 0j, 0.0
        else:
            m = self.A[0]
            valid, kappa, P = estimate(m, self.A[1], self.A[2].real)
        with np.errstate(all="ignore"):
            t = terms64(x).mean(axis=1)
        self.prev = np.array([complex(t[0], t[1]), complex(t[2], t[3]), t[4]], complex)
        self.blocks += 1
        self.refused += not valid
        rec = dict(valid=valid, kappa=complex(kappa), dc=complex(m), power=float(P), blocks=self.blocks, refused=self.refused,
                   hold=bool(self.fixed is not None and self.fixed[2]), p2max=self.p2max)
        if not valid:
            return x.copy(), rec
        d = x.astype(np.complex128) - m
        return (d - kappa * np.conj(d)).astype(np.complex64), rec


def correct_stream(x, n, alpha=ALPHA, seed=None, hold=False):
    """a stream cut into whole blocks of n samples through the model: (corrected stream, [record per block]); a tail shorter than a
    block stays as it is"""
    x = np.asarray(x, np.complex64)
    out = x.copy()
    model, recs = Model(alpha, seed, hold), []
    for b in range(len(x) // n):
        out[b * n:(b + 1) * n], rec = model.step(x[b * n:(b + 1) * n])
        recs.append(rec)
    return out, recs


def impair(s, kappa, dc):
    s = np.asarray(s, np.complex64).astype(np.complex128)
    return (s + kappa * np.conj(s) + dc).astype(np.complex64)


def proper_noise(n, seed, sigma=0.1):
    rng = np.random.default_rng(seed)
    return (sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


# ---- the decode scenario: the blanker scenario's weak frames, broadcast-like bands at the channels' mirror frequencies

FS, CF, FREQS = bf.FS, bf.CF, bf.FREQS
KAPPA, DC = 0.03 * np.exp(0.7j), 0.02 + 0.01j
BAND_HZ = 5000.0


def interferers(n, rms, seed=5):
    """three bands of complex noise, BAND_HZ wide, each of `rms`, centred where the channels' images come from: CF - (f - CF)"""
    rng = np.random.default_rng(seed)
    f = np.fft.fftfreq(n, 1.0 / FS)
    t = np.arange(n) / FS
    out = np.zeros(n, np.complex128)
    for freq in FREQS:
        w = np.fft.fft(rng.standard_normal(n) + 1j * rng.standard_normal(n))
        w[np.abs(f) > BAND_HZ / 2] = 0
        b = np.fft.ifft(w)
        b *= rms / np.sqrt(np.mean(np.abs(b) ** 2))
        out += b * np.exp(2j * np.pi * (CF - freq) * t)
    return out


_scenario = {}


def scenario(rms=0.4):
    """dict(clean: the undistorted stream with the interferers, impaired: the same through kappa and DC; sent: sorted [(freq, octets)]),
    complex64 streams of the blanker scenario's length, computed once per process and left unchanged"""
    if rms not in _scenario:
        s = bf.scenario()
        clean = (s["clean"].astype(np.complex128) + interferers(len(s["clean"]), rms)).astype(np.complex64)
        impaired = impair(clean, KAPPA, DC)
        for a in (clean, impaired):
            a.setflags(write=False)
        _scenario[rms] = dict(clean=clean, impaired=impaired, sent=s["sent"])
    return _scenario[rms]


oracle_pdus, delivered = bf.oracle_pdus, bf.delivered


# ---- the host build of iqbal.h (tests/hostsim/iqbal_check.cpp)

REC = np.dtype([("blocks", "<u8"), ("refused", "<u8"), ("kappa_re", "<f4"), ("kappa_im", "<f4"), ("dc_re", "<f4"), ("dc_im", "<f4"),
                ("power", "<f4"), ("image_rejection_db", "<f4"), ("valid", "<u4"), ("hold", "<u4")])        # hfdl_gpu_iqbal_stats


def build_host_check(directory, werror=True):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(directory), "iqbal_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra"] + (["-Werror"] if werror else []) +
                          ["-I" + os.path.join(root, "dumphfdl_amd", "csrc"), "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "hostsim", "iqbal_check.cpp"), "-o", exe])
    return exe


def host_blocks(exe, directory, x, n, alpha=ALPHA, seed=None, hold=False):
    """whole blocks of x (complex64, converted) through the host build from a fresh enable: (y complex64, records as a REC array,
    [per block: the five sums as float32], [per block: mode 1 = refused, 2 = corrected])"""
    import os
    import subprocess
    x = np.ascontiguousarray(x, np.complex64)
    nblocks = len(x) // n
    src, dst = os.path.join(str(directory), "iqbal_in.cf32"), os.path.join(str(directory), "iqbal_out.bin")
    x[:nblocks * n].tofile(src)
    cmd = [exe, src, dst, str(n), str(nblocks), repr(float(np.float32(alpha)))]
    if seed is not None:
        k, m = np.complex64(seed[0]), np.complex64(seed[1])
        cmd += [repr(float(k.real)), repr(float(k.imag)), repr(float(m.real)), repr(float(m.imag)), str(int(bool(hold)))]
    lines = subprocess.run(cmd, capture_output=True, text=True, check=True).stdout.splitlines()
    raw = open(dst, "rb").read()
    y = np.frombuffer(raw, np.complex64, nblocks * n).copy()
    recs = np.frombuffer(raw, REC, nblocks, offset=8 * nblocks * n).copy()
    sums = [np.array([int(w, 16) for w in line.split()[3:8]], np.uint32).view(np.float32) for line in lines]
    modes = [int(line.split()[1]) for line in lines]
    os.remove(src)
    os.remove(dst)
    return y, recs, sums, modes
