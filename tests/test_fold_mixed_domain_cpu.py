"""The fold in the mixed FFT domain (csrc/fold_domain.h), without a GPU.

The forward FFT is N = R1 R2 R3 in three passes, k = k1 + R1 k2 + R1 R2 k3, and pass 3 is a plain R3-point DFT over n3 of what pass 2
leaves (Z for a block, T for a channel's taps).  The fold's sum over every k with one k mod M runs over the whole k3 digit, so

    sum_k3 H[k1,k2,k3] X[k1,k2,k3] = R3 sum_n3 T[k1,k2,(-n3) mod R3] Z[k1,k2,n3]

and the fold can contract over the rows rho = (k2hi, n3) of pass 2's output: pass 3 is never run.  Here: a float64 numpy model of
the three passes, of the packed operands ([rho][j'] taps scaled by R3 and index-reversed, [g][rho][16] block) and of the contraction,
against the plain sum over alias rows of numpy's own transform -- with the index maps taken from a host build of the header
(tests/hostsim/fold_domain_check.cpp dump) AND spelled out independently in numpy, the two compared entry by entry."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fold_domain") / "fold_domain_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "dumphfdl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "hostsim", "fold_domain_check.cpp"), "-o", exe])
    return exe


def header_maps(exe, l1, l2, l3, logm):
    """(j -> j', (k2, n3) -> rho, (k2, n3) -> tap row) as the header computes them."""
    out = np.array(subprocess.run([exe, "dump", str(l1), str(l2), str(l3), str(logm)], capture_output=True, text=True, check=True).stdout.split(), dtype=np.int64)
    m = 1 << logm
    bins = out[:2 * m].reshape(m, 2)
    rows = out[2 * m:].reshape(1 << l2, 1 << l3, 4)
    assert (bins[:, 0] == np.arange(m)).all()
    return bins[:, 1], rows[:, :, 2], rows[:, :, 3]


def numpy_maps(l1, l2, l3, logm):
    """The same maps from their definition: j = k1 + R1 k2lo, j' = 16 (k1 + R1 (k2lo >> 4)) + (k2lo & 15); rho = k2hi R3 + n3."""
    q, m = logm - l1, 1 << logm
    j = np.arange(m)
    k1, k2lo = j & ((1 << l1) - 1), j >> l1
    jp = 16 * (k1 + (k2lo >> 4 << l1)) + (k2lo & 15)
    k2, n3 = np.meshgrid(np.arange(1 << l2), np.arange(1 << l3), indexing="ij")
    rho = (k2 >> q) * (1 << l3) + n3
    tap = (k2 >> q) * (1 << l3) + ((-n3) % (1 << l3))
    return jp, rho, tap


def test_the_header_maps_hold_on_every_plan(check_exe):
    """fold_domain_check.cpp: bijections, group order, the tap row's reversal, pass 2's store address against the fold's load address
    for every element, over every register-resident plan and admissible M; and the predicate's refusals."""
    out = subprocess.run([check_exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    assert int(out.stdout.split()[0]) > 10_000_000


def three_passes(x, l1, l2, l3, upto=3):
    """The library's factorisation in float64: x[n1 R2 R3 + n2 R3 + n3] -> pass 1 over n1 (twiddle W_N^(k1 c), c = n2 R3 + n3) -> pass 2
    over n2 (twiddle W_(R2 R3)^(k2 n3)) -> Z[k1, k2, n3] -> pass 3 over n3 -> X[k1 + R1 k2 + R1 R2 k3]."""
    r1, r2, r3 = 1 << l1, 1 << l2, 1 << l3
    n = r1 * r2 * r3
    a = np.fft.fft(x.reshape(r1, r2 * r3), axis=0)
    a *= np.exp(-2j * np.pi * ((np.arange(r1)[:, None] * np.arange(r2 * r3)[None, :]) % n) / n)
    z = np.fft.fft(a.reshape(r1, r2, r3), axis=1)
    z *= np.exp(-2j * np.pi * ((np.arange(r2)[:, None] * np.arange(r3)[None, :]) % (r2 * r3)) / (r2 * r3))[None]
    if upto == 2:
        return z
    return np.fft.fft(z, axis=2).transpose(2, 1, 0).reshape(n)        # [k3][k2][k1] flattened = k1 + R1 k2 + R1 R2 k3


def pack(z, t, maps, l1, l2, l3, logm):
    """Pass 2's outputs of a block and of the taps -> the fold's operands: block [j'][rho], taps [rho][j'] = R3 T[k1, k2, -n3]."""
    jp_of, rho, tap = maps
    q, m, pre = logm - l1, 1 << logm, 1 << (l1 + l2 + l3 - logm)
    k1, k2 = np.meshgrid(np.arange(1 << l1), np.arange(1 << l2), indexing="ij")
    jp = jp_of[k1 + ((k2 & ((1 << q) - 1)) << l1)]                   # [k1][k2]
    zb = np.zeros((m, pre), z.dtype)
    g = np.zeros((pre, m), t.dtype)
    zb[jp[:, :, None], rho[None, :, :]] = z
    g[tap[None, :, :], jp[:, :, None]] = t * (1 << l3)
    return zb, g


def signal(n, m, seed):
    """White noise plus a tone 20 dB up outside the pass band, and a windowed-sinc band-pass centred between two bins, n / 2 + 1 taps."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)
    x += 10.0 * np.exp(2j * np.pi * 0.31234567 * np.arange(n))
    nt = n // 2 + 1
    i = np.arange(nt) - (nt - 1) / 2
    h = np.sinc(i / m) / m * np.hamming(nt) * np.exp(2j * np.pi * (0.1234567 + 0.37 / n) * np.arange(nt))
    return x, np.concatenate([h, np.zeros(n - nt)])


@pytest.mark.parametrize("logm", [10, 11, 12])
def test_the_identity_at_6_6_6(check_exe, logm):
    """N = 2^18 split 6 / 6 / 6, M = 1024 (four bits of k2 in the bin: g = k1), 2048 (five: the generalised group index) and 4096 (all
    six: no k2hi, the rows are n3 alone).  float64: the contraction over rho equals the sum over alias rows to rounding; and with fp32
    operands and a sequential fp32 chain over the rows -- the order of the fold's fused multiply-adds, one row after the other -- the
    mixed-domain sum is no further from float64 than a chain of `pre` roundings allows: sqrt(pre) 2^-23 relative RMS (each of the pre
    complex products and additions rounds to 2^-24 relative, independently; the spectrum-domain chain is held to the same bound)."""
    l1 = l2 = l3 = 6
    n, m = 1 << 18, 1 << logm
    pre = n // m
    maps = header_maps(check_exe, l1, l2, l3, logm)
    for a, b in zip(maps, numpy_maps(l1, l2, l3, logm)):
        assert (a == b).all()
    x, h = signal(n, m, 5 + logm)
    X, H = np.fft.fft(x), np.fft.fft(h)
    assert np.abs(three_passes(x, l1, l2, l3) - X).max() < 1e-9 * np.abs(X).max()          # the model of the passes is the transform
    want = (H * X).reshape(pre, m).sum(axis=0)
    zb, g = pack(three_passes(x, l1, l2, l3, upto=2), three_passes(h, l1, l2, l3, upto=2), maps, l1, l2, l3, logm)
    got = (g.T * zb).sum(axis=1)[maps[0]]                            # Y[j] = Y'[j'(j)]
    rms = np.sqrt(np.mean(np.abs(want) ** 2))
    err = np.sqrt(np.mean(np.abs(got - want) ** 2)) / rms
    print("6/6/6 M %d float64: relative RMS %.3g" % (m, err))
    assert err < 1e-12

    def chain(a, b):                                                 # a[row][bin] * b[row][bin], rows one after the other in fp32
        a, b = a.astype(np.complex64), b.astype(np.complex64)
        acc = np.zeros(a.shape[1], np.complex64)
        for r in range(a.shape[0]):
            acc = (acc + a[r] * b[r]).astype(np.complex64)
        return acc
    e_mixed = np.sqrt(np.mean(np.abs(chain(g, zb.T)[maps[0]] - want) ** 2)) / rms
    e_spec = np.sqrt(np.mean(np.abs(chain(H.reshape(pre, m), X.reshape(pre, m)) - want) ** 2)) / rms
    print("6/6/6 M %d fp32 chain of %d rows: mixed %.3g  spectrum %.3g (relative RMS against float64)" % (m, pre, e_mixed, e_spec))
    bound = np.sqrt(pre) * 2.0 ** -23
    assert e_mixed < bound and e_spec < bound


def test_the_identity_at_8_8_7(check_exe):
    """The 40 Msps plan: l = 8 / 8 / 7, M = 4096 -- sixteen k2hi x 128 n3 = 2048 rows, g = k1.  Passes 1 and 2 do not enter the identity
    (it holds per (k1, k2) for ANY Z and T), so eight of the 256 k1 with random pass-2 outputs: pass 3 by numpy, the sum over alias
    rows a = k2hi + 16 k3 of H X at the k the library's digit order gives, against the contraction of the packed operands."""
    l1, l2, l3, logm = 8, 8, 7, 12
    maps = header_maps(check_exe, l1, l2, l3, logm)
    for a, b in zip(maps, numpy_maps(l1, l2, l3, logm)):
        assert (a == b).all()
    jp_of, rho, tap = maps
    rng = np.random.default_rng(23)
    k1s = np.array([0, 1, 15, 16, 100, 200, 254, 255])
    shape = (len(k1s), 1 << l2, 1 << l3)
    z = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    t = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    X, H = np.fft.fft(z, axis=2), np.fft.fft(t, axis=2)              # [k1][k2][k3]
    q = logm - l1
    for i, k1 in enumerate(k1s):
        for k2lo in (0, 1, 7, 15):
            j = int(k1) + (k2lo << l1)
            # k = k1 + 256 k2 + 65536 k3 with k mod 4096 = j: k2 = k2lo + 16 k2hi, every k3 -- alias row a = k >> 12 = k2hi + 16 k3
            k2 = k2lo + 16 * np.arange(16)
            want = (H[i, k2, :] * X[i, k2, :]).sum()
            rows = rho[k2, :]                                        # the block's rows of this bin
            gz = np.zeros(1 << (l2 - q + l3), complex)
            gt = np.zeros_like(gz)
            gz[rows] = z[i, k2, :]
            gt[tap[k2, :]] = t[i, k2, :] * (1 << l3)
            assert sorted(rows.ravel()) == list(range(2048))
            got = (gz * gt).sum()
            assert abs(got - want) < 1e-11 * abs(want) + 1e-9, (k1, k2lo, got, want)
            assert jp_of[j] == 16 * k1 + k2lo                        # g = k1 at this geometry
