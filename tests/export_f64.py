"""The channel export's definition in numpy (include/hfdl_gpu.h "Channel baseband export"; export_pack_kernel in
dumphfdl_amd/csrc/spectrum_kernels.hip): the fp32 emulation of the row power in the kernel's own order, term for term, the float64
value beside it, and the CS16 conversion.  Every operation of the kernel is one IEEE fp32 operation (it is compiled without FMA
contraction), which numpy repeats on float32 arrays."""
import numpy as np

THREADS = 256
LANE = np.arange(64)


def power_f32(x):
    """x: the n valid complex64 samples of a row -> float32, the word the device writes.
    term = (re re) + (im im); thread t adds terms t, t + 256, ... in turn from 0.0; xor butterfly over the 64 lanes (masks 1 .. 32);
    the four wave sums as (w0 + w1) + (w2 + w3); one division by float32(n)."""
    x = np.ascontiguousarray(x, np.complex64)
    n = len(x)
    if n == 0:
        return np.float32(0.0)
    c = x.view(np.float32).reshape(-1, 2)
    term = (c[:, 0] * c[:, 0]) + (c[:, 1] * c[:, 1])
    steps = -(-n // THREADS)
    pad = np.zeros(steps * THREADS, np.float32)            # a thread without a term in the last step adds nothing: acc + 0.0 == acc (acc >= +0)
    pad[:n] = term
    acc = np.zeros(THREADS, np.float32)
    for k in range(steps):
        acc = acc + pad[k * THREADS:(k + 1) * THREADS]
    a = acc.reshape(4, 64)
    for o in (1, 2, 4, 8, 16, 32):
        a = a + a[:, LANE ^ o]
    w = a[:, 0]
    return np.float32(((w[0] + w[1]) + (w[2] + w[3])) / np.float32(n))


def power_f64(x):
    x = np.asarray(x, np.complex128)
    return float(np.mean(x.real ** 2 + x.imag ** 2)) if len(x) else 0.0


def power_gate(P):
    """Relative bound on |power_f32 - power_f64| for rows of at most P samples: one rounding per sequential add (ceil(P / 256)), eight
    tree levels, three for the term and the division; all terms are non-negative, so the roundings are relative to the sum."""
    return (-(-P // THREADS) + 8 + 3) * 2.0 ** -23


def cs16(x, scale):
    """x: complex64 [..., P] -> (int16 [..., P, 2], clipped [...] uint32): r = rint(float32(v) * float32(scale)) per component,
    |r| > 32767 stored as +-32767, NaN stored as 0, both counted."""
    c = np.ascontiguousarray(x, np.complex64).view(np.float32).reshape(x.shape + (2,))
    nan = np.isnan(c)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(c * np.float32(scale))
    clip = nan | (np.abs(r) > 32767)
    q = np.where(nan, np.float32(0), np.clip(r, -32767, 32767)).astype(np.int16)
    return q, clip.sum(axis=(-1, -2)).astype(np.uint32)
