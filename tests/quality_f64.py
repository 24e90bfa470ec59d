"""Float64 statement of the frame quality figures (include/hfdl_gpu.h hfdl_gpu_frame_quality; dumphfdl_amd/csrc/quality.h), and the
bound the fp32 implementations are held to.

Per frame of nsym = segments * 30 stored data symbols x[i] (complex64, taken exactly), p[i] = the nearest point of the mode's
constellation -- by angle, as fec_model.demap finds it; BPSK: +1 if Re x > 0, else -1 -- and e = x - p:
  seg_err_power[s] = mean |e|^2 over the 30 symbols of segment s;  err_power = mean of seg_err_power;  err_max = max |e|^2;
  sym_power = mean |x|^2;  gain = mean x conj(p).

The bound.  K counts the roundings on the longest path of quality.h's summation order, for seg_err_power / err_power (the longest):
  per term    3     e = x - p (1), ex * ex (1), fma(ey, ey, .) (1)
  segment    30     the 30 terms added one after the other
  its mean    1     the division by 30
  lane        2     ((0 + S[k]) + S[k + 128]) + S[k + 64]: the first add is exact
  wave        6     the butterfly over 64 lanes
  the mean    1     the division by the segment count
             43, and 1 more for the constellation table, whose entries are cosf / sinf values rounded to fp32: 44.
Every rounding is relative to a partial sum of non-negative terms, which the whole sum bounds, so the error is at most 44 * 2^-24 times
the figure itself -- and |e|^2 <= (|x| + 1)^2 <= 2 (|x|^2 + 1), so at most 88 * 2^-24 (sym_power + 1).  K = 96 leaves room for the
second-order terms.  sym_power and the gain have shorter paths (2 roundings per term, no division by 30) and |x conj(p)| = |x|, so the
same K holds them: |device - model| <= K 2^-24 (sym_power + 1) for the powers, K 2^-24 (max |x|^2 + 1) for err_max,
K 2^-24 (sqrt(sym_power) + 1) for the gain (mean |x| <= sqrt(mean |x|^2))."""
import numpy as np

import fec_model as fm

K = 96
assert K <= 256
EPS = 2.0 ** -24
SEG = 30


def nearest(x, arity):
    """The nearest constellation point of each symbol (complex128)."""
    x = np.asarray(x, np.complex128)
    if arity == 1:
        return np.where(x.real > 0, 1.0, -1.0).astype(np.complex128)
    M = 1 << arity
    step = 2 * np.pi / M
    lin = np.floor(np.mod(np.angle(x) + step / 2, 2 * np.pi) / step).astype(np.int64) % M
    return np.exp(2j * np.pi * lin / M)


def model(symbols, mode):
    """dict(nsym, segments, sym_power, err_power, err_max, gain (complex), seg_err_power [segments], max_x2) in float64."""
    sz = fm.sizes(mode)
    x = np.asarray(symbols, np.complex64).astype(np.complex128)
    assert len(x) == sz["nsym"]
    p = nearest(x, sz["arity"])
    e2 = np.abs(x - p) ** 2
    x2 = np.abs(x) ** 2
    seg = e2.reshape(-1, SEG).mean(axis=1)
    return dict(nsym=len(x), segments=len(seg), sym_power=float(x2.mean()), err_power=float(seg.mean()), err_max=float(e2.max()),
                gain=complex(np.mean(x * np.conj(p))), seg_err_power=seg, max_x2=float(x2.max()))


def check(rec, m, what=""):
    """Hold one record (a dict as frontend.quality_to_dict makes it) to the bound against the model's answer m."""
    assert (rec["nsym"], rec["segments"]) == (m["nsym"], m["segments"]), what
    pw = K * EPS * (m["sym_power"] + 1.0)
    for k in ("sym_power", "err_power"):
        assert abs(float(rec[k]) - m[k]) <= pw, (what, k, float(rec[k]), m[k], pw)
    seg = np.asarray(rec["seg_err_power"], np.float64)
    worst = np.max(np.abs(seg[:m["segments"]] - m["seg_err_power"]))
    assert worst <= pw, (what, "seg_err_power", worst, pw)
    assert not seg[m["segments"]:].any() and not np.signbit(seg[m["segments"]:]).any(), (what, "seg_err_power past the frame's segments")
    assert abs(float(rec["err_max"]) - m["err_max"]) <= K * EPS * (m["max_x2"] + 1.0), (what, "err_max", float(rec["err_max"]), m["err_max"])
    g = K * EPS * (np.sqrt(m["sym_power"]) + 1.0)
    assert abs(float(rec["gain_re"]) - m["gain"].real) <= g and abs(float(rec["gain_im"]) - m["gain"].imag) <= g, \
        (what, "gain", float(rec["gain_re"]), float(rec["gain_im"]), m["gain"], g)


def decisions_are_safe(frame):
    """True when no rounding can change what a frame's figures are: every symbol clear of the decision boundaries (fec_model.margins),
    or -- the two kinds burst_frames cannot clear -- so small that either decision gives the same figures to within 1e-20 of |e|."""
    x = np.asarray(frame["symbols"], np.complex64)
    arity = fm.sizes(frame["mode"])["arity"]
    if not frame["cleared"]:
        return float(np.max(np.abs(x))) <= 1e-19                 # BPSK zeros, 8-PSK at 1e-20: |e| = 1 +- |x| whichever point is taken
    if arity == 1:
        return True                                              # the sign of an fp32 number: nothing is rounded
    return float(np.min(fm.margins(x, arity)[1])) >= fm.D_ANG
