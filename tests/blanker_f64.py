"""The wideband impulse-noise blanker's rule in float64 (dumphfdl_amd/csrc/blanker.h), the input condition that makes the device's mask
the model's, and the decode scenario the blanker is judged on.  numpy only: shared by the CPU and the GPU tests.

Rule, per block of n NEW samples and per receiver, on the fp32-converted samples x:
    P = mean |x|^2 (float64 here)      mask = |x|^2 > k2 P,  k2 = (float)10^(threshold_db / 10)
A masked sample enters the transform as (0, 0).

The device adds P up in fp32, in a fixed order whose longest path has d = blank_sum_depth(n) additions.  For a sum of non-negative
terms the relative error is at most d u (u = 2^-24); the two products and the addition of a term add 2 u; a margin of x 2 covers the
second-order terms and the final division: |P - P64| / P64 <= 2 (d + 2) u (power_bound).  So that the last bits of P cannot move a
sample across the threshold, a test input must keep every sample's power a relative 1e-3 away from it (assert_guard_band): with
d <= 40 the device's threshold is within 6e-6 of the model's."""
import numpy as np

SFMT_CF32, SFMT_CS16, SFMT_CU8 = 0, 1, 2
U = 2.0 ** -24


def convert(raw, fmt):
    """raw interleaved I, Q values of a sample format -> complex64, by the expressions the device's loads were shown to equal bit for bit
    (tests/test_gpu_parity.py, tests/test_host_lib_cpu.py): the reference's convert_cf32 / convert_cs16 / convert_cu8"""
    raw = np.asarray(raw)
    if fmt == SFMT_CS16:
        return np.ascontiguousarray(raw.astype(np.float32) / np.float32(32767.5)).view(np.complex64)
    if fmt == SFMT_CU8:
        return np.ascontiguousarray((raw.astype(np.float32) - np.float32(63.5)) / np.float32(127.0)).view(np.complex64)
    if raw.dtype == np.complex64:
        return np.ascontiguousarray(raw)
    return np.ascontiguousarray(raw, dtype=np.float32).view(np.complex64)


def k2_of(threshold_db):
    """(float)10^(threshold_db / 10), computed in double from the float the C ABI receives"""
    return np.float32(10.0 ** (float(np.float32(threshold_db)) / 10.0))


def power64(x):
    x = np.asarray(x, np.complex64)
    return x.real.astype(np.float64) ** 2 + x.imag.astype(np.float64) ** 2


def model(x, threshold_db):
    """(mask, P, T, p) of one block x (complex64, already converted); a block whose P is NaN or Inf has an empty mask"""
    p = power64(x)
    with np.errstate(invalid="ignore", over="ignore"):
        P = float(np.mean(p)) if len(p) else 0.0
        T = float(k2_of(threshold_db)) * P
        mask = p > T if np.isfinite(P) else np.zeros(len(p), bool)
    return mask, P, T, p


def assert_guard_band(p, T, rel=1e-3):
    """no sample's power lies within a relative `rel` of the threshold: a condition on the TEST INPUT"""
    if T > 0 and np.isfinite(T):
        near = np.abs(p - T) <= rel * T
        assert not near.any(), "test input inside the guard band: sample %d has power %.6g, threshold %.6g" % (int(np.argmax(near)), p[np.argmax(near)], T)


def blank(x, threshold_db, guard=True):
    """(the block as it enters the transform, mask, P): where(mask, 0, x) with the guard band asserted"""
    mask, P, T, p = model(x, threshold_db)
    if guard:
        assert_guard_band(p, T)
    return np.where(mask, np.complex64(0), np.asarray(x, np.complex64)), mask, P


def blank_stream(x, n, threshold_db):
    """a stream cut into whole blocks of n samples: (blanked stream, per-block mask counts, per-block P)"""
    x = np.asarray(x, np.complex64)
    out = x.copy()
    counts, powers = [], []
    for b in range(len(x) // n):
        y, mask, P = blank(x[b * n:(b + 1) * n], threshold_db)
        out[b * n:(b + 1) * n] = y
        counts.append(int(mask.sum()))
        powers.append(P)
    return out, counts, powers


def power_bound(depth):
    return 2.0 * (depth + 2) * U


def add_impulses(x, fs, per_second, length, amp, seed):
    """`per_second` impulses a second of `length` samples each, amplitude `amp`, random phase (constant over an impulse), at random
    places that do not overlap: one per slot of fs / per_second samples.  Returns (x + impulses, the samples an impulse covers)."""
    rng = np.random.default_rng(seed)
    x = np.array(x, np.complex64)
    slot = int(fs // per_second)
    hit = np.zeros(len(x), bool)
    for s in range(len(x) // slot):
        at = s * slot + int(rng.integers(0, slot - length))
        x[at:at + length] += np.complex64(amp * np.exp(2j * np.pi * rng.random()))
        hit[at:at + length] = True
    return x, hit


# ---- the decode scenario: weak frames under impulse noise

FS, CF = 250000, 10_000_000
FREQS = [9_958_000, 10_012_000, 10_061_000]
DURATION_S = 6.0
NOISE_SIGMA = 0.01
THRESHOLD_DB = 14.0
IMPULSES = dict(per_second=300, length=8, amp=0.9, seed=77)


def scenario_bursts(synth):
    rng = np.random.default_rng(2024)
    plan = [(0, 1, 0.20, 0.0040, 4.0), (1, 3, 0.30, 0.0050, -7.0), (2, 1, 0.40, 0.0060, 9.0),
            (0, 3, 3.00, 0.0070, -3.0), (1, 1, 3.10, 0.0080, 6.0), (2, 3, 3.20, 0.0045, -8.0)]
    return [dict(freq=FREQS[c], mode=mode, octets=synth.make_pdu(rng, mode), t0=t0, amp=amp, cfo=cfo) for c, mode, t0, amp, cfo in plan]


_scenario = None


def scenario():
    """dict(clean, impulsive: complex64 streams of DURATION_S at FS; hit: the impulse samples; sent: sorted [(freq, octets)]),
    computed once per process and left unchanged"""
    global _scenario
    if _scenario is None:
        import hfdl_synth as synth
        bursts = scenario_bursts(synth)
        clean = synth.synth_wideband(FS, CF, int(DURATION_S * FS), bursts, noise_sigma=NOISE_SIGMA, seed=31)
        imp, hit = add_impulses(clean, FS, **IMPULSES)
        for a in (clean, imp, hit):
            a.setflags(write=False)
        _scenario = dict(clean=clean, impulsive=imp, hit=hit, sent=sorted((b["freq"], bytes(b["octets"])) for b in bursts))
    return _scenario


def oracle_pdus(pyoracle, x, fs=FS, cf=CF, freqs=FREQS):
    """sorted [(freq, octets)] the oracle decodes from stream x"""
    ora = pyoracle.Frontend(fs, cf, freqs)
    n = ora.ddc.input_size
    for b in range(len(x) // n):
        ora.push_block(x[b * n:(b + 1) * n])
    out = sorted((p["freq"], bytes(p["octets"])) for p in ora.pdus)
    ora.close()
    return out


def delivered(pdus, sent):
    """how many of the sent (freq, octets) appear among the decoded ones (a decoded PDU may carry padding behind the sent octets)"""
    left = list(pdus)
    got = 0
    for f, o in sent:
        for i, (pf, po) in enumerate(left):
            if pf == f and po[:len(o)] == o:
                got += 1
                del left[i]
                break
    return got
