"""CPU tests of the spectrum monitor: the float64 definition (tests/spectrum_f64.py) against itself from two sides, the fp32 emulation
of the device's summation order against it under the GPU tests' gate, and the argument checks of the two entry points."""
import ctypes as C

import numpy as np
import pytest

import spectrum_f64 as S

N = 1 << 18


@pytest.fixture(scope="module")
def window():
    return S.make_signal(N, N, seed=7)


@pytest.mark.parametrize("bins", [16, 256, N // 64, N // 16])
@pytest.mark.parametrize("hann", [False, True])
def test_three_tap_hann_equals_the_time_domain_window(window, bins, hann):
    """band powers from the spectrum (three-tap Hann, circular at the ends, wpow = 0.375) = from np.fft.fft(w x): 1e-12 relative to
    the total, per band."""
    a = S.band_powers(S.spectrum_of(window), bins, hann)
    b = S.band_powers_from_samples(window, bins, hann)
    assert np.abs(a - b).max() <= 1e-12 * b.sum()
    # the wrap between s = N - 1 and s = 0 matters: without it the first and last band are off by far more than that
    X = S.spectrum_of(window)
    if hann:
        Xw = 0.5 * X
        Xw[1:] -= 0.25 * X[:-1]
        Xw[:-1] -= 0.25 * X[1:]
        nowrap = (np.abs(Xw) ** 2).reshape(bins, -1).sum(axis=1) / (float(N) ** 2 * 0.375)
        assert abs(nowrap[0] - b[0]) > 1e-9 * b[0] or abs(nowrap[-1] - b[-1]) > 1e-9 * b[-1]


def test_parseval_and_unit_tone(window):
    p = S.band_powers(S.spectrum_of(window), 256)
    assert abs(p.sum() - np.mean(np.abs(window) ** 2)) <= 1e-12 * p.sum()
    n = np.arange(N)
    for k in (1000.0, -3000.0, 17.0):                  # on a bin: RECT puts all of it into one band, HANN into the bins k - 1 .. k + 1
        tone = np.exp(2j * np.pi * k * n / N)
        for hann in (False, True):
            p = S.band_powers(S.spectrum_of(tone), 1024, hann)
            assert abs(p.sum() - 1.0) <= 1e-12
            assert abs(p[int((k + N / 2) // (N // 1024))] - 1.0) <= 1e-12
    # between two bins the power spreads, the total stays (a constant-modulus signal: mean of w^2 / 0.375 = 1)
    tone = np.exp(2j * np.pi * S.TONE_BIN * n / N)
    for hann in (False, True):
        assert abs(S.band_powers(S.spectrum_of(tone), 1024, hann).sum() - 1.0) <= 1e-12


def test_band_edges_hold_the_tone():
    fs, cf, bins = 2_400_000, 10_000_000, 4096
    lo, hi = S.band_edges(cf, fs, N, bins)
    G = N // bins
    assert lo[0] == cf - fs / 2 - 0.5 * fs / N and np.allclose(hi - lo, G * fs / N) and np.allclose(lo[1:], hi[:-1])
    f_tone = cf + S.TONE_BIN * fs / N
    b = int(np.argmax(S.band_powers(S.spectrum_of(np.exp(2j * np.pi * S.TONE_BIN * np.arange(N) / N)), bins)))
    assert lo[b] <= f_tone < hi[b]
    assert b == int((S.TONE_BIN + N / 2 + 0.5) // G)


def test_weak_tone_needs_the_hann_window(window):
    """64-bin bands: with HANN the -70 dBFS tone's band stands >= 10 dB above both neighbours; with RECT the 0 dBFS tone's leakage
    covers it.  (The same two inequalities the GPU test asserts of the device.)"""
    bins = N // 64
    b = int((S.WEAK_BIN + N / 2 + 0.5) // 64)
    out = {}
    for hann in (False, True):
        p = S.band_powers(S.spectrum_of(window), bins, hann)
        out[hann] = 10 * np.log10(p[b] / max(p[b - 1], p[b + 1]))
    print("weak tone above its louder neighbour: RECT %.1f dB, HANN %.1f dB" % (out[False], out[True]))
    assert out[True] >= 10.0 and out[False] < 10.0


@pytest.mark.parametrize("bins", [16, 256, N // 16])
@pytest.mark.parametrize("hann", [False, True])
def test_fp32_order_meets_the_gate_by_arithmetic_alone(bins, hann):
    """The device's summation order emulated in fp32 on the GPU tests' input (an fp32 spectrum of it), T = 1 and T = 40 blocks, against
    the float64 model of the SAME fp32 spectra under the GPU tests' gate: |mean32 - mean64| <= (log2 G + 8) 2^-23 ref."""
    G = N // bins
    overlap = N // 8
    x = S.make_signal(N, 40 * (N - overlap), seed=11)
    acc, p64, ref, worst = S.Accumulator(), [], [], {}
    for t, w in enumerate(S.windows(x, N, overlap, range(40))):
        X32 = S.spectrum_of(w).astype(np.complex64)
        acc.add(S.emulate_block(X32, bins, hann))
        p64.append(S.band_powers(X32, bins, hann))
        ref.append(S.hann_ref(X32, bins) if hann else p64[-1])
        if t + 1 in (1, 40):
            mean, peak = acc.read()
            e = np.abs(mean - np.mean(p64, axis=0)) / (S.gate(G) * np.mean(ref, axis=0))
            ep = np.abs(peak - np.max(p64, axis=0)) / (S.gate(G) * np.max(ref, axis=0))
            worst[t + 1] = (float(e.max()), float(ep.max()))
    print("bins %d %s: worst |error| / gate (mean, peak) %s" % (bins, "HANN" if hann else "RECT", worst))
    assert all(m <= 0.5 and p <= 0.5 for m, p in worst.values()), worst


def test_spectrum_entry_points_check_arguments_without_a_device():
    from dumphfdl_amd import frontend as F
    L = F.load()
    EINVAL = -1
    T, first = C.c_uint64(0), C.c_uint64(0)
    buf = (C.c_float * 16)()
    assert L.hfdl_gpu_frontend_spectrum_enable(None, 256, 0) == EINVAL
    assert b"null" in L.hfdl_gpu_last_error()
    assert L.hfdl_gpu_frontend_spectrum_read(None, 0, buf, None, 16, C.byref(T), C.byref(first), 0) == EINVAL
    assert b"null" in L.hfdl_gpu_last_error()
    assert "hfdl_gpu_frontend_spectrum_enable" in F.EXPORTS and "hfdl_gpu_frontend_spectrum_read" in F.EXPORTS
    assert (F.SPECTRUM_HANN, F.SPECTRUM_MAXHOLD) == (1, 2)


def _host_lib():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    L = C.CDLL(os.path.join(root, "dumphfdl_amd", "libhfdl_host.so"))
    L.hfdl_spectrum_csv_line.argtypes = [C.c_char_p, C.c_size_t, C.c_double, C.c_double, C.c_double, C.c_uint64, C.c_void_p, C.c_int32]
    L.hfdl_frontend_set_spectrum.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int]
    return L


def parse_rtl_power(line):
    """One rtl_power CSV line -> dict(date, time, low, high, step, samples, db)."""
    f = [t.strip() for t in line.strip().split(",")]
    return dict(date=f[0], time=f[1], low=float(f[2]), high=float(f[3]), step=float(f[4]), samples=int(f[5]), db=np.array([float(v) for v in f[6:]]))


def test_csv_line_is_rtl_power_format():
    L = _host_lib()
    mean = np.array([1.0, 0.1, 0.0, 2e-7], np.float32)
    buf = C.create_string_buffer(256)
    n = L.hfdl_spectrum_csv_line(buf, 256, 86400.0 * 365 + 3723.9, 9_875_000.0, 62_500.0, 5, mean.ctypes.data_as(C.c_void_p), 4)
    # 1971-01-01 01:02:03 UTC; 10 log10: 0, -10, the floor for an empty band, -66.99
    assert buf.value.decode() == "1971-01-01, 01:02:03, 9875000, 10125000, 62500.0000, 5, 0.00, -10.00, -200.00, -66.99\n"
    assert n == len(buf.value)
    assert L.hfdl_spectrum_csv_line(buf, 40, 0.0, 0.0, 1.0, 1, mean.ctypes.data_as(C.c_void_p), 4) == -1      # does not fit
    assert L.hfdl_spectrum_csv_line(None, 256, 0.0, 0.0, 1.0, 1, mean.ctypes.data_as(C.c_void_p), 4) == -1


def test_csv_round_trip():
    L = _host_lib()
    rng = np.random.default_rng(5)
    bins = 4096
    mean = (10.0 ** rng.uniform(-12, 0.3, bins)).astype(np.float32)
    fs, cf, N = 2_400_000, 10_000_000, 1 << 19
    lo, hi = S.band_edges(cf, fs, N, bins)
    buf = C.create_string_buffer(64 + 12 * bins)
    assert L.hfdl_spectrum_csv_line(buf, len(buf), 1.7e9 + 0.25, lo[0], hi[0] - lo[0], 37, mean.ctypes.data_as(C.c_void_p), bins) > 0
    p = parse_rtl_power(buf.value.decode())
    assert p["samples"] == 37 and len(p["db"]) == bins and (p["date"], p["time"]) == ("2023-11-14", "22:13:20")
    assert abs(p["low"] - lo[0]) <= 0.5 and abs(p["high"] - hi[-1]) <= 0.5 and abs(p["step"] - (hi[0] - lo[0])) <= 0.005
    assert abs((p["high"] - p["low"]) / p["step"] - bins) < 1e-3             # rtl_power readers derive the bin count from these three
    assert np.abs(p["db"] - 10 * np.log10(mean.astype(np.float64))).max() <= 0.005 + 1e-9


def test_set_spectrum_checks_its_arguments():
    L = _host_lib()
    for bins, interval in ((8, 1), (100, 1), (8192, 1), (256, 0)):
        assert L.hfdl_frontend_set_spectrum(b"/nonexistent/x.csv", bins, interval, 0) == -1
    assert L.hfdl_frontend_set_spectrum(b"/nonexistent/x.csv", 256, 2, 1) == 0
    assert L.hfdl_frontend_set_spectrum(None, 0, 0, 0) == 0                     # off again
