"""CPU tests of the spectrum monitor: the float64 definition (tests/spectrum_f64.py) against itself from two sides, the fp32 emulation
of the device's summation order against it under the GPU tests' gate, and the argument checks of the two entry points."""
import ctypes as C

import numpy as np
import pytest

import spectrum_f64 as S

N = 1 << 18
WIDTHS = (16, 32, 64, 128, 256, 512, 1024, 2048)       # every band width G at which spectrum_bands takes another path, and both its neighbours
EVERY_WIDTH = [16] + [N // G for G in reversed(WIDTHS)]      # as bins: a band of N / 16 bins, then G = 2048 ... 16


@pytest.fixture(scope="module")
def window():
    return S.make_signal(N, N, seed=7)


@pytest.mark.parametrize("bins", EVERY_WIDTH)
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


@pytest.fixture(scope="module")
def spectra40():
    """fp32 spectra of 40 blocks of the GPU tests' input, computed once for every width"""
    overlap = N // 8
    x = S.make_signal(N, 40 * (N - overlap), seed=11)
    return [S.spectrum_of(w).astype(np.complex64) for w in S.windows(x, N, overlap, range(40))]


@pytest.mark.parametrize("bins", EVERY_WIDTH)
@pytest.mark.parametrize("hann", [False, True])
def test_fp32_order_meets_the_gate_by_arithmetic_alone(spectra40, bins, hann):
    """The device's summation order emulated in fp32 on the GPU tests' input (an fp32 spectrum of it), T = 1 and T = 40 blocks, against
    the float64 model of the SAME fp32 spectra under the GPU tests' gate: |mean32 - mean64| <= (log2 G + 8) 2^-23 ref."""
    G = N // bins
    acc, p64, ref, worst = S.Accumulator(), [], [], {}
    for t, X32 in enumerate(spectra40):
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


def per_thread_band_sums(X32, bins, hann, slip=False):
    """spectrum_bands for G = N / bins <= 512 restated thread by thread (spectrum_kernels.hip, from the load to `p`): one row per
    workgroup, one column per thread, explicit `lane`, `wave` and `wsum`, every shuffle a gather by thread index.  No reshape decides
    what is added to what: the partner of thread t in the butterfly is thread t ^ o, and the partner of a wave is the one the kernel names.
    slip: the two mistakes the LDS step invites -- a wave paired with itself (G = 256), the waves 2 and 3 forgotten (G = 512)."""
    X32 = np.asarray(X32, np.complex64)
    n, tile, threads = len(X32), S.TILE, S.THREADS
    g = n // bins
    assert g <= tile and n % tile == 0
    re, im = X32.real.astype(np.float32), X32.imag.astype(np.float32)
    t = np.arange(threads)
    lane, wave = t & 63, t >> 6
    s0 = (np.arange(n // tile) * tile)[:, None] + 2 * t[None, :]                 # [workgroup][thread]: the thread's bins s0, s0 + 1
    ax, ay, bx, by = re[s0], im[s0], re[s0 + 1], im[s0 + 1]
    if hann:
        up, down = np.maximum(t - 1, 0), np.minimum(t + 1, threads - 1)         # __shfl_up / __shfl_down by one lane ...
        lx, ly, rx, ry = bx[:, up], by[:, up], ax[:, down], ay[:, down]
        first, last = lane == 0, lane == 63                                     # ... but for a wave's first and last lane: from memory
        hl, hr = (s0 + n - 1) & (n - 1), (s0 + 2) & (n - 1)
        lx, ly = np.where(first, re[hl], lx), np.where(first, im[hl], ly)
        rx, ry = np.where(last, re[hr], rx), np.where(last, im[hr], ry)
        h, q = np.float32(0.5), np.float32(0.25)
        ax, ay, bx, by = h * ax - q * (lx + bx), h * ay - q * (ly + by), h * bx - q * (ax + rx), h * by - q * (ay + ry)
    s = (ax * ax + ay * ay) + (bx * bx + by * by)
    assert s.dtype == np.float32
    per_band = g // 2
    o = 1
    while o < min(per_band, 64):
        s = s + s[:, t ^ o]
        o <<= 1
    if per_band > 64:
        wsum = s[:, lane == 0]                                                  # wsum[wave] = the sum lane 0 of the wave holds
        assert wsum.shape[1] == threads // 64
        if per_band == 128:
            s = wsum[:, wave & ~1] + wsum[:, wave if slip else wave | 1]
        else:
            s = np.repeat(((wsum[:, 0] + wsum[:, 1]) + (0 if slip else wsum[:, 2] + wsum[:, 3]))[:, None], threads, axis=1)
    owners = t % per_band == 0
    band = (np.arange(n // tile) * (tile // g))[:, None] + (t // per_band)[None, :]
    out = np.zeros(bins, np.float32)
    out[band[:, owners]] = s[:, owners]
    assert sorted(band[:, owners].ravel()) == list(range(bins))                 # every band has one owner
    return out * np.float32(1.0 / (float(n) * float(n) * (0.375 if hann else 1.0)))


@pytest.mark.parametrize("G", [16, 128, 256, 512])
@pytest.mark.parametrize("hann", [False, True])
def test_the_tree_of_the_emulation_is_the_kernels_thread_by_thread(G, hann):
    """emulate_block's reshape-and-halve tree against the per-thread restatement, as uint32: the two ways waves meet through LDS
    (G = 256: wsum[wave & ~1] + wsum[wave | 1], two bands per workgroup; G = 512: (wsum[0] + wsum[1]) + (wsum[2] + wsum[3])), the widest
    band that stays inside a wave, and the narrowest.  Then what the restatement is for: with the partner wave or the pair of waves 2, 3
    taken wrong it no longer equals the emulation, so agreement is not `_tree` agreeing with itself."""
    n = 1 << 13
    X32 = S.spectrum_of(S.make_signal(n, n, seed=23)).astype(np.complex64)
    a, b = S.emulate_block(X32, n // G, hann), per_thread_band_sums(X32, n // G, hann)
    assert a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32)), int((a.view(np.uint32) != b.view(np.uint32)).sum())
    p64 = S.band_powers(X32, n // G, hann)
    ref = S.hann_ref(X32, n // G) if hann else p64
    assert (np.abs(b - p64) <= S.gate(G) * ref).all()
    if G >= 256:
        wrong = per_thread_band_sums(X32, n // G, hann, slip=True)
        assert (np.abs(wrong - p64) > S.gate(G) * ref).mean() > 0.9          # on noise a half band is about the other half: most bands, not all


def test_stage_check_takes_the_emulation_and_refuses_one_wrong_band():
    """check_against_model as the GPU tests call it, fed the emulation in the device's place: it passes; with one band one ulp off it
    fails on the words; with one band off by two gates it fails on the gate; a band of exact zeros (bound 0) passes at 0 and fails above."""
    n, bins, G = 1 << 13, 32, 256
    X32 = S.spectrum_of(S.make_signal(n, n, seed=29)).astype(np.complex64)
    X32[3 * G - 1:4 * G + 1] = 0                                   # band 3 and both its neighbours' edge bins: HANN's reference is 0 there too
    for hann in (False, True):
        p64, ref = S.band_powers(X32, bins, hann)[None], (S.hann_ref(X32, bins) if hann else S.band_powers(X32, bins))[None]
        assert p64[0, 3] == 0 and ref[0, 3] == 0
        acc = S.Accumulator()
        acc.add(S.emulate_block(X32, bins, hann))
        mean, peak = acc.read()
        S.check_against_model("cpu", dict(mean=mean, peak=peak, blocks=1), p64, ref, (mean, peak), G, 1)
        ulp, gates, dust = mean.copy(), mean.copy(), mean.copy()
        ulp[7], gates[7], dust[3] = np.nextafter(mean[7], np.float32(1)), np.float32(mean[7] + 2 * S.gate(G) * ref[0, 7]), np.float32(1e-30)
        # (device words, emulation words): one ulp passes the gate and fails on the words; the other two are handed their own words
        for wrong, emu in ((ulp, mean), (gates, gates), (dust, dust)):
            with pytest.raises(AssertionError):
                S.check_against_model("cpu", dict(mean=wrong, peak=peak, blocks=1), p64, ref, (emu, peak), G, 1)
        assert S.over(np.abs(ulp - p64[0]), S.gate(G) * ref[0]).max() <= 1.0


@pytest.mark.parametrize("side", ["below", "above"])
def test_on_bin_tones_share_out_as_sixths(side):
    """The GPU halo test's input in the float64 model: tones exactly on the bins on one side of the circular wrap, of a wave boundary, of
    a tile boundary and of a tile boundary inside an owner's walk.  From the samples (np.fft of w x) and from the spectrum (three taps)
    a tone leaves 2/3 of its power in its bin and 1/6 in each neighbour, in whatever block of the stream; written out for the bands
    next to each boundary at G = 16 and G = 2048, and for a window that forgets the wrap."""
    n, overlap, amp = 1 << 15, 4099, 0.1
    pos = S.halo_tones(n, side)
    assert pos == ([n - 1, 127, 511, 1023] if side == "below" else [0, 128, 512, 1024])
    x = S.tone_stream(n, 3 * (n - overlap), pos, amp)
    sixth = amp * amp / 6
    total = len(pos) * amp * amp
    near, far = (5 * sixth, sixth) if side == "below" else (sixth, 5 * sixth)      # the band below / above each boundary
    want16 = np.zeros(n // 16)
    for e in S.HALO_EDGES:
        want16[(e // 16 - 1) % (n // 16)], want16[e // 16] = near, far
    want2048 = np.zeros(16)
    want2048[15], want2048[0] = near, 3 * amp * amp + far                          # the three inner tones lie whole in band 0
    for G, want in ((16, want16), (2048, want2048)):
        bins = n // G
        assert np.abs(S.tone_band_powers(n, pos, amp, bins) - want).max() <= 1e-15
        rect = S.tone_band_powers(n, pos, amp, bins, hann=False)
        assert abs(rect.sum() - total) <= 1e-15 and np.count_nonzero(rect) == (len(pos) if G == 16 else 1 + (side == "below"))
        for w in S.windows(x, n, overlap, [1, 2]):                                 # (block 0 begins with a history of zeros: a seam)
            assert np.abs(S.band_powers_from_samples(w, bins, True) - want).max() <= 1e-12 * total
            assert np.abs(S.band_powers(S.spectrum_of(w), bins, True) - want).max() <= 1e-12 * total
            assert np.abs(S.band_powers_from_samples(w, bins) - rect).max() <= 1e-12 * total
    # a neighbour that is not taken round the ends moves the first or the last band by a sixth of a tone
    X = S.spectrum_of(S.windows(x, n, overlap, [1])[0])
    Xw = 0.5 * X
    Xw[1:] -= 0.25 * X[:-1]
    Xw[:-1] -= 0.25 * X[1:]
    nowrap = (np.abs(Xw) ** 2).reshape(n // 16, 16).sum(axis=1) / (float(n) ** 2 * 0.375)
    b = 0 if side == "below" else n // 16 - 1
    assert abs((want16 - nowrap)[b] - sixth) <= 1e-12 * total and np.abs(np.delete(want16 - nowrap, b)).max() <= 1e-12 * total


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
