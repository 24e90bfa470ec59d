"""Real-sampled input, the parts that need no GPU (tests/real_f64.py is the model):

  a. the two identities in float64 -- the untangle against numpy.fft.fft, the even / odd tap combine against the zero-padded 2N'
     transform -- and the blockwise definition in its two forms (every sample of the N'-point inverse transform picked / a size-M inverse
     transform of the folded rows), each <= 1e-12 relative;
  b. the planner mapping: the host build of real_input.h (tests/hostsim/real_input_check.cpp) agrees field by field with
     plan_block(fs') as the oracle states it, and its real-rate taps are the oracle's design bit for bit;
  c. the pair index map covers every bin once, k = 0 and k = N'/2 included, N' = 2^4 .. 2^23; the host build of the untangle and of
     the combine in fp32 against float64;
  d. the gap from the blockwise definition to the global models, REPORTED (DESIGN.md section 4.16 quotes it);
  e. every argument check answers HFDL_GPU_EINVAL without a device; the ABI."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import ddc_f64 as M
import real_f64 as R
import dumphfdl_amd as hf
from dumphfdl_amd import frontend as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
RATES = (96_000, 500_000, 2_800_000, 80_000_000)


def toy_plan(offsetbin=-1236):
    """N' = 2^14, overlap' = N'/4, 64 alias rows"""
    n, ov, pre = 1 << 14, 1 << 12, 64
    m = n // pre
    return types.SimpleNamespace(fft_size=n, overlap_length=ov, input_size=n - ov, pre_decimation=pre, post_decimation=2, fft_inv_size=m, scrap=ov // pre,
                                 post_input_size=m - ov // pre, offsetbin=offsetbin, nco_rate=np.float32(0.0123), taps_length=ov + 1)


def toy_taps(plan, centre, rng):
    """a windowed-sinc band-pass at the real rate, 2 overlap' + 1 complex taps, +- 0.25 / decimation' wide, its samples perturbed by 1e-4"""
    L = 2 * plan.overlap_length + 1
    t = np.arange(L) - L // 2
    fc = 0.25 / (plan.pre_decimation * plan.post_decimation)
    return np.sinc(2 * fc * t) * np.hamming(L) * (2 * fc) * np.exp(2j * np.pi * centre * np.arange(L)) * (1 + 1e-4 * rng.standard_normal(L))


# ---------------------------------------------------------------- a. identities

def test_untangle_is_the_real_transform_on_its_non_negative_frequencies():
    rng = np.random.default_rng(1)
    for logn in (4, 9, 14):
        n = 1 << logn
        x = rng.standard_normal(2 * n)
        want = np.fft.fft(x)[:n]
        got = R.untangle(np.fft.fft(x[0::2] + 1j * x[1::2]))
        err = np.abs(got - want).max() / np.abs(want).max()
        print("N' = 2^%d: untangle off numpy.fft.fft by %.3g" % (logn, err))
        assert err <= 1e-12
        assert abs(got[0].imag) <= 1e-12 * np.abs(want).max() and np.allclose(got, np.fft.rfft(x)[:n], rtol=0, atol=1e-12 * np.abs(want).max())


def test_even_odd_tap_combine_is_the_zero_padded_transform():
    rng = np.random.default_rng(2)
    plan = toy_plan()
    h = toy_taps(plan, 0.1234, rng)
    got = 0.5 * R.tap_combine(h, plan.fft_size)
    want = R.stored_filter(h, plan)
    err = np.abs(got - want).max() / np.abs(want).max()
    print("tap combine off the 2N' transform by %.3g" % err)
    assert err <= 1e-12


def test_blockwise_definition_in_its_two_forms():
    rng = np.random.default_rng(3)
    plan = toy_plan()
    x = rng.standard_normal(2 * plan.input_size * 3)
    h = toy_taps(plan, 0.25 + plan.offsetbin / (2.0 * plan.fft_size), rng)
    a = R.real_ddc_reference(x, h, plan)
    b = R.real_ddc_reference(x, h, plan, fast=True)
    assert len(a) == 3 and all(len(v) == plan.post_input_size // 2 for v in a)
    for k in range(3):
        e = M.errors(b[k], a[k])
        print("block %d: folded form off the definition by rms %.3g max %.3g" % (k, e[0], e[1]))
        assert e[1] <= 1e-12
    assert np.sqrt(np.mean(np.abs(a[1]) ** 2)) > 1e-3          # (the channel holds signal: the toy band-pass sits on the mixer's bin)


# ---------------------------------------------------------------- b. planner mapping

@pytest.fixture(scope="module")
def check(tmp_path_factory):
    d = tmp_path_factory.mktemp("real_input")
    return R.build_host_check(d), d


@pytest.mark.parametrize("fs_r", RATES)
def test_planner_mapping_is_plan_block_of_the_equivalent_stream(check, oracle, fs_r):
    exe, d = check
    base = 0 if fs_r != 500_000 else 7_000_000
    fs, centre = R.equiv(fs_r, base)
    dec, tbw, d0 = oracle.geometry(fs)
    for freq in R.channel_freqs(fs_r, base, d0.overlap_length):
        hp = R.host_plan(exe, fs_r, base, freq)
        shift = np.float32(centre - (freq + 1440)) / np.float32(fs)          # what design_channel forms for a complex receiver on (fs', centre')
        want = oracle.fastddc_init(tbw, dec, float(shift))
        assert (hp["fs"], hp["centre"], hp["dec"]) == (fs, centre, dec) and hp["tbw"] == np.float32(tbw)
        assert hp["shift"] == shift, (fs_r, freq)                           # fs_r a multiple of four: the very quotient
        got = (hp["n"], hp["overlap"], hp["input_size"], hp["pre"], hp["post"], hp["m"], hp["scrap"], hp["post_input_size"], hp["taps_length"], hp["offsetbin"])
        assert got == (want.fft_size, want.overlap_length, want.input_size, want.pre_decimation, want.post_decimation, want.fft_inv_size, want.scrap,
                       want.post_input_size, want.taps_length, want.offsetbin), (fs_r, freq)
        assert (hp["sindelta"], hp["cosdelta"], hp["rate"]) == (np.float32(want.nco_sindelta), np.float32(want.nco_cosdelta), np.float32(want.nco_rate))
        assert hp["taps_real"] == 2 * want.overlap_length + 1
        lo, hi = R.band32(fs_r, base, freq, dec)
        assert (hp["lowcut"], hp["highcut"]) == (lo, hi)
        assert want.offsetbin % want.v == 0 and (2 * want.overlap_length) * want.v == 2 * want.fft_size          # the phase-continuity condition, as today
        c = float(lo + hi) / 2
        assert abs(c - (0.25 - float(shift) / 2)) < 1e-6                     # the same band, seen from the two rates
    # a rate that is even and no multiple of four: centre' is taken exactly, half a hertz above the integer the geometry reports
    hp = R.host_plan(exe, 96_002, 0, 20_000)
    assert hp["centre"] == 24_000 and abs(float(hp["shift"]) - (24_000.5 - 21_440) / 48_001) < 1e-7


@pytest.mark.parametrize("fs_r", RATES[:3])
def test_real_rate_taps_are_the_oracles_design_bit_for_bit(check, oracle, fs_r):
    exe, d = check
    fs, _ = R.equiv(fs_r, 0)
    _, _, d0 = oracle.geometry(fs)
    for freq in R.channel_freqs(fs_r, 0, d0.overlap_length)[::3]:
        plan, taps = R.channel_plan(oracle, fs_r, 0, freq)
        h, split = R.host_taps(exe, d, fs_r, 0, freq)
        T = plan.taps_length
        assert len(h) == 2 * T - 1 and len(split) == 2 * T
        assert np.array_equal(h.view(np.uint32), taps.astype(np.complex64).view(np.uint32))
        assert np.array_equal(split[:T], h[0::2]) and np.array_equal(split[T:2 * T - 1], h[1::2]) and split[-1] == 0


def test_library_and_host_build_design_their_taps_with_one_function():
    """Bit-equality of the library's time-domain taps with the host build of real_input.h holds by construction: band, design_bandpass and
    split are ONE function of the header, real_design_taps, and it is what design_channel (the library: create and retune) and
    tests/hostsim/real_input_check.cpp (the host build, whose words the test above holds to the oracle's design) both call.  Neither file
    spells the sequence out for itself."""
    lib = open(os.path.join(ROOT, "dumphfdl_amd", "csrc", "frontend_create.cpp")).read()
    sim = open(os.path.join(ROOT, "tests", "hostsim", "real_input_check.cpp")).read()
    for name, src in (("frontend_create.cpp", lib), ("real_input_check.cpp", sim)):
        assert src.count("real_design_taps(") == 1, name
        assert "real_split_taps(" not in src and src.count("design_bandpass(") == (1 if name == "frontend_create.cpp" else 0), name       # (the library's one call is the complex path's)
    for other in ("hfdl_gpu.cpp", "frontend_query.cpp", "frontend_options.cpp", "stages.cpp"):
        assert "design_bandpass(" not in open(os.path.join(ROOT, "dumphfdl_amd", "csrc", other)).read(), other


def test_the_oracle_decodes_six_of_six_on_the_complex_stream(oracle):
    """The condition on the input of the end-to-end GPU tests (tests/test_gpu_real_input.py uses the same real_f64.decode_scene): at the
    chosen in-channel SNR the oracle decodes every frame sent on the complex stream at (fs' = 250 ksps, centre'), and the real stream made
    of it fits int16."""
    s = R.decode_scene(oracle)
    sent = sorted((b["freq"], b["mode"], b["octets"]) for b in s["sent"])
    assert len(sent) == 6 and len(s["want"]) == 6
    assert [(f, m, o[:len(so)]) for (f, m, o), (_, _, so) in zip(s["want"], sent)] == sent
    assert s["fs"] == 250_000 and len(s["v16"]) == 2 * len(s["w"]) == 2 * s["nblk"] * s["n"] and s["v16"].dtype == np.int16


# ---------------------------------------------------------------- c. pair indices; the host build in fp32

@pytest.mark.parametrize("logn", range(4, 24))
def test_pair_index_map_covers_every_bin_once(check, logn):
    out = subprocess.run([check[0], "pairs", str(logn)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


@pytest.mark.parametrize("logn", (4, 10, 11, 16))
def test_host_build_of_untangle_and_combine_against_float64(check, logn):
    """fp32, one rounding per operation: five on the way from Z to X, against |Z| terms of the size of the largest: 8 x 2^-24 of the
    spectrum's largest magnitude bounds every element (the twiddle's own rounding included)"""
    exe, d = check
    rng = np.random.default_rng(logn)
    n = 1 << logn
    z = (rng.standard_normal(2 * n) + 1j * rng.standard_normal(2 * n)).astype(np.complex64)
    for mode, src, want in (("untangle", z[:n], R.untangle(z[:n])), ("combine", z, 0.5 * (z[:n].astype(np.complex128) + np.exp(-1j * np.pi * np.arange(n) / n) * z[n:]))):
        a, b = os.path.join(str(d), "in.bin"), os.path.join(str(d), "out.bin")
        src.tofile(a)
        subprocess.check_call([exe, mode, a, b, str(logn)])
        got = np.fromfile(b, np.complex64)
        err = np.abs(got - want).max() / np.abs(z).max()
        print("N' = 2^%d %s: host fp32 off float64 by %.3g of the largest input" % (logn, mode, err))
        assert len(got) == n and err <= 8 * 2.0 ** -24


def test_host_check_under_the_sanitizers(check, tmp_path):
    """the stand-alone program, built with -fsanitize=address,undefined and run as its own process"""
    exe = R.build_host_check(tmp_path, sanitize=True)
    for args in (["pairs", "4"], ["pairs", "12"], ["plan", "96000", "0", "20000"], ["taps", "96000", "0", "20000", str(tmp_path / "t.bin")]):
        out = subprocess.run([exe] + args, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
    z = np.arange(64, dtype=np.float32)
    z.tofile(tmp_path / "z.bin")
    assert subprocess.run([exe, "untangle", str(tmp_path / "z.bin"), str(tmp_path / "x.bin"), "4"], capture_output=True).returncode == 0
    assert subprocess.run([exe, "combine", str(tmp_path / "z.bin"), str(tmp_path / "x.bin"), "4"], capture_output=True).returncode == 0


# ---------------------------------------------------------------- d. the gap to the global models (reported, not gated)

def test_gap_from_the_blockwise_definition_to_the_global_models_is_reported():
    """Five interferers 60 dB above an in-band tone, one within 1 % of DC and one within 1 % of Nyquist.  Printed: the distance (relative
    RMS per block, blocks 1 .. 4) from the blockwise definition to the same convolution on the whole record's analytic signal, and to the
    full direct form h * x, images included.  The definition is what the device is gated against; these two figures say how far that is
    from the two things one might have wanted instead."""
    rng = np.random.default_rng(4)
    plan = toy_plan()
    n, ins = plan.fft_size, plan.input_size
    nblk = 6
    t = np.arange(2 * ins * nblk, dtype=np.float64)
    f_ch = 0.25 + plan.offsetbin / (2.0 * n)                 # cycles per real sample: the mixer's bin
    h = toy_taps(plan, f_ch, np.random.default_rng(5))
    x =1e-3 * np.cos(2 * np.pi * (f_ch + 0.001) * t + 0.3) + 1e-4 * rng.standard_normal(len(t))
    for f, ph in ((0.005 * 0.5, 0.1), (0.5 - 0.004 * 0.5, 0.7), (0.081, 1.1), (0.333, 2.0), (0.447, 2.9)):
        x = x + 1.0 * np.cos(2 * np.pi * f * t + ph)
    blocks = [1, 2, 3, 4]
    a = R.real_ddc_reference(x, h, plan, blocks=blocks, fast=True)
    g = R.global_reference(x, h, plan, blocks)
    gi = R.global_reference(x, h, plan, blocks, images=True)
    ea = [M.errors(a[i], g[i])[0] for i in range(len(blocks))]
    ei = [M.errors(a[i], gi[i])[0] for i in range(len(blocks))]
    print("REPORTED blockwise -> global analytic-signal model: relative RMS %.3g .. %.3g" % (min(ea), max(ea)))
    print("REPORTED blockwise -> full direct form h * x:        relative RMS %.3g .. %.3g" % (min(ei), max(ei)))
    assert all(np.isfinite(ea)) and all(np.isfinite(ei))


# ---------------------------------------------------------------- e. arguments, ABI

def create_real(L, out=True, fs_r=96_000, nrx=1, bases=(0,), freqs=(20_000,), counts=(1,)):
    h = C.c_void_p(7)
    b = np.array(bases, np.int32) if bases is not None else None
    f = np.array(freqs, np.int32) if freqs is not None else None
    c = np.array(counts, np.int32) if counts is not None else None
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    rc = L.hfdl_gpu_frontend_create_real(C.byref(h) if out else None, 0, fs_r, nrx, p(b), p(f), p(c))
    return rc, h.value


@pytest.mark.parametrize("case", [dict(fs_r=96_001), dict(fs_r=21_598), dict(fs_r=0), dict(fs_r=-96_000), dict(freqs=(48_000,)), dict(freqs=(-10,)), dict(freqs=(0,)),
                                  dict(bases=(5_000_000,), freqs=(4_999_000,)), dict(out=False), dict(bases=None), dict(freqs=None), dict(counts=None),
                                  dict(nrx=0), dict(nrx=65), dict(counts=(0,)), dict(bases=(2**31 - 1,)), dict(bases=(2**31 - 40_000,), freqs=(2**31 - 20_000,)),
                                  dict(bases=(-2**31,)), dict(bases=(-2**30 - 1,), freqs=(-2**30 + 20_000,)), dict(nrx=2, bases=(0, 1_000_000), freqs=(20_000, 20_000), counts=(1, 1))])
def test_create_real_checks_every_argument_before_a_device_is_selected(case):
    rc, h = create_real(hf.load(), **case)
    assert rc == EINVAL and h in (None, 7), (case, rc, hf.load().hfdl_gpu_last_error())


def test_a_null_handle_is_refused_and_the_formats_are_named():
    L = hf.load()
    a, b = C.c_int32(5), C.c_int32(5)
    assert L.hfdl_gpu_frontend_real_input(None, C.byref(a), C.byref(b)) == EINVAL and (a.value, b.value) == (5, 5)
    buf = np.zeros(16, np.int16)
    for fmt in (F.SFMT_RS16, F.SFMT_RF32):
        assert L.hfdl_gpu_frontend_push_block_raw(None, buf.ctypes.data_as(C.c_void_p), 16, fmt, 0) == EINVAL
        assert L.hfdl_gpu_frontend_prefetch_block_raw(None, buf.ctypes.data_as(C.c_void_p), 16, fmt) == EINVAL
        assert L.hfdl_gpu_frontend_push_blocks_raw(None, None, 16, fmt, 0) == EINVAL
    assert (F.SFMT_RS16, F.SFMT_RF32) == (3, 4)


def test_host_setter_and_its_refusals(tmp_path):
    """hfdl_frontend_set_real_input takes -1 (off) and 0 .. 2 000 000 kHz.  With the real library underneath, fft_create() refuses real
    input together with the I/Q corrector -- a check that needs no device; hfdl_replay --real-input against the plain stand-in
    (tests/hostsim/gpu_standin.c has no real input) is refused with the library's message, and the option refuses what it cannot take."""
    HOST = os.path.join(ROOT, "dumphfdl_amd", "host")
    H = C.CDLL(os.path.join(ROOT, "dumphfdl_amd", "libhfdl_host.so"))
    f = H.hfdl_frontend_set_real_input
    f.argtypes = [C.c_int32]
    for base, want in ((0, 0), (5000, 0), (2_000_000, 0), (2_000_001, -1), (-2, -1), (-1, 0)):
        assert f(base) == want, base
    H.hfdl_frontend_set_iq_correction.argtypes = [C.c_float]
    H.fft_create.argtypes, H.fft_create.restype = [C.c_int32, C.c_float], C.c_void_p
    H.fft_destroy.argtypes = [C.c_void_p]
    assert f(0) == 0 and H.hfdl_frontend_set_iq_correction(0.125) == 0
    assert H.fft_create(32, 0.001) is None                               # real input + I/Q correction: refused at create
    assert H.hfdl_frontend_set_iq_correction(0.0) == 0
    blk = H.fft_create(32, 0.001)
    assert blk is not None
    H.fft_destroy(blk)
    assert f(-1) == 0
    src = open(os.path.join(HOST, "frontend.c")).read()
    assert "#pragma weak hfdl_gpu_frontend_create_real" in src
    exe = str(tmp_path / "replay")
    subprocess.check_call(["gcc", "-g", "-O1", "-std=c11", "-D_GNU_SOURCE", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", HOST] +
                          [os.path.join(HOST, s) for s in ("hfdl_replay.c", "ring.c", "blocks.c", "input.c", "sink.c", "frontend.c")] +
                          [os.path.join(ROOT, "tests", "hostsim", "gpu_standin.c"), "-o", exe, "-lpthread", "-lm"])
    raw = tmp_path / "in.rs16"
    np.random.default_rng(5).integers(0, 256, (10 * 3072 + 100) * 4, dtype=np.uint8).tofile(raw)

    def run(*options, fmt="CS16", rate="500000"):
        cmd = [exe, "--iq-file", str(raw), "--sample-rate", rate, "--sample-format", fmt, "--read-buffer-size", "4096"] + list(options) + ["10010", "10020"]
        return subprocess.run(cmd, capture_output=True, text=True, timeout=60)
    out = run("--real-input=9900")
    assert out.returncode == 1 and "real-input: this GPU library has no real-sampled input" in out.stderr, (out.returncode, out.stderr)
    for options, kw in ((("--real-input=-5",), {}), (("--real-input=x",), {}), (("--real-input=1e12",), {}), (("--real-input=2000000",), dict(rate="400000000")), (("--real-input", "--centerfreq", "10000"), {}), (("--real-input",), dict(fmt="CU8")),
                        (("--real-input",), dict(rate="500001")), (("--real-input",), dict(rate="21598"))):
        out = run(*options, **kw)
        assert out.returncode == 1 and "--real-input" in out.stderr, (options, kw, out.stderr)
    out = run("--centerfreq", "10000", rate="250000")
    assert out.returncode == 0 and "real-input" not in out.stderr


def test_abi_is_pinned():
    hdr = open(os.path.join(ROOT, "include", "hfdl_gpu.h")).read()
    assert "#define HFDL_GPU_SFMT_RS16 3" in hdr and "#define HFDL_GPU_SFMT_RF32 4" in hdr
    dyn = subprocess.run(["nm", "-D", "--defined-only", hf.lib_path()], capture_output=True, text=True, check=True).stdout
    for name in ("hfdl_gpu_frontend_create_real", "hfdl_gpu_frontend_real_input"):
        assert name in F.EXPORTS and (" T " + name) in dyn and name in hdr, name
    assert issubclass(F.RealFrontend, F.MultiFrontend) and hf.RealFrontend is F.RealFrontend
    host = open(os.path.join(ROOT, "include", "hfdl_host.h")).read()
    assert "int           hfdl_frontend_set_real_input(int32_t base_khz);" in host
