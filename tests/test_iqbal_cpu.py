"""The wideband I/Q imbalance and DC corrector, the parts that need no GPU (tests/iqbal_f64.py is the model):

  a. every argument check of the four entry points answers HFDL_GPU_EINVAL without a device and leaves the outputs untouched, and the
     ABI is pinned;
  b. the host build of iqbal.h (tests/hostsim/iqbal_check.cpp) against float64: the five sums within 2 (d + 2) 2^-24 of the sum of their
     terms' magnitudes, m and kappa within the bounds iqbal_f64 derives from that, the corrected samples within what follows;
  c. the closed form gives kappa back; d. what is refused is copied word for word;
  e. the decode scenario on the oracle;  f. the host library: the setter's range, hfdl_replay --iq-correct against the stand-in."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import iqbal_f64 as iq
import dumphfdl_amd as hf
from dumphfdl_amd import frontend as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dumphfdl_amd", "host")
EINVAL = -1
SIZES = (1, 63, 4096, 4097, 28672, 1048576 + 4097)      # 1048576 + 4097: 258 chunks, two partial sums for a thread of step 5


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------- a. arguments, ABI

def blocks_call(L, raw=True, n=8, nblocks=2, fmt=0, alpha=0.125, seed=None, hold=0, out=True, recs=True):
    x = np.zeros(64, np.float32)
    y = np.full(64, 7.0, np.float32)
    r = (F.IqbalStats * 4)()
    r[0].blocks = 7
    sd = None if seed is None else np.array(seed, np.float32)
    rc = L.hfdl_gpu_iqbal_blocks(0, x.ctypes.data_as(C.c_void_p) if raw else None, n, nblocks, fmt, alpha, sd.ctypes.data_as(C.c_void_p) if sd is not None else None,
                                 hold, y.ctypes.data_as(C.c_void_p) if out else None, C.cast(r, C.c_void_p) if recs else None)
    return rc, bool((y == 7.0).all() and r[0].blocks == 7)


@pytest.mark.parametrize("case", [dict(raw=False), dict(out=False), dict(recs=False), dict(n=0), dict(n=-3), dict(n=(1 << 24) + 1), dict(nblocks=0), dict(nblocks=65),
                                  dict(fmt=3), dict(fmt=-1), dict(alpha=0.0), dict(alpha=2.0 ** -11), dict(alpha=1.001), dict(alpha=-0.5), dict(alpha=float("nan")),
                                  dict(hold=1), dict(hold=2, seed=(0, 0, 0, 0)), dict(seed=(0.2, 0.2, 0, 0)), dict(seed=(float("nan"), 0, 0, 0)),
                                  dict(seed=(0, 0, float("inf"), 0)), dict(seed=(0, 0, 0, float("nan")))])
def test_iqbal_blocks_checks_every_argument_before_any_device_work(case):
    rc, untouched = blocks_call(hf.load(), **case)
    assert rc == EINVAL and untouched, case


@pytest.mark.parametrize("alpha", [-1.0, 2.0 ** -11, 1.5, float("nan"), float("inf"), 0.125, 0.0])
def test_a_null_handle_is_refused(alpha):
    L = hf.load()
    assert L.hfdl_gpu_frontend_iqbal_enable(None, -1, alpha) == EINVAL
    assert L.hfdl_gpu_frontend_iqbal_seed(None, 0, 0.01, 0.01, 0.0, 0.0, 0) == EINVAL
    assert L.hfdl_gpu_frontend_iqbal_seed(None, 0, 0.3, 0.0, 0.0, 0.0, 0) == EINVAL
    st = F.IqbalStats()
    st.blocks = 7
    assert L.hfdl_gpu_frontend_iqbal_stats(None, 0, C.byref(st)) == EINVAL and st.blocks == 7


def test_abi_is_pinned():
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c11", "-D_GNU_SOURCE", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + inc, os.path.join(ROOT, "tests", "abi", "hfdl_gpu_iqbal_abi.c")])
    assert C.sizeof(F.IqbalStats) == 48 == iq.REC.itemsize and F.IqbalStats.kappa_re.offset == 16 and F.IqbalStats.valid.offset == 40
    assert [n for n, _ in F.IqbalStats._fields_] == list(iq.REC.names[:7]) + ["image_rejection_db", "valid", "hold"]
    names = ("hfdl_gpu_frontend_iqbal_enable", "hfdl_gpu_frontend_iqbal_seed", "hfdl_gpu_frontend_iqbal_stats", "hfdl_gpu_iqbal_blocks")
    dyn = subprocess.run(["nm", "-D", "--defined-only", hf.lib_path()], capture_output=True, text=True, check=True).stdout
    for name in names:
        assert name in F.EXPORTS and (" T " + name) in dyn, name
    src = open(os.path.join(HOST, "frontend.c")).read()
    assert "#pragma weak hfdl_gpu_frontend_iqbal_enable" in src and "#pragma weak hfdl_gpu_frontend_iqbal_stats" in src


# ---------------------------------------------------------------- b. the documented order, built for the host

@pytest.fixture(scope="module")
def check(tmp_path_factory):
    d = tmp_path_factory.mktemp("iqbal")
    return iq.build_host_check(d), d


@pytest.fixture(scope="module")
def impaired_noise():
    """proper noise (sigma 0.1) through the scenario's kappa and DC: three blocks of the largest size"""
    x = iq.impair(iq.proper_noise(3 * max(SIZES), 3), iq.KAPPA, iq.DC)
    x.setflags(write=False)
    return x


worst = dict(kappa=0.0, m=0.0)


@pytest.mark.parametrize("n", SIZES)
def test_host_build_agrees_with_float64(check, impaired_noise, n):
    exe, d = check
    nblocks = 3 if n > 28672 else 4
    x = impaired_noise[:nblocks * n] if n > 28672 else impaired_noise[5 * n:(5 + nblocks) * n]
    y, recs, sums, modes = iq.host_blocks(exe, d, x, n)
    depth = F.blank_sum_depth(n)
    eps = iq.sum_bound(depth)
    model = iq.Model()
    for b in range(nblocks):
        blk = x[b * n:(b + 1) * n]
        t = iq.terms64(blk)
        S64, T = t.sum(axis=1), np.abs(t).sum(axis=1)
        err = np.abs(sums[b].astype(np.float64) - S64)
        print("n %d block %d: sums' errors / bound %s" % (n, b, np.array2string(err / np.maximum(eps * T, 1e-300), precision=3)))
        assert (err <= eps * T).all(), (n, b, err, eps * T)
        want, rec = model.step(blk)
        got = recs[b]
        # the test input keeps the model away from the two thresholds, so the last bits cannot decide whether there is an estimate
        if b > 0 and rec["power"] != 0:
            m, c2, p2 = model.A
            assert rec["power"] > 1e-4 * p2.real and abs(abs(c2 - m * m) ** 2 / rec["power"] ** 2 - 0.25) > 1e-3, "test input too close to a threshold"
        assert bool(got["valid"]) == rec["valid"] and (got["blocks"], got["refused"]) == (rec["blocks"], rec["refused"]), (n, b, got, rec)
        assert modes[b] == (2 if rec["valid"] else 1)
        if not rec["valid"]:
            assert (bits(y[b * n:(b + 1) * n]) == bits(blk)).all()
            continue
        k32, m32 = complex(got["kappa_re"], got["kappa_im"]), complex(got["dc_re"], got["dc_im"])
        kb, mb = iq.kappa_bound(depth, rec["p2max"], rec["power"]), iq.m_bound(depth, rec["p2max"], rec["dc"])
        ek, em = abs(k32 - rec["kappa"]), abs(m32 - rec["dc"])
        worst["kappa"], worst["m"] = max(worst["kappa"], ek), max(worst["m"], em)
        print("n %d block %d: |kappa32 - kappa64| = %.3g (bound %.3g), |m32 - m64| = %.3g (bound %.3g), P %.6g" % (n, b, ek, kb, em, mb, rec["power"]))
        assert ek <= kb and em <= mb, (n, b)
        assert abs(float(got["power"]) - rec["power"]) <= (1 + 2 * np.sqrt(2)) * eps * rec["p2max"] + 4 * iq.U * rec["p2max"]
        # y = d - kappa conj(d): the errors of m and kappa, and six roundings of quantities no larger than |x| + |m|
        mag = np.abs(blk.astype(np.complex128)) + abs(rec["dc"])
        tol = (1 + abs(rec["kappa"])) * mb + kb * mag + 8 * iq.U * mag
        assert (np.abs(y[b * n:(b + 1) * n].astype(np.complex128) - want.astype(np.complex128)) <= tol).all(), (n, b)
    print("largest so far: |kappa32 - kappa64| = %.3g, |m32 - m64| = %.3g" % (worst["kappa"], worst["m"]))
    # measured over these sizes: 1.42e-8 and 1.75e-9; four times that
    assert worst["kappa"] <= 4 * 1.42e-8 and worst["m"] <= 4 * 1.75e-9


def test_sum_depth_is_the_blankers():
    assert F.blank_sum_depth(1) == 26 and F.blank_sum_depth(28672) == 26 and F.blank_sum_depth(1048576 + 4097) == 27


# ---------------------------------------------------------------- c. the closed form

@pytest.mark.parametrize("kappa", [0.0, 0.03 * np.exp(0.7j), 0.2, -0.2j, 0.2 * np.exp(2.5j), 1e-4 * np.exp(-1j)])
@pytest.mark.parametrize("dc", [0.0, 0.02 + 0.01j, -3.0 + 5.0j])
def test_closed_form_gives_kappa_back(kappa, dc):
    """s exactly proper (its sample mean and its sample mean of s^2 removed): kappa and the DC offset come back to 1e-9"""
    rng = np.random.default_rng(12)
    n = 4096
    s = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    s -= s.mean()
    s -= np.conj(s) * np.mean(s * s) / (2 * np.mean(np.abs(s) ** 2))            # E s^2 -> 0 to first order ...
    for _ in range(4):                                                          # ... and to rounding
        s -= s.mean()
        s -= np.conj(s) * np.mean(s * s) / (2 * np.mean(np.abs(s) ** 2))
    assert abs(np.mean(s * s)) < 1e-15 and abs(s.mean()) < 1e-15
    x = s + kappa * np.conj(s) + dc
    valid, got, P = iq.estimate(x.mean(), np.mean(x * x), np.mean(np.abs(x) ** 2))
    assert valid and abs(got - kappa) <= 1e-9 and abs(x.mean() - dc) <= 1e-9
    d = x - x.mean()
    assert np.abs((d - got * np.conj(d)) - (1 - abs(kappa) ** 2) * s).max() <= 1e-8


# ---------------------------------------------------------------- d. refusals

def test_what_is_refused_is_copied_word_for_word(check):
    exe, d = check
    n = 4097
    noise = iq.impair(iq.proper_noise(4 * n, 9), iq.KAPPA, iq.DC)
    # a real-valued stream: |C| = P, the rule would cancel the signal against itself
    real = noise.real.astype(np.complex64)
    y, recs, _, modes = iq.host_blocks(exe, d, real, n)
    assert modes == [1, 1, 1, 1] and (bits(y) == bits(real)).all() and recs[-1]["refused"] == 4 and not recs["valid"].any()
    # all zero: P = 0
    zero = np.zeros(3 * n, np.complex64)
    y, recs, _, modes = iq.host_blocks(exe, d, zero, n)
    assert modes == [1, 1, 1] and not bits(y).any()
    # a NaN block first: no estimate yet, so it is copied, payload and all, and it leaves none behind either
    nan = noise.copy()
    nan[:n][100] = np.complex64(complex(np.nan, 1.0))
    nan.view(np.uint32)[2 * 200] = 0x7FC01234
    y, recs, _, modes = iq.host_blocks(exe, d, nan, n)
    assert modes == [1, 1, 2, 2] and (bits(y[:2 * n]) == bits(nan[:2 * n])).all()
    # ... and a NaN block in the middle: the block after it is corrected from the state before it -- the first block's alone
    nan = noise.copy()
    nan[n:2 * n][7] = np.complex64(complex(0.0, np.inf))
    y, recs, _, modes = iq.host_blocks(exe, d, nan, n)
    y_ref, recs_ref, _, _ = iq.host_blocks(exe, d, noise, n)
    assert modes == [1, 2, 2, 2]
    assert (recs[2]["kappa_re"], recs[2]["kappa_im"], recs[2]["dc_re"], recs[2]["dc_im"]) == (recs[1]["kappa_re"], recs[1]["kappa_im"], recs[1]["dc_re"], recs[1]["dc_im"])
    assert (bits(y[:n]) == bits(y_ref[:n])).all() and (recs_ref[2]["kappa_re"], recs_ref[2]["dc_re"]) != (recs[2]["kappa_re"], recs[2]["dc_re"])
    want, _ = iq.correct_stream(nan, n)
    fin = np.isfinite(want[2 * n:].view(np.float32))
    assert fin.all() and np.abs(y[2 * n:] - want[2 * n:]).max() < 1e-6
    # a held preset is applied from the first block on and never moves; a seed is used as given for one block
    y, recs, _, modes = iq.host_blocks(exe, d, noise, n, seed=(iq.KAPPA, iq.DC), hold=True)
    assert modes == [2, 2, 2, 2] and recs["hold"].all() and len(set(zip(recs["kappa_re"], recs["kappa_im"], recs["dc_re"], recs["dc_im"]))) == 1
    assert recs[0]["kappa_re"] == np.float32(iq.KAPPA.real) and recs[0]["dc_im"] == np.float32(iq.DC.imag)
    want, _ = iq.correct_stream(noise, n, seed=(iq.KAPPA, iq.DC), hold=True)
    assert np.abs(y - want).max() < 1e-6
    y, recs, _, modes = iq.host_blocks(exe, d, noise, n, seed=(iq.KAPPA, iq.DC), hold=False)
    want, mrecs = iq.correct_stream(noise, n, seed=(iq.KAPPA, iq.DC), hold=False)
    assert modes == [2, 2, 2, 2] and not recs["hold"].any() and recs[0]["kappa_re"] == np.float32(iq.KAPPA.real)
    assert np.abs(y - want).max() < 1e-6 and all(abs(complex(r["kappa_re"], r["kappa_im"]) - m["kappa"]) < 1e-6 for r, m in zip(recs, mrecs))


# ---------------------------------------------------------------- e. the decode scenario on the oracle

def test_scenario_on_the_oracle(oracle):
    """six weak frames on three channels, three 5 kHz bands of rms 0.4 where the channels' images come from,
    kappa = 0.03 e^0.7j, DC 0.02 + 0.01j.  Undistorted: all decoded.  Impaired: at most half.  Impaired, corrected by the model at
    alpha = 1/8: all decoded, and so is the undistorted stream through the corrector."""
    s = iq.scenario()
    sent = s["sent"]
    n = oracle.geometry(iq.FS)[2].input_size
    assert iq.delivered(iq.oracle_pdus(oracle, s["clean"]), sent) == len(sent) == 6
    got = iq.delivered(iq.oracle_pdus(oracle, s["impaired"]), sent)
    print("impaired: %d of 6" % got)
    assert got <= 3
    y, recs = iq.correct_stream(s["impaired"], n)
    assert iq.delivered(iq.oracle_pdus(oracle, y), sent) == 6
    errs = [abs(r["kappa"] - iq.KAPPA) / abs(iq.KAPPA) for r in recs[1:]]
    print("kappa: off by %.2f %% at the first corrected block, %.2f %% at worst" % (100 * errs[0], 100 * max(errs)))
    assert recs[-1]["refused"] == 1 and max(errs) < 0.02
    y, recs = iq.correct_stream(s["clean"], n)
    assert iq.delivered(iq.oracle_pdus(oracle, y), sent) == 6 and max(abs(r["kappa"]) for r in recs) < 1e-3


# ---------------------------------------------------------------- f. the host library

def test_host_setter_takes_0_and_the_alphas():
    H = C.CDLL(os.path.join(ROOT, "dumphfdl_amd", "libhfdl_host.so"))
    f = H.hfdl_frontend_set_iq_correction
    f.argtypes = [C.c_float]
    for alpha, want in ((0.125, 0), (2.0 ** -10, 0), (1.0, 0), (2.0 ** -11, -1), (1.01, -1), (-0.125, -1), (float("nan"), -1), (0.0, 0)):
        assert f(alpha) == want, alpha


def test_replay_iq_correct_is_refused_by_a_library_without_it(tmp_path):
    """hfdl_replay --iq-correct against the plain stand-in (tests/hostsim/gpu_standin.c has no corrector): the message, a non-zero
    status, no crash; an alpha out of range is refused by the option itself; without the option nothing has changed."""
    exe = str(tmp_path / "replay")
    subprocess.check_call(["gcc", "-g", "-O1", "-std=c11", "-D_GNU_SOURCE", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", HOST] +
                          [os.path.join(HOST, f) for f in ("hfdl_replay.c", "ring.c", "blocks.c", "input.c", "sink.c", "frontend.c")] +
                          [os.path.join(ROOT, "tests", "hostsim", "gpu_standin.c"), "-o", exe, "-lpthread", "-lm"])
    src = tmp_path / "in.cs16"
    np.random.default_rng(5).integers(0, 256, (10 * 3072 + 100) * 4, dtype=np.uint8).tofile(src)

    def run(*options):
        cmd = [exe, "--iq-file", str(src), "--sample-rate", "250000", "--sample-format", "CS16", "--read-buffer-size", "4096", "--centerfreq", "10000"] + \
            list(options) + ["10010", "10020"]
        return subprocess.run(cmd, capture_output=True, text=True, timeout=60)
    out = run("--iq-correct", "0.125")
    assert out.returncode == 1 and "iq-correct: this GPU library has no I/Q imbalance corrector" in out.stderr, (out.returncode, out.stderr)
    out = run("--iq-correct", "3")
    assert out.returncode == 1 and "--iq-correct wants an alpha of 1/1024 to 1" in out.stderr
    out = run()
    assert out.returncode == 0 and "iq-correct" not in out.stderr
