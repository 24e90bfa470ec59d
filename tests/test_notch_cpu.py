"""The adaptive carrier canceller, the parts that need no GPU (tests/notch_f64.py has the float64 model and the
scenario, tests/hostsim/notch_check.cpp is the host build of dumphfdl_amd/csrc/notch.h):

  a. the host build, compiled with the address and undefined-behaviour sanitizers, agrees with itself however a stream is cut into rows;
  b. fp32 against float64 on the scenario's inputs;
  c. ten million samples, with and without a tone: finite, far below the reset bound, no reset -- the case against tap leakage;
  d. the guards: zeros, a NaN sample, taps beyond the bound;
  e. the decode scenario on the oracle at 7812.5 and 9765.625 sps;
  f. the interface: exports, ABI, argument checks without a device, the host library's setter, hfdl_replay --notch against a stand-in
     GPU library without the entry points and against one with them."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import notch_f64 as nf
import dumphfdl_amd as hf
from dumphfdl_amd import frontend as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dumphfdl_amd", "host")
EINVAL = -1

# max |y32 - y64| / rms(x) over the scenario's six inputs (three cases at 7812.5 and 9765.625 sps), as measured with this host build:
# 7.6e-07, 8.4e-07, 1.12e-06 and 8.6e-07, 9.3e-07, 1.19e-06.  Rounding noise through a contractive recurrence: it depends on the
# realisation, hence a factor over the measured figure and not a bound derived from the format.
FP32_ERR_MEASURED = 1.2e-06
FP32_ERR_GATE = 4 * FP32_ERR_MEASURED


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    d = tmp_path_factory.mktemp("notch")
    return dict(fast=nf.build_check(d), san=nf.build_check(d, sanitize=True), dir=d)


def tone_in_noise(n, seed, tone=0.15, sigma=0.01, f=0.055):
    rng = np.random.default_rng(seed)
    x = sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) + tone * np.exp(2j * np.pi * f * np.arange(n))
    return x.astype(np.complex64)


# ---------------------------------------------------------------- a. the host build

def test_host_build_under_sanitizers_does_not_depend_on_the_cuts(check, tmp_path):
    """the same stream as one row, as rows of 896 and as ragged rows (0, 1 and D + L - 1 among them): y word for word; the state of a
    `rows` call carried into the next one continues the stream"""
    x = tone_in_noise(5000, 1)
    whole, _, s0 = nf.host_stream(check["san"], tmp_path, x, len(x))
    assert s0["rows"] == 1 and s0["finite"]
    for counts in (896, [0, 1, 23, 24, 25, 55, 56, 57, 0, 897, 3000, 862]):
        y, recs, s = nf.host_stream(check["san"], tmp_path, x, counts)
        assert (y.view(np.uint32) == whole.view(np.uint32)).all() and s["resets"] == 0
    assert sum([0, 1, 23, 24, 25, 55, 56, 57, 0, 897, 3000, 862]) == 5000 and len(recs) == 12 and recs[-1]["blocks"] == 12
    state, parts = None, []
    for a, b in ((0, 1), (1, 900), (900, 5000)):
        y, state, recs = nf.host_rows(check["san"], tmp_path, x[None, a:b], state=state)
        parts.append(y[0])
    assert (np.concatenate(parts).view(np.uint32) == whole.view(np.uint32)).all()
    # the state: the taps, then the last 55 inputs, newest first
    assert (state[0, 64:].view(np.complex64) == x[::-1][:nf.HIST]).all()
    # and what it is worth: the noise is 2e-4 of power beside a tone of 0.0225, so a cancelled tone leaves 0.9 % of the power; twice that
    # is allowed for what the moving taps add
    tail = slice(3000, 5000)
    assert np.mean(np.abs(whole[tail]) ** 2) < 0.02 * np.mean(np.abs(x[tail]) ** 2)


# ---------------------------------------------------------------- b. fp32 against float64

@pytest.mark.parametrize("rate", [7812.5, 9765.625])
def test_fp32_rule_against_float64_on_the_scenario_inputs(check, tmp_path, rate):
    cases, _ = nf.scenario(rate)
    for name, x in cases.items():
        y32, _, s = nf.host_stream(check["fast"], tmp_path, x, nf.BLOCK)
        y64, E64, resets = nf.model64(x, row=nf.BLOCK)
        rms = np.sqrt(np.mean(np.abs(x.astype(np.complex128)) ** 2))
        err = float(np.max(np.abs(y32.astype(np.complex128) - y64)) / rms)
        print("rate %g, %s: max |y32 - y64| / rms(x) = %.3e, sum |w|^2 = %.6f (fp32) %.6f (float64)" % (rate, name, err, s["tap_energy"], E64))
        assert err <= FP32_ERR_GATE, (rate, name, err)
        assert s["resets"] == resets == 0 and abs(s["tap_energy"] - E64) <= 1e-4 * max(E64, 1e-3)


# ---------------------------------------------------------------- c. the long run

@pytest.mark.parametrize("tone", [0.15, 0.0])
def test_ten_million_samples_leave_the_taps_where_they_belong(check, tmp_path, tone):
    """no leakage in the rule: sum |w|^2 stays at about 1 / L = 0.031 with a tone (measured: 0.03123 at the end, 0.03147 at most over
    the rows) and near zero without one (0.00093 / 0.00202), against a reset bound of 4; no reset, every output finite.  The issue's
    bound is the reset bound; the tighter one here -- 1.6 / L with a tone, a sixth of 1 / L without -- would show a drift long before."""
    x = tone_in_noise(10_000_000, 5, tone=tone)
    _, _, s = nf.host_stream(check["fast"], tmp_path, x, nf.BLOCK, want_y=False)
    print("tone %g: sum |w|^2 at the end %.6g, at most %.6g" % (tone, s["tap_energy"], s["max_tap_energy"]))
    assert s["finite"] and s["resets"] == 0 and s["rows"] == -(-10_000_000 // nf.BLOCK)
    assert s["max_tap_energy"] < (0.05 if tone else 0.005)


# ---------------------------------------------------------------- d. the guards

def test_zeros_change_nothing_and_come_out_as_zeros(check, tmp_path):
    x = tone_in_noise(600, 2)
    _, state, _ = nf.host_rows(check["san"], tmp_path, x[None, :])
    y, after, recs = nf.host_rows(check["san"], tmp_path, np.zeros((1, 100), np.complex64), state=state)
    # the delay line still holds the tone for D + L - 1 samples: the prediction is not zero there, the taps move; after that, nothing
    y2, after2, _ = nf.host_rows(check["san"], tmp_path, np.zeros((1, 100), np.complex64), state=after)
    assert (y2 == 0).all() and (after2[0, :64].view(np.uint32) == after[0, :64].view(np.uint32)).all() and (after2[0, 64:] == 0).all()
    assert (y[0, nf.HIST:] == 0).all()
    fresh, st, recs = nf.host_rows(check["san"], tmp_path, np.zeros((1, 100), np.complex64))
    assert (fresh == 0).all() and (st == 0).all() and recs[0]["resets"] == 0 and recs[0]["in_power"] == 0 and recs[0]["tap_energy"] == 0


def test_a_nan_sample_never_reaches_the_taps_and_is_gone_56_samples_later(check, tmp_path):
    x = tone_in_noise(3000, 3)
    bad = x.copy()
    bad[2000] = np.complex64(complex(float("nan"), 1.0))
    y, state, recs = nf.host_rows(check["san"], tmp_path, bad[None, :])
    good, _, _ = nf.host_rows(check["san"], tmp_path, x[None, :])
    assert np.isfinite(state[0, :64]).all() and recs[0]["resets"] == 0
    assert (y[0, :2000].view(np.uint32) == good[0, :2000].view(np.uint32)).all()
    assert np.isnan(y[0, 2000]) and np.isfinite(y[0, 2001:2000 + nf.D]).all()          # the sample itself; then the delay has not reached it
    assert np.isnan(y[0, 2000 + nf.D:2000 + nf.D + nf.L]).all()                         # in the delay line
    assert np.isfinite(y[0, 2000 + nf.HIST + 1:]).all()                                 # 56 samples later: normal again
    tail = slice(2500, 3000)
    assert np.mean(np.abs(y[0, tail]) ** 2) < 0.02 * np.mean(np.abs(x[tail]) ** 2)      # and the tone is still held down
    inf = x.copy()
    inf[2000] = np.complex64(complex(float("inf"), 0.0))
    y, state, _ = nf.host_rows(check["san"], tmp_path, inf[None, :])
    assert np.isfinite(state[0, :64]).all() and np.isfinite(y[0, 2000 + nf.HIST + 1:]).all()


def test_taps_beyond_the_bound_are_reset_and_counted(check, tmp_path):
    x = tone_in_noise(200, 4)
    for w0, resets in ((0.36, 1), (0.35, 0), (float("nan"), 1), (float("inf"), 1)):        # 32 taps of (w0, 0): sum |w|^2 = 4.15 / 3.92
        state = np.zeros((1, nf.STATE_FLOATS), np.float32)
        state[0, 0:64:2] = w0
        _, after, recs = nf.host_rows(check["san"], tmp_path, np.zeros((1, 10), np.complex64), state=state)
        assert recs[0]["resets"] == resets and recs[0]["blocks"] == 1
        assert (after[0, :64] == 0).all() == bool(resets)
    # a reset channel works on: the next row adapts from zero taps like a fresh channel with the same delay line
    state = np.zeros((1, nf.STATE_FLOATS), np.float32)
    state[0, 0:64:2] = 0.36
    _, after, _ = nf.host_rows(check["san"], tmp_path, np.zeros((1, 60), np.complex64), state=state)
    y, _, _ = nf.host_rows(check["san"], tmp_path, x[None, :], state=after)
    fresh, _, _ = nf.host_rows(check["san"], tmp_path, x[None, :])
    assert (y.view(np.uint32) == fresh.view(np.uint32)).all()


# ---------------------------------------------------------------- e. the decode scenario on the oracle

@pytest.mark.parametrize("rate", [7812.5, 9765.625])
def test_scenario_on_the_oracle_with_the_fp32_rule(oracle, check, tmp_path, rate):
    """six frames (modes 3, 0, 6, 5, 1, 7 at amplitude 0.05, cfo -11 Hz, noise 0.002), a carrier of 0.15 at 430
    Hz, a second of 0.10 at -900 Hz.  Clean: 6 of 6 off and on.  One tone, two tones: at most 1 of 6 off, 6 of 6 on."""
    cases, sent = nf.scenario(rate)
    assert len(sent) == 6
    for name, x in cases.items():
        off = nf.decoded(oracle, rate, x, sent)
        y, _, s = nf.host_stream(check["fast"], tmp_path, x, nf.BLOCK)
        on = nf.decoded(oracle, rate, y, sent)
        print("rate %g, %s: %d of 6 off, %d of 6 on" % (rate, name, off, on))
        assert s["resets"] == 0
        assert on == 6, (rate, name, on)
        assert off == 6 if name == "clean" else off <= 1, (rate, name, off)


def test_pipeline_scenario_amplitudes_on_the_oracle(oracle):
    """the wideband scenario of tests/test_gpu_notch.py at 250 ksps: noise 0.01, six frames of 0.006 on the middle channel, a carrier of
    0.02 (10.5 dB above them) 430 Hz above its carrier, one frame on each other channel.  The oracle decodes all six without the
    carrier and none with it (at most one is what is asked); the other channels' two either way."""
    s = nf.pipeline_scenario()
    mid = nf.FREQS[nf.MID]
    clean, tone = nf.oracle_pdus(oracle, s["clean"]), nf.oracle_pdus(oracle, s["tone"])
    assert nf.delivered([o for f, o in clean if f == mid], s["sent_mid"]) == 6 == len(s["sent_mid"])
    assert nf.delivered([o for f, o in tone if f == mid], s["sent_mid"]) <= 1
    for got in (clean, tone):
        assert all(any(f == sf and o[:len(so)] == so for f, o in got) for sf, so in s["sent_other"])


# ---------------------------------------------------------------- f. the interface

def test_exports_and_abi():
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c11", "-D_GNU_SOURCE", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + inc, os.path.join(ROOT, "tests", "abi", "hfdl_gpu_notch_abi.c")])
    assert C.sizeof(F.NotchStats) == 32 and F.NotchStats.last_in_power.offset == 16 and F.NotchStats.tap_energy.offset == 24
    assert F.NOTCH_STATE_FLOATS == nf.STATE_FLOATS == 174 and F.TAP_NOTCH_OUT == 10
    L = hf.load()
    for name in ("hfdl_gpu_frontend_notch_enable", "hfdl_gpu_frontend_notch_stats", "hfdl_gpu_notch_rows"):
        assert name in F.EXPORTS and hasattr(L, name)
    assert hf.notch_rows is F.notch_rows and hasattr(F.Frontend, "notch_enable") and hasattr(F.MultiFrontend, "notch_stats")
    src = open(os.path.join(HOST, "frontend.c")).read()
    assert "#pragma weak hfdl_gpu_frontend_notch_enable" in src and "#pragma weak hfdl_gpu_frontend_notch_stats" in src


@pytest.mark.parametrize("mu", [-0.002, 0.9e-5, 0.051, 1.0, float("nan"), float("inf"), 0.0, 0.002])
def test_a_null_handle_and_a_bad_step_are_refused_without_a_device(mu):
    L = hf.load()
    sel = np.zeros(2, np.int32)
    assert L.hfdl_gpu_frontend_notch_enable(None, None, 0, mu) == EINVAL
    assert L.hfdl_gpu_frontend_notch_enable(None, sel.ctypes.data_as(C.c_void_p), 2, mu) == EINVAL
    st = F.NotchStats()
    assert L.hfdl_gpu_frontend_notch_stats(None, 0, C.byref(st)) == EINVAL
    assert L.hfdl_gpu_frontend_notch_stats(None, 0, None) == EINVAL


def test_notch_rows_checks_every_argument_before_a_device():
    L = hf.load()
    x = np.zeros(16, np.float32)
    y = np.full(16, 7.0, np.float32)
    p, o = x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p)
    for args in ((None, 1, 8, 0.002, None, o), (p, 1, 8, 0.002, None, None), (p, 0, 8, 0.002, None, o), (p, 1, 0, 0.002, None, o), (p, -1, 8, 0.002, None, o),
                 (p, 1, 8, 0.0, None, o), (p, 1, 8, 0.06, None, o), (p, 1, 8, float("nan"), None, o), (p, 1 << 14, 1 << 14, 0.002, None, o)):
        assert L.hfdl_gpu_notch_rows(0, *args) == EINVAL, args
    assert (y == 7.0).all()


def test_host_setter_takes_0_and_1e5_to_005():
    H = C.CDLL(os.path.join(ROOT, "dumphfdl_amd", "libhfdl_host.so"))
    f = H.hfdl_frontend_set_notch
    f.argtypes = [C.c_float, C.c_void_p, C.c_int]
    khz = np.array([10010, 10020], np.int32)
    p = khz.ctypes.data_as(C.c_void_p)
    for mu, lst, n, want in ((0.002, None, 0, 0), (1e-5, p, 2, 0), (0.05, p, 1, 0), (0.051, None, 0, -1), (0.9e-5, None, 0, -1), (-1.0, None, 0, -1),
                             (float("nan"), None, 0, -1), (0.002, None, 2, -1), (0.002, p, -1, -1), (0.002, p, 4097, -1), (0.0, None, 0, 0)):
        assert f(mu, lst, n) == want, (mu, n)


def build_replay(tmp_path, standin):
    exe = str(tmp_path / ("replay_" + standin))
    subprocess.check_call(["gcc", "-g", "-O1", "-std=c11", "-D_GNU_SOURCE", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", HOST] +
                          [os.path.join(HOST, f) for f in ("hfdl_replay.c", "ring.c", "blocks.c", "input.c", "sink.c", "frontend.c")] +
                          [os.path.join(ROOT, "tests", "hostsim", standin + ".c"), "-o", exe, "-lpthread", "-lm"])
    return exe


def run_replay(exe, src, *options):
    cmd = [exe, "--iq-file", str(src), "--sample-rate", "250000", "--sample-format", "CS16", "--read-buffer-size", "4096", "--centerfreq", "10000"] + \
        list(options) + ["10010", "10020", "10030"]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=60)


@pytest.fixture()
def iq_file(tmp_path):
    src = tmp_path / "in.cs16"
    np.random.default_rng(5).integers(0, 256, (10 * 3072 + 100) * 4, dtype=np.uint8).tofile(src)
    return src


def test_replay_notch_is_refused_by_a_library_without_it(tmp_path, iq_file):
    """hfdl_replay --notch against the plain stand-in (tests/hostsim/gpu_standin.c has no canceller): the message, a non-zero status, no
    crash; a malformed option is refused by the option itself; without the option nothing has changed."""
    exe = build_replay(tmp_path, "gpu_standin")
    out = run_replay(exe, iq_file, "--notch", "0.002")
    assert out.returncode == 1 and "notch: this GPU library has no carrier canceller" in out.stderr, (out.returncode, out.stderr)
    for bad in ("0.5", "x", "0.002:", "0.002:10010,", "0.002;10010", "nan"):
        out = run_replay(exe, iq_file, "--notch", bad)
        assert out.returncode == 1 and "--notch wants MU[:KHZ,KHZ,...]" in out.stderr, (bad, out.stderr)
    out = run_replay(exe, iq_file)
    assert out.returncode == 0 and "notch" not in out.stderr


def test_replay_notch_passes_the_step_and_the_selection_through(tmp_path, iq_file):
    """... and against tests/hostsim/gpu_standin_notch.c, which has the entry points: the step and the selection arrive, frequencies as
    channel indices; a line per selected channel at the end and none for the others; a frequency that is no channel stops the run."""
    exe = build_replay(tmp_path, "gpu_standin_notch")
    out = run_replay(exe, iq_file, "--notch", "0.002:10030,10010")
    assert out.returncode == 0, out.stderr
    assert "STANDIN notch_enable mu=0.002 nsel=2 channels=2,0\n" in out.stderr
    lines = [ln for ln in out.stderr.split("\n") if ln.startswith("notch: ")]
    assert [ln.split()[1] for ln in lines] == ["10010000", "10030000"] and all("(mu 0.002)" in ln and "0 tap resets" in ln for ln in lines), lines
    out = run_replay(exe, iq_file, "--notch", "0.004")
    assert out.returncode == 0 and "STANDIN notch_enable mu=0.004 nsel=0 channels=\n" in out.stderr
    assert len([ln for ln in out.stderr.split("\n") if ln.startswith("notch: ")]) == 3
    out = run_replay(exe, iq_file, "--notch", "0.002:10050")
    assert "notch: 10050 kHz is not a channel of this front end" in out.stderr and "STANDIN notch_enable" not in out.stderr, out.stderr
    out = run_replay(exe, iq_file)
    assert out.returncode == 0 and "notch" not in out.stderr
