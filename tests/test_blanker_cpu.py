"""The wideband impulse-noise blanker, the parts that need no GPU (tests/blanker_f64.py is the model):

  a. every argument check of the three entry points answers HFDL_GPU_EINVAL without a device, and the ABI is pinned;
  b. Markov's bound holds on the model: at most 1 / k2 of a block can be blanked, whatever the block;
  c. the host build of blanker.h's sum (tests/hostsim/blanker_sum_check.cpp) agrees with float64 within 2 (d + 2) 2^-24, and its depth d
     is the Python mirror's;
  d. the decode scenario on the oracle: every frame of the clean stream, every frame of the model-blanked stream, at most half of the
     frames of the impulsive stream as it is;
  e. the host library: the setter's range, and hfdl_replay --blanker against a stand-in GPU library without the entry points."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import blanker_f64 as bf
import dumphfdl_amd as hf
from dumphfdl_amd import frontend as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dumphfdl_amd", "host")
EINVAL = -1
SIZES = (1, 63, 64, 65, 1023, 4096, 4097, 4113, 28672, 1048576 + 4097)      # 1048576 + 4097: 258 chunks, two partial sums for a thread of step 5


# ---------------------------------------------------------------- a. arguments, ABI

@pytest.mark.parametrize("db", [-1.0, 5.9, 60.1, float("nan"), float("inf"), 0.0])
def test_blank_block_refuses_a_threshold_outside_6_to_60_before_any_device_work(db):
    L = hf.load()
    x = np.zeros(16, np.float32)
    out = np.full(16, 7.0, np.float32)
    P, cnt = C.c_float(7.0), C.c_uint64(7)
    assert L.hfdl_gpu_blank_block(0, x.ctypes.data_as(C.c_void_p), 8, F.SFMT_CF32, db, out.ctypes.data_as(C.c_void_p), C.byref(P), C.byref(cnt)) == EINVAL
    assert (P.value, cnt.value) == (7.0, 7) and (out == 7.0).all()


def test_blank_block_checks_every_argument():
    L = hf.load()
    x = np.zeros(16, np.float32)
    out = np.zeros(16, np.float32)
    p, o = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    P, cnt = C.c_float(0), C.c_uint64(0)
    for args in ((None, 8, 0, 14.0, o, C.byref(P), C.byref(cnt)), (p, 8, 0, 14.0, None, C.byref(P), C.byref(cnt)), (p, 8, 0, 14.0, o, None, C.byref(cnt)),
                 (p, 8, 0, 14.0, o, C.byref(P), None), (p, 0, 0, 14.0, o, C.byref(P), C.byref(cnt)), (p, -4, 0, 14.0, o, C.byref(P), C.byref(cnt)),
                 (p, (1 << 24) + 1, 0, 14.0, o, C.byref(P), C.byref(cnt)), (p, 8, 3, 14.0, o, C.byref(P), C.byref(cnt)), (p, 8, -1, 14.0, o, C.byref(P), C.byref(cnt))):
        assert L.hfdl_gpu_blank_block(0, *args) == EINVAL, args


@pytest.mark.parametrize("db", [-1.0, 5.9, 60.1, float("nan"), 14.0, 0.0])
def test_a_null_handle_is_refused(db):
    L = hf.load()
    assert L.hfdl_gpu_frontend_blanker_enable(None, db) == EINVAL
    st = F.BlankerStats()
    assert L.hfdl_gpu_frontend_blanker_stats(None, 0, C.byref(st)) == EINVAL


def test_abi_is_pinned():
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c11", "-D_GNU_SOURCE", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + inc, os.path.join(ROOT, "tests", "abi", "hfdl_gpu_blanker_abi.c")])
    assert C.sizeof(F.BlankerStats) == 24 and F.BlankerStats.last_power.offset == 16
    for name in ("hfdl_gpu_frontend_blanker_enable", "hfdl_gpu_frontend_blanker_stats", "hfdl_gpu_blank_block"):
        assert name in F.EXPORTS
    src = open(os.path.join(HOST, "frontend.c")).read()
    assert "#pragma weak hfdl_gpu_frontend_blanker_enable" in src and "#pragma weak hfdl_gpu_frontend_blanker_stats" in src


# ---------------------------------------------------------------- b. Markov

@pytest.mark.parametrize("db", [6.0, 14.0, 30.0])
def test_markov_bound_holds_on_the_model(db):
    """whatever the block -- noise, a level jump, impulses of any share, one huge sample -- at most n / k2 samples exceed k2 times the mean"""
    rng = np.random.default_rng(8)
    n = 4113
    k2 = float(bf.k2_of(db))
    noise = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    blocks = [noise, np.where(np.arange(n) < n // 2, noise, 100 * noise).astype(np.complex64), np.ones(n, np.complex64)]
    for share in (0.001, 0.01, 1 / k2, 0.3):
        b = 0.01 * noise
        b[rng.random(n) < share] += 50
        blocks.append(b.astype(np.complex64))
    one = 0.01 * noise
    one[17] = 1e6
    blocks.append(one.astype(np.complex64))
    for x in blocks:
        mask, P, T, p = bf.model(x, db)
        assert mask.sum() <= n / k2, (db, int(mask.sum()))
        assert not mask.all()
    assert not bf.model(np.ones(n, np.complex64), db)[0].any()          # a constant level: nothing is above k2 times itself


# ---------------------------------------------------------------- c. the documented order, built for the host

@pytest.fixture(scope="module")
def sum_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("blank") / "blanker_sum_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "dumphfdl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "hostsim", "blanker_sum_check.cpp"), "-o", exe])
    return exe


def test_host_build_of_the_sum_agrees_with_float64(sum_check, tmp_path):
    rng = np.random.default_rng(3)
    n = max(SIZES)
    x = (0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    x[rng.integers(0, n, 200)] += np.complex64(0.9)
    path = tmp_path / "x.cf32"
    x.tofile(path)
    out = subprocess.run([sum_check, str(path)] + [str(k) for k in SIZES], capture_output=True, text=True, check=True).stdout.split("\n")
    for k, line in zip(SIZES, out):
        nn, depth, bits, _, kbits = line.split()
        P = float(np.array([int(bits, 16)], np.uint32).view(np.float32)[0])
        P64 = float(np.mean(bf.power64(x[:k])))
        assert (int(nn), int(depth)) == (k, F.blank_sum_depth(k))
        assert abs(P - P64) / P64 <= bf.power_bound(int(depth)), (k, P, P64)
        assert int(kbits, 16) == int(np.array([bf.k2_of(14.0)]).view(np.uint32)[0])
    assert F.blank_sum_depth(1) == 26 and F.blank_sum_depth(7340032) == 32 and F.blank_sum_depth(1 << 24) == 41


# ---------------------------------------------------------------- d. the decode scenario on the oracle

def test_scenario_on_the_oracle(oracle):
    """six weak frames on three channels, 300 impulses a second of 8 samples at amplitude 0.9.  Clean: all
    decoded.  Impulsive: at most half.  Impulsive, blanked by the model at 14 dB: all decoded; the rule zeroes nothing of the clean
    stream and at least 99 % of the impulse samples."""
    s = bf.scenario()
    sent = s["sent"]
    n = oracle.geometry(bf.FS)[2].input_size
    assert bf.delivered(bf.oracle_pdus(oracle, s["clean"]), sent) == len(sent) == 6
    assert bf.delivered(bf.oracle_pdus(oracle, s["impulsive"]), sent) <= len(sent) // 2
    blanked, counts, _ = bf.blank_stream(s["impulsive"], n, bf.THRESHOLD_DB)
    assert bf.delivered(bf.oracle_pdus(oracle, blanked), sent) == len(sent)
    whole = (len(blanked) // n) * n
    hit = s["hit"][:whole]
    assert ((blanked[:whole] == 0) & hit).sum() >= 0.99 * hit.sum() and sum(counts) <= hit.sum()
    assert sum(bf.blank_stream(s["clean"], n, bf.THRESHOLD_DB)[1]) == 0


# ---------------------------------------------------------------- e. the host library

def test_host_setter_takes_0_and_6_to_60():
    H = C.CDLL(os.path.join(ROOT, "dumphfdl_amd", "libhfdl_host.so"))
    f = H.hfdl_frontend_set_blanker
    f.argtypes = [C.c_float]
    for db, want in ((14.0, 0), (6.0, 0), (60.0, 0), (5.9, -1), (60.1, -1), (-1.0, -1), (float("nan"), -1), (0.0, 0)):
        assert f(db) == want, db


def test_replay_blanker_is_refused_by_a_library_without_it(tmp_path):
    """hfdl_replay --blanker against the plain stand-in (tests/hostsim/gpu_standin.c has no blanker): the message, a non-zero status, no
    crash; a threshold out of range is refused by the option itself; without the option nothing has changed."""
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
    out = run("--blanker", "14")
    assert out.returncode == 1 and "blanker: this GPU library has no impulse-noise blanker" in out.stderr, (out.returncode, out.stderr)
    out = run("--blanker", "3")
    assert out.returncode == 1 and "--blanker wants a threshold of 6 to 60 dB" in out.stderr
    out = run()
    assert out.returncode == 0 and "blanker" not in out.stderr
