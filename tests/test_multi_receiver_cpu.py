"""A front end of several receivers (hfdl_gpu_frontend_create_multi) without a device: every argument check runs before a device is
selected, and the padded tap layout of the receivers' channels is a bijection that never puts two receivers in one octet."""
import ctypes as C
import os
import subprocess

import numpy as np

from dumphfdl_amd import frontend as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def _create(L, fs, centres, freqs, counts, nrx=None):
    h = C.c_void_p()
    c = np.ascontiguousarray(centres, np.int32)
    f = np.ascontiguousarray(freqs, np.int32)
    n = np.ascontiguousarray(counts, np.int32)
    nrx = len(counts) if nrx is None else nrx
    rc = L.hfdl_gpu_frontend_create_multi(C.byref(h), 0, fs, nrx, c.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p),
                                          n.ctypes.data_as(C.c_void_p))
    return rc, h


def test_create_multi_rejects_bad_arguments_without_a_device():
    """Null pointers, nrx = 0 / 65, a zero channel count, a channel inside ANOTHER receiver's band but outside its own, a sample rate
    below 5400: HFDL_GPU_EINVAL with a per-thread text, before any device is touched (the device index 0 is never looked at)."""
    L = F.load()
    fs = 2_048_000
    good_c, good_f, good_n = [10_000_000, 12_000_000], [10_100_000, 12_100_000, 11_900_000], [1, 2]
    h = C.c_void_p()
    arr = np.zeros(4, np.int32).ctypes.data_as(C.c_void_p)
    assert L.hfdl_gpu_frontend_create_multi(None, 0, fs, 1, arr, arr, arr) == EINVAL
    assert L.hfdl_gpu_frontend_create_multi(C.byref(h), 0, fs, 1, None, arr, arr) == EINVAL
    assert L.hfdl_gpu_frontend_create_multi(C.byref(h), 0, fs, 1, arr, None, arr) == EINVAL
    assert L.hfdl_gpu_frontend_create_multi(C.byref(h), 0, fs, 1, arr, arr, None) == EINVAL
    assert b"null" in L.hfdl_gpu_last_error()
    rc, h = _create(L, fs, [10_000_000], [10_000_000], [1], nrx=0)
    assert rc == EINVAL and b"receivers" in L.hfdl_gpu_last_error() and not h.value
    rc, h = _create(L, fs, [10_000_000] * 65, [10_000_000] * 65, [1] * 65)
    assert rc == EINVAL and b"65 receivers" in L.hfdl_gpu_last_error()
    rc, h = _create(L, fs, good_c, good_f[:2], [2, 0])
    assert rc == EINVAL and b"receiver 1 has 0 channels" in L.hfdl_gpu_last_error()
    # receiver 1's second channel lies 100 kHz from receiver 0's centre, 2.1 MHz from its own: outside +-fs/2 of ITS receiver
    rc, h = _create(L, fs, good_c, [10_100_000, 12_100_000, 10_100_000], good_n)
    assert rc == EINVAL and b"receiver 1" in L.hfdl_gpu_last_error() and b"channel 2" in L.hfdl_gpu_last_error()
    rc, h = _create(L, 5399, good_c, good_f, good_n)
    assert rc == EINVAL and b"5400" in L.hfdl_gpu_last_error()
    # the text is per calling thread
    import threading
    seen = []
    t = threading.Thread(target=lambda: seen.append(L.hfdl_gpu_last_error()))
    t.start()
    t.join()
    assert seen[0] != L.hfdl_gpu_last_error()


def test_multi_receiver_entry_points_reject_null_without_a_device():
    L = F.load()
    buf = (C.c_void_p * 1)()
    assert L.hfdl_gpu_frontend_push_blocks_raw(None, buf, 0, 0, 0) == EINVAL
    assert L.hfdl_gpu_frontend_push_blocks_raw(None, None, 0, 0, 0) == EINVAL
    rx, cf = C.c_int32(0), C.c_int32(0)
    assert L.hfdl_gpu_frontend_channel_receiver(None, 0, C.byref(rx), C.byref(cf)) == EINVAL
    assert b"null" in L.hfdl_gpu_last_error()


def test_multi_receiver_symbols_are_exported():
    for name in ("hfdl_gpu_frontend_create_multi", "hfdl_gpu_frontend_push_blocks_raw", "hfdl_gpu_frontend_channel_receiver"):
        assert name in F.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "hfdl_gpu.h")).read()
    assert "#define HFDL_GPU_RECEIVERS_MAX 64" in hdr and F.RECEIVERS_MAX == 64


def test_padded_receiver_layout_is_a_bijection(tmp_path):
    """planner.h plan_receiver_slots / fold_group_tables on the host (tests/hostsim/rx_layout_check.cpp): each receiver's channels take
    consecutive slots of a run padded to whole tap-layout groups (octets, or single slots for the plain layout), no group holds two
    receivers, and for every workgroup width each octet goes to exactly one fold workgroup inside its own receiver."""
    exe = str(tmp_path / "rx_layout_check")
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "dumphfdl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "hostsim", "rx_layout_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


def test_batch_plan_and_row_windows_follow_the_documented_rules(tmp_path):
    """planner.h plan_batches / fold_row_windows on the host (tests/hostsim/batch_plan_check.cpp): the slices, fold and demodulator
    batches, halves and staging buffers DESIGN.md documents for cfg1 .. cfg3, the multi-receiver memory cap, explicit HFDL_GPU_DEMOD_BATCH /
    HFDL_GPU_FOLD_BATCH; and the pruned fold's row windows: a single peak, a peak wrapping row p - 1 -> 0, an all-padding octet = (0, 2),
    counts even and at most p / 4, a smaller tolerance never folds fewer rows."""
    exe = str(tmp_path / "batch_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "dumphfdl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "hostsim", "batch_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
