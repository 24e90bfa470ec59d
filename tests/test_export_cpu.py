"""CPU tests of the channel baseband export: the argument checks of both entry points that need no front end (they run before any
device work, as everywhere in include/hfdl_gpu.h), the public headers' declarations, and the numpy definition's own corner cases."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import export_f64 as E
from dumphfdl_amd import frontend as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
NAMES = ("hfdl_gpu_frontend_export_enable", "hfdl_gpu_frontend_export_read")


def test_export_entry_points_check_arguments_without_a_device():
    L = F.load()
    err = L.hfdl_gpu_last_error
    ch = (C.c_int32 * 2)(1, 0)
    for nsel, fmt, scale, ring in ((2, F.EXPORT_CF32, 1.0, 64), (0, F.EXPORT_CF32, 1.0, 64), (-1, 7, -1.0, 1)):
        assert L.hfdl_gpu_frontend_export_enable(None, ch, nsel, fmt, scale, ring) == EINVAL
        assert b"null" in err(), err()
    assert L.hfdl_gpu_frontend_export_enable(None, None, 2, F.EXPORT_CS16, 100.0, 8) == EINVAL
    samples, counts, info = (C.c_float * 16)(), (C.c_int32 * 2)(), (C.c_uint64 * 1)()
    n, nxt = C.c_int32(7), C.c_uint64(7)
    for wait in (0, 1):
        assert L.hfdl_gpu_frontend_export_read(None, 0, 1, samples, counts, None, None, info, C.byref(n), C.byref(nxt), wait) == EINVAL
        assert b"null" in err(), err()
    # null n / next_block: refused before the handle is looked at and before anything is written
    bogus = C.c_void_p(8)
    assert L.hfdl_gpu_frontend_export_read(bogus, 0, 1, samples, counts, None, None, info, None, C.byref(nxt), 0) == EINVAL
    assert b"null" in err()
    assert L.hfdl_gpu_frontend_export_read(bogus, 0, 1, samples, counts, None, None, info, C.byref(n), None, 1) == EINVAL
    assert b"null" in err()
    assert (n.value, nxt.value) == (7, 7)


def test_headers_declare_the_export():
    hdr = open(os.path.join(ROOT, "include", "hfdl_gpu.h")).read()
    declared = set(re.findall(r"\b(hfdl_gpu_[a-z0-9_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared and name in F.EXPORTS
    assert re.search(r"#define\s+HFDL_GPU_EXPORT_CF32\s+0\b", hdr) and F.EXPORT_CF32 == 0
    assert re.search(r"#define\s+HFDL_GPU_EXPORT_CS16\s+1\b", hdr) and F.EXPORT_CS16 == 1
    assert re.search(r"#define\s+HFDL_GPU_EXPORT_RING_MAX\s+4096\b", hdr) and F.EXPORT_RING_MAX == 4096
    assert re.search(r"typedef struct \{\s*uint64_t block;\s*\}\s*hfdl_gpu_export_block;", hdr)
    host = open(os.path.join(ROOT, "include", "hfdl_host.h")).read()
    assert re.search(r"\bint\s+hfdl_frontend_set_iq_export\s*\(\s*const char \*dir,\s*const int32_t \*freqs,\s*int32_t nfreqs,\s*int format,\s*float scale\s*\)\s*;", host)


def test_host_prototype_is_pinned():
    """tests/abi/hfdl_host_export_abi.c: the host library's new prototype, by type, in C11 with every warning an error; and the host
    library refuses bad arguments without a device."""
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c11", "-D_GNU_SOURCE", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + inc, os.path.join(ROOT, "tests", "abi", "hfdl_host_export_abi.c")])
    H = C.CDLL(os.path.join(ROOT, "dumphfdl_amd", "libhfdl_host.so"))
    f = H.hfdl_frontend_set_iq_export
    f.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.c_int32, C.c_int, C.c_float]
    fr = (C.c_int32 * 2)(10_000_000, 10_040_000)
    assert f(b"/tmp", fr, 2, 0, 0.0) == 0 and f(b"/tmp", None, 0, 1, 100.0) == 0
    for args in ((b"/tmp", fr, -1, 0, 1.0), (b"/tmp", None, 2, 0, 1.0), (b"/tmp", fr, 2, 2, 1.0), (b"/tmp", fr, 2, 1, 0.0), (b"/tmp", fr, 2, 1, float("inf")),
                 (b"/tmp", fr, 2, 1, float("nan"))):
        assert f(*args) == -1, args
    assert f(None, None, 0, 0, 0.0) == 0


def test_definition_corner_cases():
    """The numpy definition itself (tests/export_f64.py), not the library: it guards the reference the GPU tests compare with, and
    passes with or without the feature.  Half-way cases round to even, +-32767 is the last value not clipped, NaN stores 0 and counts, and
    the power's order is the plain sum where every partial sum is exact."""
    x = np.array([0.5 + 1.5j, 2.5 - 0.5j, 32767.4 - 32767.4j, 32767.5 - 32767.5j, complex(np.nan, 1.0), complex(np.inf, -np.inf)], np.complex64)
    q, clipped = E.cs16(x[None, :], 1.0)
    assert q[0].tolist() == [[0, 2], [2, 0], [32767, -32767], [32767, -32767], [0, 1], [32767, -32767]] and clipped.tolist() == [5]
    q, clipped = E.cs16(x[None, :2], 2.0)
    assert q[0].tolist() == [[1, 3], [5, -1]] and clipped.tolist() == [0]
    for n in (0, 1, 255, 256, 257, 1171):
        v = (np.arange(n) % 7 + 1j * (np.arange(n) % 3)).astype(np.complex64)           # small integers: every fp32 sum is exact
        want = np.float32(np.float32(np.sum(np.abs(v.astype(np.complex128)) ** 2)) / np.float32(n)) if n else np.float32(0)
        assert E.power_f32(v).view(np.uint32) == want.view(np.uint32), n
    rng = np.random.default_rng(3)
    v = (rng.standard_normal(1171) + 1j * rng.standard_normal(1171)).astype(np.complex64)
    assert abs(float(E.power_f32(v)) - E.power_f64(v)) <= E.power_gate(1171) * E.power_f64(v)
