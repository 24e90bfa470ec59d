"""CPU tests of the spectrum monitor's history of interval rows: the argument checks of the three entry points that need no device
(they run before any device work, as everywhere in include/hfdl_gpu.h) and the public header's declarations."""
import ctypes as C
import os
import re

from dumphfdl_amd import frontend as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
NAMES = ("hfdl_gpu_frontend_spectrum_history", "hfdl_gpu_frontend_spectrum_row_close", "hfdl_gpu_frontend_spectrum_rows")


def test_history_entry_points_check_arguments_without_a_device():
    L = F.load()
    err = L.hfdl_gpu_last_error
    # rows and interval_blocks are judged before the handle is looked at: the text says which argument it was
    for rows in (1, -1, F.SPECTRUM_ROWS_MAX + 1):
        assert L.hfdl_gpu_frontend_spectrum_history(None, rows, 0) == EINVAL
        assert b"rows %d" % rows in err(), err()
    assert L.hfdl_gpu_frontend_spectrum_history(None, 8, -1) == EINVAL
    assert b"interval" in err()
    for rows in (0, 2, F.SPECTRUM_ROWS_MAX):
        assert L.hfdl_gpu_frontend_spectrum_history(None, rows, 4) == EINVAL
        assert b"null" in err()
    row = C.c_uint64(0)
    assert L.hfdl_gpu_frontend_spectrum_row_close(None, C.byref(row)) == EINVAL
    assert b"null" in err()
    mean = (C.c_float * 16)()
    info, n, nxt = F.SpectrumRow(), C.c_int32(7), C.c_uint64(7)
    assert L.hfdl_gpu_frontend_spectrum_rows(None, 0, 0, 1, mean, None, C.byref(info), C.byref(n), C.byref(nxt), 0) == EINVAL
    assert b"null" in err()
    # null n / next_row: refused before anything is written (a handle that is not looked at either: the null checks come first)
    bogus = C.c_void_p(8)
    assert L.hfdl_gpu_frontend_spectrum_rows(bogus, 0, 0, 1, mean, None, C.byref(info), None, C.byref(nxt), 0) == EINVAL
    assert b"null" in err()
    assert L.hfdl_gpu_frontend_spectrum_rows(bogus, 0, 0, 1, mean, None, C.byref(info), C.byref(n), None, 1) == EINVAL
    assert b"null" in err()
    assert L.hfdl_gpu_frontend_spectrum_row_close(bogus, None) == EINVAL
    assert (n.value, nxt.value) == (7, 7)


def test_header_declares_the_history():
    hdr = open(os.path.join(ROOT, "include", "hfdl_gpu.h")).read()
    declared = set(re.findall(r"\b(hfdl_gpu_[a-z0-9_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared and name in F.EXPORTS
    assert re.search(r"#define\s+HFDL_GPU_SPECTRUM_ROWS_MAX\s+1024\b", hdr) and F.SPECTRUM_ROWS_MAX == 1024
    m = re.search(r"typedef struct \{([^}]*)\}\s*hfdl_gpu_spectrum_row;", hdr)
    fields = re.findall(r"\b(uint64_t|uint32_t)\s+(\w+);", m.group(1))
    assert fields == [("uint64_t", "row"), ("uint64_t", "first_block"), ("uint32_t", "blocks"), ("uint32_t", "pad")]
    assert [(n, C.sizeof(t)) for n, t in F.SpectrumRow._fields_] == [("row", 8), ("first_block", 8), ("blocks", 4), ("pad", 4)] and C.sizeof(F.SpectrumRow) == 24
