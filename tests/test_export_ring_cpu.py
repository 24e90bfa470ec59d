"""The channel export's host bookkeeping (dumphfdl_amd/csrc/export_ring.h), as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer (no GPU)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_export_ring_bookkeeping(tmp_path):
    """An empty ring, R = 2, a half of 5 blocks into R = 4, the enable boundary, from_block before / inside / after the kept range, a
    finished prefix that ends inside a launch's successor.  tests/hostsim/export_ring_check.cpp."""
    exe = str(tmp_path / "export_ring_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "dumphfdl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "hostsim", "export_ring_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
