"""The CU partition rule and the demodulator's LDS budget, on the host (no GPU)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cu_partition_and_demodulator_lds(tmp_path):
    """planner.h plan_cu_partition for 128, 130, 256 and 512 channels: the two masks are disjoint and cover the 256 CUs, every XCD gives
    an equal share whether the mask counts XCD-major or XCD-interleaved, the demodulator's CUs hold every channel's workgroup, and there is
    no partition below 128 channels.  demod_lds.h DemodLds: the same total for launches of 1 000, 3 000 and 5 400 samples, within the 40 KiB
    budget (four workgroups per CU).  tests/hostsim/partition_lds_check.cpp."""
    exe = str(tmp_path / "partition_lds_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unused-function", "-I" + os.path.join(ROOT, "dumphfdl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "hostsim", "partition_lds_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
