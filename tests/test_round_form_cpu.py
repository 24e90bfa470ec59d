"""The timing-recovery wave takes its filter-bank index as (int)(bf + copysignf(0x1.fffffep-2f, bf)) where the reference (liquid's
symsync_crcf, tests/hostsim/serial_demod.h) writes (int)roundf(bf): tests/hostsim/round_form_check.cpp compares the two forms pattern by
pattern with the device's float-to-int conversion spelled out (truncating, saturating, NaN -> 0).  Over all 2^32 patterns it takes some
seconds on sixteen cores (run once: profiles/r14_experiments.md); here it runs over the range the loop works in and over the edges."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("round_form") / "round_form_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread",
                           os.path.join(ROOT, "tests", "hostsim", "round_form_check.cpp"), "-o", exe])

    def run(lo, hi):
        out = subprocess.run([exe, "%x" % lo, "%x" % hi], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        assert out.stdout.split() == ["ok", str(2 * (hi - lo + 1))]
    return run


def test_binades_of_the_filter_bank_index(check):
    """16 tau lies in [-16, 48) in lock and within a few thousand of it at the worst: the binades 2^-3 .. 2^13, both signs, every pattern
    (2.85e8), among them every x.5 tie the two forms could part on."""
    check(0x3E000000, 0x467FFFFF)


@pytest.mark.parametrize("lo,hi", [
    (0x00000000, 0x00000001),      # +-0 and the smallest subnormals
    (0x007FFFFF, 0x00800000),      # the largest subnormals, the smallest normals
    (0x3EFFFFFF, 0x3F000001),      # around one half: the largest float below it is the constant that is added
    (0x4AFFFFFF, 0x4B800001),      # 2^23 .. 2^24: the sum is no longer exact, and every float is an integer
    (0x4EFFFFFF, 0x4F000001),      # around 2^31: the conversion saturates
    (0x7F7FFFFF, 0x7F800001),      # the largest finite values, +-inf, the first NaNs
    (0x7FBFFFFF, 0x7FC00001),      # signalling / quiet NaNs
    (0x7FFFFFFF, 0x7FFFFFFF),
])
def test_edges(check, lo, hi):
    check(lo, hi)
