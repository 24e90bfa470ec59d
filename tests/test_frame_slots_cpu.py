"""Frame records and data slots of a demodulator launch that spans several frames, and the launch sizes that go with them, on the host (no GPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, name):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unused-function", "-I" + os.path.join(ROOT, "dumphfdl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "hostsim", name + ".cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def slots_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("frame_slots"), "frame_slots_check")


def test_no_slot_is_rewritten_before_its_frame_is_read(slots_exe):
    """planner.h plan_frame_slots: F = floor(T_L / T_F) + 1 records per channel and set, S = floor(2 T_L / T_F) + 2 data slots per channel.
    tests/hostsim/frame_slots_check.cpp steps frames that end at least T_F apart through launches cut anywhere up to T_L (one-block
    launches included), with the burst decoder of launch i done anywhere before the demodulator of launch i + 2 starts: no slot is
    written while its frame can still be read, no set holds more than F records of a channel."""
    out = subprocess.run([slots_exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    assert int(out.stdout.split()[0]) > 1_000_000


@pytest.mark.parametrize("fewer", ["S-1", "F-1"])
def test_one_slot_or_record_fewer_is_caught(slots_exe, fewer):
    """The same schedules with one data slot, or one frame record, fewer than the rule gives: every launch length must show a violation."""
    out = subprocess.run([slots_exe, fewer], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("violated"), out.stdout + out.stderr


def test_a_half_that_closes_full_is_one_launch(tmp_path):
    """planner.h plan_batches with the product's bound on a launch (the block table and the 16-bit output counts): cfg3 plans launches of 32
    blocks in halves of 32 (the first half after a drain 16), cfg2 8 in halves of 8; the multi-receiver cap and an override of 32."""
    out = subprocess.run([_build(tmp_path, "half_launch_plan_check")], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
