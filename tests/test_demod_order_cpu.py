"""What orders a closed half's demodulator launches, burst decoders and the polls that read their snapshots, on the host (no GPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def order_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("demod_order") / "demod_order_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unused-function", "-I" + os.path.join(ROOT, "dumphfdl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "hostsim", "demod_order_check.cpp"), "-o", exe])
    return exe


def test_demod_order_over_every_short_call_sequence(order_exe):
    """planner.h DemodOrder, the one place that says which frame queue, frame counter, wait and done event a demodulator launch gets and
    which snapshot slot a poll reads: tests/hostsim/demod_order_check.cpp runs it inside a front end reduced to launches and waits
    (streams A, B and D, D also as an alias of B; halves of 2, then 3 blocks; 1, 2 and 3 blocks per launch; fold-bound and not) over every
    sequence of up to six calls out of {push, sync, poll_pdus_ready 1 / 2, push_baseband, channelize-only block, retune}.  A
    demodulator follows every kernel that used its frame queue or counter before -- the decoder of two launches ago above all, the
    premise of frame_slots_check.cpp; a decoder follows its demodulator; an inverse FFT into a half follows the half's last demodulator;
    no poll reads a snapshot slot that a queued, unfinished decoder can still write; nothing waits for an event no launch carried."""
    out = subprocess.run([order_exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    assert int(out.stdout.split()[0]) > 1_000_000


@pytest.mark.parametrize("fault", ["drop-b", "drop-a", "drop-d", "drop-ifft", "wrong-slot"])
def test_a_dropped_wait_or_the_wrong_slot_is_caught(order_exe, fault):
    """The same sequences with one wait left out -- stream B's for the decoder of two launches ago, stream A's for the same, stream D's
    for the demodulator, the inverse FFT's for the half's last demodulator -- or with the poll reading the other snapshot slot: each
    must show a violation."""
    out = subprocess.run([order_exe, fault], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("violated"), out.stdout + out.stderr
