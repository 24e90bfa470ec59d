"""Which stream a block's forward FFT runs on, and what orders it against its neighbours, on the host (no GPU)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fft_order_over_every_short_call_sequence(tmp_path):
    """planner.h FftOrder, the one place that decides for a pushed block on which stream its forward FFT runs, what that stream waits for
    first and what becomes of held-back demodulators: tests/hostsim/fft_order_check.cpp runs it inside a front end reduced to launches
    and waits over every sequence of up to eight calls out of {host push, device push, draining poll, channelize-only host / device
    block} (halves of 2, then 3 blocks closing by filling), for the three rules and both kinds of geometry.  No stream waits for an
    event no launch carries; every forward FFT follows the one before it, a set's first FFT the inverse FFT that read the set last,
    a fold its half's FFTs, a half's demodulators its inverse FFT and the demodulators of the half before; sequences of host pushes
    alone decide what they did before device blocks had a stream of their own."""
    exe = str(tmp_path / "fft_order_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unused-function", "-I" + os.path.join(ROOT, "dumphfdl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "hostsim", "fft_order_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    assert int(out.stdout.split()[0]) > 2_000_000
