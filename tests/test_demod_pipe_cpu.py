"""How far the demodulator's four stages may run apart, and that its LDS rings hold what can still be read, on the host (no GPU)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_demod_pipeline_rules_over_adversarial_schedules(tmp_path):
    """demod_lds.h resampler_advance / agc_advance / timing_advance / carrier_advance, the one place that decides how far a stage of the
    demodulator's pipeline goes in a step: tests/hostsim/demod_pipe_check.cpp steps a model of the four stages through the double-buffered
    mailbox, every stage seeing the progress as of the previous barrier, with what the rules leave open chosen against them -- 0 to 4
    timing-recovery outputs per input sample, a carrier stage that finishes any 1 to DM_CHUNK samples of its chunk (cut where more than
    64 outputs end) and reports a reset of the timing loop at any of them.  Corner schedules (always in step, every chunk cut to one
    sample, a reset at every sample in turn, a reset during the last sample) and 100 000 seeded random launches, of 0 to 5400 outputs.
    In every step no entry of a ring (resampler output, matched-filter output with its mirror, level, output counts, AGC output,
    channelizer input with its look-ahead fetch and history, timing-recovery outputs) is written while an entry with the same index
    modulo the ring's size can still be read, and some stage advances until the carrier stage has finished the launch."""
    exe = str(tmp_path / "demod_pipe_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unused-function", "-I" + os.path.join(ROOT, "dumphfdl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "hostsim", "demod_pipe_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    assert int(out.stdout.split()[0]) > 3_000_000           # the run checks 3 299 371 steps
