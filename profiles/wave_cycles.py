#!/usr/bin/env python3
"""Cycles per 5400-sps sample of the demodulator's pipelined phase (P) and of each of its four waves, per framer state: the stage alone
(hfdl_gpu_frontend_push_baseband, taps on), one channel of the oracle's channelizer output at 250 ksps, one single-slot burst per stream
(modes 1, 2, 3), launches of 512 resampler outputs -- the inputs and launches of profiles/r11_experiments.md section 1.

The phase counters at the end of the level tap hold P, W1 (timing recovery) and W2 (carrier) in every build; the slot in front of them
holds wave 0's busy cycles (AGC + matched filter) in a -DHFDL_DM_PROBE=4 build and wave 3's (resampler + input fetch) in a
-DHFDL_DM_PROBE=5 build, and in a -DHFDL_DM_PROBE=6 build S: the sum over the pipeline's steps of the longest of waves 0, 1, 2 in that
step (demod_core.h, end of demod_block; P - S is the barrier and mailbox step itself, S - max(W) what the waves' per-chunk variation adds).  So every arm is two libraries, merged into one row P / W0 / W1 / W2 / W3 per
state:

    cd dumphfdl_amd/csrc
    HFDL_OUT=../../build_ab/libprobe4.so HFDL_BUILD_DIR=../../build_ab/p4 HFDL_EXTRA_FLAGS=-DHFDL_DM_PROBE=4 bash build.sh
    HFDL_OUT=../../build_ab/libprobe5.so HFDL_BUILD_DIR=../../build_ab/p5 HFDL_EXTRA_FLAGS=-DHFDL_DM_PROBE=5 bash build.sh
    python profiles/wave_cycles.py branch=build_ab/libprobe4.so,build_ab/libprobe5.so[,build_ab/libprobe6.so] [parent=...]

A launch is classed by the framer state before and after it and by the frame counter: "search" = FR_A1 throughout, "preamble T" = the
first two launches that begin and end in the equaliser's training after M2, "data" = every later launch inside the frame, "mixed" = a
launch that holds a transition.  Each library runs in a process of its own (HFDL_GPU_LIB)."""
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

FS, CF, FREQ = 250000, 10_000_000, 10_021_000
FR_A1, FR_EQ_TRAIN = 1, 5
LAUNCH = 512
COLS = ("P", "W0", "W1", "W2", "W3", "S")


def child():
    import hfdl_synth as synth
    import dumphfdl_amd as hf
    from dumphfdl_amd import frontend as F
    from oracle import pyoracle
    rows = []
    for mode in (1, 2, 3):
        rng = np.random.default_rng(300 + mode)
        b = dict(freq=FREQ, mode=mode, octets=synth.make_pdu(rng, mode), t0=1.1, amp=0.1, cfo=(-1) ** mode * (3.0 + mode))
        n = int((b["t0"] + synth.burst_symbols_len(mode) / 1800.0 + 0.3) * FS)
        x = synth.synth_wideband(FS, CF, n, [b], noise_sigma=0.004, seed=70 + mode)
        ora = pyoracle.Frontend(FS, CF, [FREQ])
        size, parts = ora.ddc.input_size, []
        for i in range(len(x) // size):
            ora.push_block(x[i * size:(i + 1) * size])
            parts.append(np.array(ora.channel_view(0)["chan_out"], np.complex64))
        ora.close()
        chan = np.concatenate(parts)
        fe = hf.Frontend(FS, CF, [FREQ])
        step = int(round(float(1 << 24) / float(fe.geometry.resamp_rate)))
        n_in = (LAUNCH * step) >> 24                         # about 512 outputs; the exact count is read back
        before, in_t = fe.channel_stats(0), 0
        for at in range(0, len(chan) - n_in + 1, n_in):
            fe.push_baseband([chan[at:at + n_in]])
            cyc = np.array(fe.read_tap(F.TAP_PHASE_CYCLES, 0), np.float64)
            n_out = len(fe.read_tap(F.TAP_AGC_LEVEL, 0))
            after = fe.channel_stats(0)
            s0, s1 = before["framer_state"], after["framer_state"]
            if s0 == s1 == FR_A1 and before["frames"] == after["frames"] and before["a2_found"] == after["a2_found"]:
                kind, in_t = "search", 0
            elif s0 >= FR_EQ_TRAIN and s1 >= FR_EQ_TRAIN and before["frames"] == after["frames"]:
                in_t += 1
                kind = "mode %d preamble T" % mode if in_t <= 2 else "mode %d data" % mode
            else:
                kind = "mixed"
            rows.append((kind, (cyc / n_out).tolist()))
            before = after
        fe.poll_pdus()
        fe.close()
    print(json.dumps(rows))


def main(arms):
    """arms: NAME=PROBE4_LIB,PROBE5_LIB[,PROBE6_LIB]"""
    table = {}
    names = []
    for arm in arms:
        name, libs = arm.split("=")
        names.append(name)
        for slot0, lib in zip(("W0", "W3", "S"), libs.split(",")):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=dict(os.environ, HFDL_GPU_LIB=os.path.abspath(lib)),
                               capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.exit("%s: exit %d\n%s" % (lib, r.returncode, r.stderr[-2000:]))
            for kind, c in json.loads(r.stdout.strip().splitlines()[-1]):
                t = table.setdefault(kind, {}).setdefault(name, {k: [] for k in COLS})
                t[slot0].append(c[0]); t["P"].append(c[1]); t["W1"].append(c[2]); t["W2"].append(c[3])
    print("cycles per 5400-sps sample, min - max over the launches of a class (P, W1, W2: over both builds of the arm)")
    print("| state (launches) | arm | P | W0 | W1 | W2 | W3 | S |\n|---|---|---|---|---|---|---|---|")
    for kind in sorted(table):
        for name in names:
            t = table[kind].get(name)
            if t:
                print("| %s (%d) | %s | %s |" % (kind, len(t["W0"]), name, " | ".join("%.0f - %.0f" % (min(t[k]), max(t[k])) if t[k] else "" for k in COLS)))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child()
    else:
        main(sys.argv[1:])
