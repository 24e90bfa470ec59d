#!/usr/bin/env python3
"""What the frame quality records cost: in ONE process, arms alternating, input resident in HBM,
  off:  the front end as it is (its spread over the repetitions is the margin);
  rec:  quality_enable(4096), quality_read(wait=False) after EVERY push;
  sym:  the same with the frames' data symbols kept and read too;
each arm's rest collected behind the draining poll, inside the timed span, for cfg3 (40 Msps x 256 channels) and cfg4 (the burst-dense
one, which exercises it).  REPS repetitions of each arm: Msamples/s of the timed steps (bench.py's `value` arithmetic: steps x
input_size / wall time including the draining poll).  One JSON line per workload.
  python profiles/frame_quality.py [cfg3|cfg4] ... [steps=N] [reps=N] [dicts]    (default: both workloads, 256 steps, 3 repetitions;
                                                                                 dicts: read through quality_read(), a dict per record)
  python profiles/frame_quality.py kernel                                  (the kernel alone: the stage entry on 256 double-slot frames)
The kernel's time per frame: `kernel` prints hfdl_gpu_last_stage_ms() / frames of the stage entry (events around the one launch)."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
import dumphfdl_amd as hf
from dumphfdl_amd import frontend as F

STEPS, WARM, REPS = 256, 8, 3
RAW = True          # reads fill the caller's buffers (quality_read_raw); `dicts`: through quality_read(), which allocates and makes a dict per record
ARMS = ("off", "rec", "sym")


def run(fe, push_step, nblocks, first, arm):
    fe.quality_enable(0 if arm == "off" else 4096, symbols=arm == "sym")
    for i in range(WARM):
        push_step((first + i) % nblocks)
    fe.poll_pdus(16384)
    if arm != "off":
        fe.quality_read(wait=False)
    torch.cuda.synchronize()
    frames, dropped = 0, 0
    out = fe.quality_read_raw(max_frames=64)[:2] if arm != "off" and RAW else None        # the caller's buffers, filled again by every read
    t0 = time.perf_counter()
    for i in range(STEPS):
        push_step((first + WARM + i) % nblocks)
        if arm != "off":
            if RAW:
                got, dropped = fe.quality_read_raw(max_frames=64, wait=False, out=out)[2:]
            else:
                recs, _, dropped = fe.quality_read(max_frames=64, wait=False)
                got = len(recs)
            frames += got
    pd = len(fe.poll_pdus(16384))
    while arm != "off":
        got, dropped = fe.quality_read_raw(max_frames=64, wait=False, out=out)[2:] if RAW else (lambda r: (len(r[0]), r[2]))(fe.quality_read(max_frames=64, wait=False))
        frames += got
        if got < 64:
            break
    torch.cuda.synchronize()
    return time.perf_counter() - t0, pd, frames, dropped


def measure(name):
    w = bench.WORKLOADS[name]
    fe = hf.Frontend(w["fs"], w["centerfreq"], bench.channel_plan(w), device=0)
    fe.enable_taps(False)
    n = fe.input_size
    x = bench.make_input(w, n, 0, 1)[0]
    nblocks = len(x) // n
    dev = torch.from_numpy(np.array(x).view(np.float32)).cuda()
    torch.cuda.synchronize()
    push = lambda b: fe.push_block(dev.data_ptr() + 8 * b * n)
    rates, pdus, frames, dropped = ({a: [] for a in ARMS} for _ in range(4))
    for rep in range(REPS):
        for arm in ARMS:
            el, pd, fr, dr = run(fe, push, nblocks, rep * STEPS, arm)
            rates[arm].append(round(STEPS * n / el / 1e6, 1))
            pdus[arm].append(pd)
            frames[arm].append(fr)
            dropped[arm].append(dr)
    fe.quality_enable(0)
    off = rates["off"]
    print(json.dumps(dict(workload=name, reads="raw" if RAW else "dicts", channels=fe.geometry.channels, steps=STEPS, reps=REPS, ring_frames=4096,
                          off_Msamples_s=off, rec_Msamples_s=rates["rec"], sym_Msamples_s=rates["sym"],
                          off_spread_pct=round(100 * (max(off) - min(off)) / np.mean(off), 2),
                          rec_over_off=round(float(np.mean(rates["rec"]) / np.mean(off)), 4), sym_over_off=round(float(np.mean(rates["sym"]) / np.mean(off)), 4),
                          pdus=pdus, records=frames, dropped=dropped)), flush=True)
    fe.close()


def kernel():
    rng = np.random.default_rng(1)
    out = {}
    for mode, nframes in ((2, 256), (6, 256), (6, 1)):
        nsym = 5040 if mode & 4 else 2160
        sym = [np.exp(2j * np.pi * (rng.integers(0, 4, nsym) / 4 + rng.normal(0, 0.01, nsym))).astype(np.complex64) for _ in range(nframes)]
        best = 1e9
        for _ in range(5):
            F.frame_quality(sym, [mode] * nframes)
            best = min(best, F.last_stage_ms())
        out["mode %d x %d frames" % (mode, nframes)] = dict(launch_us=round(1e3 * best, 1), per_frame_us=round(1e3 * best / nframes, 2))
    print(json.dumps(dict(kernel="frame_quality_kernel, stage entry, best of 5", **out)), flush=True)


for a in sys.argv[1:]:
    if a.startswith("steps="):
        STEPS = int(a[6:])
    if a.startswith("reps="):
        REPS = int(a[5:])
RAW = "dicts" not in sys.argv[1:]
which = [a for a in sys.argv[1:] if "=" not in a and a != "dicts"] or ["cfg3", "cfg4"]
if "kernel" in which:
    kernel()
for name in ("cfg3", "cfg4"):
    if name in which:
        measure(name)
