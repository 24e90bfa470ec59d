#!/usr/bin/env python3
"""What the channel baseband export costs: in ONE process, arms alternating, input resident in HBM,
  off:  the front end as it is (its spread over the repetitions is the margin);
  b16:  16 channels CF32 (spread over the channel list), export_read(wait=False) after EVERY push;
  all:  every channel CS16 (scale 32767), collected every 32 pushes with export_read(wait=False);
each arm's rest collected with wait=True behind the draining poll, inside the timed span (the pushes are not throttled and run far ahead
of the device, so the ring holds the whole run, RING = 512 blocks: with 128 the blocks were overwritten before their launch had run), for (1) cfg3 (40 Msps x 256 channels, 256
steps) and (2) eight cfg2 receivers in one MultiFrontend.  REPS repetitions of each arm: Msamples/s of the timed steps (bench.py's
`value` arithmetic: steps x input_size x receivers / wall time including the draining poll).  One JSON line per workload.
  python profiles/channel_export.py [cfg3|multi] ... [steps=N] [reps=N]     (default: both workloads, 256 steps, 3 repetitions)
The kernel's own time comes from a separate run under `rocprofv3 --kernel-trace --stats -- python profiles/channel_export.py cfg3`
(the export's events carry no timing: DESIGN.md section 4.10)."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
import dumphfdl_amd as hf

STEPS, WARM, REPS, EVERY, RING = 256, 8, 3, 32, 512
ARMS = ("off", "b16", "all")


def run(fe, push_step, nrx, nblocks, first, arm):
    nch = fe.geometry.channels
    if arm == "b16":
        fe.export_enable(list(range(0, nch, max(1, nch // 16)))[:16], fmt="cf32", ring_blocks=RING)
    elif arm == "all":
        fe.export_enable(list(range(nch)), fmt="cs16", scale=32767.0, ring_blocks=RING)
    else:
        fe.export_enable([])
    for i in range(WARM):
        push_step((first + i) % nblocks)
    fe.poll_pdus(16384 * nrx)
    torch.cuda.synchronize()
    # the warm-up blocks stay in the ring uncollected: the timed span starts at the block count, so it collects the timed blocks alone
    start, got_blocks, lost = fe.counters()["blocks"], 0, 0
    nxt = start
    t0 = time.perf_counter()
    for i in range(STEPS):
        push_step((first + WARM + i) % nblocks)
        if arm == "b16" or (arm == "all" and i % EVERY == EVERY - 1):
            while True:
                got = fe.export_read(nxt, max_blocks=8, wait=False)
                lost += got[5] - nxt - len(got[4])            # next_block moves past blocks the ring has overwritten, returned or not
                got_blocks += len(got[4])
                nxt = got[5]
                if len(got[4]) < 8:
                    break
    pd = len(fe.poll_pdus(16384 * nrx))
    while arm != "off":
        got = fe.export_read(nxt, max_blocks=8, wait=True)
        lost += got[5] - nxt - len(got[4])
        got_blocks += len(got[4])
        nxt = got[5]
        if len(got[4]) < 8:
            break
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    if arm != "off":
        assert nxt == start + STEPS and got_blocks + lost == STEPS, (nxt, start, got_blocks, lost)     # every timed block collected, or counted as lost
    return el, pd, got_blocks, lost


def measure(name, fe, push_step, nrx, nblocks, n):
    fe.enable_taps(False)
    rates, pdus, blocks, lost = ({a: [] for a in ARMS} for _ in range(4))
    for rep in range(REPS):
        for arm in ARMS:
            el, pd, gb, ls = run(fe, push_step, nrx, nblocks, rep * STEPS, arm)
            rates[arm].append(round(nrx * STEPS * n / el / 1e6, 1))
            pdus[arm].append(pd)
            blocks[arm].append(gb)
            lost[arm].append(ls)
    fe.export_enable([])
    off = rates["off"]
    g = fe.geometry
    print(json.dumps(dict(workload=name, receivers=nrx, channels=g.channels, row_samples=g.max_outputs_per_block, steps=STEPS, reps=REPS, ring_blocks=RING,
                          off_Msamples_s=off, b16_Msamples_s=rates["b16"], all_Msamples_s=rates["all"],
                          off_spread_pct=round(100 * (max(off) - min(off)) / np.mean(off), 2),
                          b16_over_off=round(float(np.mean(rates["b16"]) / np.mean(off)), 4), all_over_off=round(float(np.mean(rates["all"]) / np.mean(off)), 4),
                          blocks_collected=blocks, blocks_lost=lost, pdus=pdus)), flush=True)


for a in sys.argv[1:]:
    if a.startswith("steps="):
        STEPS = int(a[6:])
    if a.startswith("reps="):
        REPS = int(a[5:])
which = [a for a in sys.argv[1:] if "=" not in a] or ["cfg3", "multi"]
if "cfg3" in which:
    w = bench.WORKLOADS["cfg3"]
    freqs = bench.channel_plan(w)
    fe = hf.Frontend(w["fs"], w["centerfreq"], freqs, device=0)
    n = fe.input_size
    x = bench.make_input(w, n, 0, 1)[0]
    nblocks = len(x) // n
    dev = torch.from_numpy(np.array(x).view(np.float32)).cuda()
    torch.cuda.synchronize()
    measure("cfg3", fe, lambda b: fe.push_block(dev.data_ptr() + 8 * b * n), 1, nblocks, n)
    fe.close()
    del dev
if "multi" in which:
    K, W = 8, bench.WORKLOADS["cfg2"]
    ws = [dict(W, seed=100 + r, centerfreq=W["centerfreq"] + 3_000_000 * (r - K // 2)) for r in range(K)]
    fr = [bench.channel_plan(w) for w in ws]
    fe = hf.MultiFrontend(W["fs"], [(w["centerfreq"], f) for w, f in zip(ws, fr)], device=0)
    n = fe.input_size
    xs = [bench.make_input(w, n, 0, 1)[0] for w in ws]
    nblocks = min(len(x) for x in xs) // n
    devs = [torch.from_numpy(np.array(x).view(np.float32)).cuda() for x in xs]
    torch.cuda.synchronize()
    measure("8 x cfg2", fe, lambda b: fe.push_blocks([d.data_ptr() + 8 * b * n for d in devs]), K, nblocks, n)
    fe.close()
