#!/usr/bin/env python3
"""What the spectrum monitor costs: in ONE process, arms alternating, input resident in HBM,
  off: the front end as it is;   on: spectrum_enable(4096, HANN | MAXHOLD), a spectrum_read with reset of every receiver every 32 steps;
  noread: the monitor on and never read (the kernel's cost without the reads' waits);
  rows: the history of interval rows (spectrum_history(64)): spectrum_row_close() every 32 steps, spectrum_rows(wait=False) of every
        receiver after EVERY push, the rest collected with wait=True behind the draining poll (inside the timed span)
for (1) cfg3 (40 Msps x 256 channels, 256 steps) and (2) eight cfg2 receivers in one MultiFrontend.  REPS repetitions of each arm:
Msamples/s of the timed steps (bench.py's `value` arithmetic: steps x input_size x receivers / wall time including the draining poll),
then one timed-launch pass per arm for the steady-state step period and stage_times().  One JSON line per workload.
  python profiles/spectrum_monitor.py [cfg3|multi] ... [bins=N]     (default: both workloads, 4096 bands)
steady_state_ms_per_step = wall time of the timed steps / steps, draining poll included (1 / bench.py's `value`, per step).
The kernel's own time comes from a separate run under `rocprofv3 --kernel-trace --stats -- python profiles/spectrum_monitor.py cfg3`."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
import dumphfdl_amd as hf

STEPS, WARM, REPS, BINS, EVERY = 256, 8, 3, 4096, 32


def run(fe, push_step, nrx, nblocks, first, arm):
    monitor = arm != "off"
    fe.spectrum_enable(BINS if monitor else 0, hann=True, maxhold=True)
    if arm == "rows":
        fe.spectrum_history(64)
    nxt, rows = [0] * nrx, 0
    for i in range(WARM):
        push_step((first + i) % nblocks)
    fe.poll_pdus(16384 * nrx)
    torch.cuda.synchronize()
    reads = 0
    t0 = time.perf_counter()
    for i in range(STEPS):
        push_step((first + WARM + i) % nblocks)
        if arm == "on" and i % EVERY == EVERY - 1:
            for r in range(nrx):
                reads += fe.spectrum_read(r, reset=True)["blocks"]
        if arm == "rows":
            if i % EVERY == EVERY - 1:
                fe.spectrum_row_close()
            for r in range(nrx):
                got = fe.spectrum_rows(r, from_row=nxt[r], max_rows=4, wait=False)
                nxt[r], rows = got["next_row"], rows + sum(got["blocks"])
    pd = len(fe.poll_pdus(16384 * nrx))
    if arm == "rows":
        for r in range(nrx):
            rows += sum(fe.spectrum_rows(r, from_row=nxt[r], wait=True)["blocks"])
        reads = rows
    torch.cuda.synchronize()
    return time.perf_counter() - t0, pd, reads


def measure(name, fe, push_step, nrx, nblocks, n):
    fe.enable_taps(False)
    ARMS = ("off", "on", "noread", "rows")
    rates, pdus, ms = {a: [] for a in ARMS}, {a: [] for a in ARMS}, {a: [] for a in ARMS}
    for rep in range(REPS):
        for mon in ARMS:
            el, pd, reads = run(fe, push_step, nrx, nblocks, rep * STEPS, mon)
            assert reads == (nrx * (WARM + (STEPS // EVERY) * EVERY) if mon in ("on", "rows") else 0)       # the warm-up blocks are in the first average / row
            rates[mon].append(round(nrx * STEPS * n / el / 1e6, 1))
            ms[mon].append(round(1e3 * el / STEPS, 4))
            pdus[mon].append(pd)
    timed = {}
    for mon in ARMS:
        fe.reset_timers(True)
        run(fe, push_step, nrx, nblocks, 0, mon)
        timed[mon] = dict(step_period_ms=round(fe.step_period_ms(), 4), stage_times_ms_launches={k: (round(v[0], 3), v[1]) for k, v in fe.stage_times().items()})
        fe.reset_timers(False)
    g = fe.geometry
    floor_us = nrx * g.fft_size * 8 / 8e12 * 1e6
    off = rates["off"]
    print(json.dumps(dict(workload=name, receivers=nrx, fft_size=g.fft_size, bins=BINS, steps=STEPS, reps=REPS,
                          off_Msamples_s=off, on_Msamples_s=rates["on"], noread_Msamples_s=rates["noread"], rows_Msamples_s=rates["rows"],
                          steady_state_ms_per_step=ms, rows_over_off=round(float(np.mean(rates["rows"]) / np.mean(off)), 4), off_spread_pct=round(100 * (max(off) - min(off)) / np.mean(off), 2),
                          on_over_off=round(float(np.mean(rates["on"]) / np.mean(off)), 4), noread_over_off=round(float(np.mean(rates["noread"]) / np.mean(off)), 4),
                          pdus_off=pdus["off"], pdus_on=pdus["on"], pdus_rows=pdus["rows"], timed_off=timed["off"], timed_on=timed["on"], timed_noread=timed["noread"], timed_rows=timed["rows"], monitor_read_floor_us=round(floor_us, 2))), flush=True)


for a in sys.argv[1:]:
    if a.startswith("bins="):
        BINS = int(a[5:])
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
