#!/usr/bin/env python3
"""K cfg2 receivers on ONE MI355X, input resident in HBM, aggregate wideband rate, two arms in one process, alternating:
  (a) K independent front ends (Frontend), blocks pushed round-robin -- a single demodulator-bound receiver occupies 96 of 1024 SIMDs;
  (b) ONE front end of K receivers (MultiFrontend, hfdl_gpu_frontend_create_multi): one batched forward FFT, one fold, one inverse FFT,
      one demodulator and one burst decoder launch per step for all K x 32 channels.
Receiver r: bench.WORKLOADS["cfg2"] with its own seed and centre frequency.  Prints one JSON line per K: the aggregate Msamples/s of each
arm per repetition, stage_times() of arm (b) from a timed extra pass, and the PDUs per receiver of both arms."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
import dumphfdl_amd as hf

W = bench.WORKLOADS["cfg2"]
STEPS, WARM, REPS = 256, 8, 3


def receivers(K):
    ws = [dict(W, seed=100 + r, centerfreq=W["centerfreq"] + 3_000_000 * (r - K // 2)) for r in range(K)]
    return ws, [bench.channel_plan(w) for w in ws]


def run(push_step, poll, nblocks, first):
    """WARM steps + a drain, then STEPS timed steps (from block `first` on, cycling the resident stretch) and a draining poll."""
    for i in range(WARM):
        push_step((first + i) % nblocks)
    poll()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(STEPS):
        push_step((first + WARM + i) % nblocks)
    pd = poll()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, pd


out = []
for K in (1, 2, 4, 8):
    ws, freqs = receivers(K)
    single = [hf.Frontend(w["fs"], w["centerfreq"], fr, device=0) for w, fr in zip(ws, freqs)]
    multi = hf.MultiFrontend(W["fs"], [(w["centerfreq"], fr) for w, fr in zip(ws, freqs)], device=0)
    g = multi.geometry
    n = g.input_size
    xs = [bench.make_input(w, n, 0, 1)[0] for w in ws]
    nblocks = min(len(x) for x in xs) // n
    dev = [torch.from_numpy(np.array(x).view(np.float32)).cuda() for x in xs]
    ptrs = [[d.data_ptr() + 8 * b * n for b in range(nblocks)] for d in dev]
    torch.cuda.synchronize()
    for fe in single + [multi]:
        fe.enable_taps(False)

    def step_a(b):
        for r, fe in enumerate(single):
            fe.push_block(ptrs[r][b])

    def poll_a():
        return [len(fe.poll_pdus(16384)) for fe in single]

    def step_b(b):
        multi.push_blocks([p[b] for p in ptrs])

    def poll_b():
        got = multi.poll_pdus(16384 * K)
        return [sum(1 for p in got if p["receiver"] == r) for r in range(K)]

    rates = {"a": [], "b": []}
    pdus = {"a": [], "b": []}
    for rep in range(REPS):
        for arm, (st, po) in (("a", (step_a, poll_a)), ("b", (step_b, poll_b))):
            el, pd = run(st, po, nblocks, rep * STEPS)
            rates[arm].append(round(K * STEPS * n / el / 1e6))
            pdus[arm].append(pd)
    # arm (b) once more with the stage timers on: which stage bounds the step
    multi.reset_timers(True)
    el, _ = run(step_b, poll_b, nblocks, 0)
    st = {k: (round(v[0], 2), v[1]) for k, v in multi.stage_times().items()}
    multi.reset_timers(False)
    out.append(dict(receivers=K, channels=g.channels, fold_batch=g.fold_batch, demod_batch=g.demod_batch, fold_slices=g.fold_slices,
                    separate_Msamples_s=rates["a"], multi_Msamples_s=rates["b"],
                    separate_mean=round(float(np.mean(rates["a"]))), multi_mean=round(float(np.mean(rates["b"]))),
                    ratio=round(float(np.mean(rates["b"]) / np.mean(rates["a"])), 2),
                    pdus_per_receiver_separate=pdus["a"], pdus_per_receiver_multi=pdus["b"],
                    multi_timed_pass_Msamples_s=round(K * STEPS * n / el / 1e6), multi_stage_times_ms_launches=st))
    print(json.dumps(out[-1]), flush=True)
    for fe in single + [multi]:
        fe.close()
    del dev
print(json.dumps(out))
