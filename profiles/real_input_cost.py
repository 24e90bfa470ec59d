"""What real-sampled input costs (profiles/r25_experiments.md).  The protocol is profiles/iqbal_cost.py's.

  python profiles/real_input_cost.py [--workload cfg3] [--pairs 5] [--steps 256]
      TWO front ends in one process on the bench's device-resident stream: the workload's complex front end (fs, centre) and a real one of
      twice the rate whose equivalent stream it is (fs_r = 2 fs, base = centre - fs / 2): the same N', the same channels, the same bytes of
      filter taps.  The real one reads the very same device buffers, a cf32 block being 2 input_size floats (what the words say does not
      matter to the clock).  Timed segments of `steps` blocks alternate between the two, so drift of the machine hits both arms alike.
      Also, from the dispatches' own start / stop events (hfdl_gpu_frontend_stage_times): the forward FFT per block -- first pass start to
      last launch stop, which for the real front end is the untangle launch -- of either arm; their difference is the untangle launch
      (8 bytes read and 8 written per bin) and what it displaces.
One JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=256)
    args = ap.parse_args()
    import torch
    import bench
    import dumphfdl_amd as hf
    from dumphfdl_amd import frontend as F
    w = bench.WORKLOADS[args.workload]
    freqs = bench.channel_plan(w)
    fes = {"complex": hf.Frontend(w["fs"], w["centerfreq"], freqs), "real": hf.RealFrontend(2 * w["fs"], [(w["centerfreq"] - w["fs"] // 2, freqs)])}
    g = fes["complex"].geometry
    gr = fes["real"].geometry
    assert (g.fft_size, g.input_size, g.channels, g.sample_rate) == (gr.fft_size, gr.input_size, gr.channels, gr.sample_rate)
    x, _ = bench.make_input(w, g.input_size, 0, 1)
    nblocks = len(x) // g.input_size
    dev = torch.from_numpy(x.view(np.float32)).cuda()
    ptrs = [dev.data_ptr() + 8 * b * g.input_size for b in range(nblocks)]
    push = {"complex": lambda i: fes["complex"].push_block(ptrs[i]), "real": lambda i: fes["real"].push_real([ptrs[i]], F.SFMT_RF32, on_device=True)}
    step = {"complex": 0, "real": 0}
    for arm, fe in fes.items():
        fe.enable_taps(False)
        for _ in range(max(8, nblocks)):
            push[arm](step[arm] % nblocks); step[arm] += 1
        fe.poll_pdus()
    torch.cuda.synchronize()
    ms = {"complex": [], "real": []}
    fft_us = {"complex": [], "real": []}
    for _ in range(args.pairs):
        for arm, fe in fes.items():
            fe.reset_timers(True)
            el, _, step[arm] = bench.timed_blocks(torch, fe, push[arm], args.steps, step[arm], nblocks)
            ms[arm].append(el / args.steps * 1e3)
            t, n = fe.stage_times()["fft"]
            fft_us[arm].append(t / max(1, n) * 1e3)
            fe.reset_timers(False)
    med = {a: statistics.median(v) for a, v in ms.items()}
    fmed = {a: statistics.median(v) for a, v in fft_us.items()}
    out = dict(workload=args.workload, steps=args.steps, fft_size=g.fft_size, block_samples_equiv=g.input_size, channels=g.channels, real_rate=2 * w["fs"],
               ms_per_step=ms, median_ms_per_step=med, real_minus_complex_us=(med["real"] - med["complex"]) * 1e3,
               forward_fft_us=fft_us, forward_fft_median_us=fmed, untangle_by_difference_us=fmed["real"] - fmed["complex"], untangle_bytes=16 * g.fft_size)
    for fe in fes.values():
        fe.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
