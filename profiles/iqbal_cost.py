"""What the I/Q imbalance and DC corrector costs (profiles/r24_experiments.md).  The protocol is
profiles/blanker_cost.py's.

  python profiles/iqbal_cost.py onoff --workload cfg3 [--pairs 5] [--steps 256]
      ONE front end on the bench's device-resident stream; timed segments of `steps` blocks alternate corrector off / on (alpha 1/8), so
      drift of the machine hits both arms alike.  Also the corrector's launch alone on blocks of the workload's input_size
      (hfdl_gpu_iqbal_blocks: HIP events around four launches, copies excluded, divided by four).
  python profiles/iqbal_cost.py off --workload cfg3 [--rounds 5] [--steps 256]
      the same segments, never enabling anything: run alternately on two builds of the library (HFDL_GPU_LIB) to set `off` against the
      parent commit.  A build without the corrector's entry points loads here too.
One JSON line each."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from blanker_cost import _AnyBuild  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["onoff", "off"])
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--alpha", type=float, default=0.125)
    args = ap.parse_args()
    import torch
    import bench
    import dumphfdl_amd as hf
    from dumphfdl_amd import frontend as F
    if args.mode == "off":
        F._lib = F._bind(_AnyBuild(F.lib_path(), mode=C.RTLD_GLOBAL))
    w = bench.WORKLOADS[args.workload]
    freqs = bench.channel_plan(w)
    fe = hf.Frontend(w["fs"], w["centerfreq"], freqs)
    g = fe.geometry
    fe.enable_taps(False)
    x, _ = bench.make_input(w, g.input_size, 0, 1)
    nblocks = len(x) // g.input_size
    dev = torch.from_numpy(x.view(np.float32)).cuda()
    ptrs = [dev.data_ptr() + 8 * b * g.input_size for b in range(nblocks)]
    push = lambda i: fe.push_block(ptrs[i])
    step = 0
    for _ in range(max(8, nblocks)):
        push(step % nblocks); step += 1
    fe.poll_pdus()
    torch.cuda.synchronize()

    def segment(step):
        el, raw, step = bench.timed_blocks(torch, fe, push, args.steps, step, nblocks)
        return el / args.steps * 1e3, sum(n for _, n in raw), step

    out = dict(mode=args.mode, workload=args.workload, lib=os.path.basename(F.lib_path()), steps=args.steps, block_samples=g.input_size, channels=g.channels)
    if args.mode == "off":
        ms = []
        for _ in range(args.rounds):
            m, _, step = segment(step)
            ms.append(m)
        out.update(ms_per_step=ms, median_ms_per_step=statistics.median(ms))
    else:
        arms = {"off": [], "on": []}
        pdus = {"off": [], "on": []}
        fe.iqbal_enable(args.alpha)                      # the allocation happens here, outside the timed segments
        for _ in range(args.pairs):
            for arm in ("off", "on"):
                fe.iqbal_enable(args.alpha if arm == "on" else 0.0)
                m, n, step = segment(step)
                arms[arm].append(m)
                pdus[arm].append(n)
        st = fe.iqbal_stats()
        med = {a: statistics.median(v) for a, v in arms.items()}
        out.update(ms_per_step=arms, median_ms_per_step=med, on_minus_off_us=(med["on"] - med["off"]) * 1e3, pdus=pdus, alpha=args.alpha,
                   blocks=st["blocks"], refused=st["refused"], kappa_abs=float(abs(st["kappa"])))
        four = x[:4 * g.input_size]
        stage = []
        for _ in range(5):
            hf.iqbal_blocks(four, g.input_size, F.SFMT_CF32, args.alpha)
            stage.append(F.last_stage_ms() * 1e3 / 4)
        out.update(launch_alone_us=stage, launch_alone_median_us=statistics.median(stage), bytes_moved=g.input_size * (8 + 8))
    fe.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
