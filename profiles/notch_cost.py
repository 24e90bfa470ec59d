"""What the adaptive carrier canceller costs (profiles/r22_experiments.md).

  python profiles/notch_cost.py onoff --workload cfg3 [--pairs 5] [--steps 256]
      ONE front end on the bench's device-resident stream; timed segments of `steps` blocks alternate canceller off / on 16 channels / on
      every channel (mu 0.002), so drift of the machine hits the arms alike.  Then one more segment per arm with the launch timers on:
      the demodulator stream's kernel time per half.  Also the canceller's launch alone on one half of the workload (hfdl_gpu_notch_rows
      on channels x (fold_batch x outputs_per_block) samples: HIP events around the launch, copies excluded).
  python profiles/notch_cost.py off --workload cfg3 [--rounds 5] [--steps 256]
      the same segments, never enabling anything: run alternately on two builds of the library (HFDL_GPU_LIB) to set `off` against the
      parent commit.  A build without the canceller's entry points loads here too.
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


class _Absent:
    argtypes = restype = None


class _AnyBuild(C.CDLL):
    """a library build that may lack newer entry points: binding their argument types is a no-op, calling them is an error"""
    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            if name.startswith("hfdl_gpu_"):
                return _Absent()
            raise


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["onoff", "off"])
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--mu", type=float, default=0.002)
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
        some = list(range(0, g.channels, max(1, g.channels // 16)))[:16]
        select = {"off": lambda: fe.notch_enable(0.0), "on16": lambda: fe.notch_enable(args.mu, some), "all": lambda: fe.notch_enable(args.mu)}
        arms = {a: [] for a in select}
        pdus = {a: [] for a in select}
        fe.notch_enable(args.mu)                         # the allocation happens here, outside the timed segments
        for _ in range(args.pairs):
            for arm, enable in select.items():
                enable()
                m, n, step = segment(step)
                arms[arm].append(m)
                pdus[arm].append(n)
        med = {a: statistics.median(v) for a, v in arms.items()}
        out.update(ms_per_step=arms, median_ms_per_step=med, pdus=pdus, mu=args.mu, selected_on16=len(some),
                   all_minus_off_us=(med["all"] - med["off"]) * 1e3, on16_minus_off_us=(med["on16"] - med["off"]) * 1e3)
        # the streams' kernel time per half, launch timers on (the canceller's launch itself is not a timed stage: it shows as the gap
        # between what the demodulator stream's kernels sum to and what the block period is)
        stages = {}
        for arm, enable in select.items():
            enable()
            fe.reset_timers(True)
            _, _, step = segment(step)
            st = fe.stage_times()
            halves = max(1, st["ifft"][1])
            stages[arm] = dict(halves=halves, period_ms=fe.step_period_ms(), **{k: v[0] / halves for k, v in st.items()})
            fe.reset_timers(False)
        out.update(stage_ms_per_half=stages)
        st = fe.notch_stats(0)
        out.update(resets_channel0=st["resets"], tap_energy_channel0=float(st["tap_energy"]))
        # the launch alone: every channel walks one half's worth of samples
        n = g.fold_batch * g.outputs_per_block
        rng = np.random.default_rng(1)
        rows = (0.05 * (rng.standard_normal((g.channels, n)) + 1j * rng.standard_normal((g.channels, n)))).astype(np.complex64)
        stage = []
        for _ in range(5):
            hf.notch_rows(rows, args.mu)
            stage.append(F.last_stage_ms())
        out.update(notch_launch_alone_ms=stage, notch_launch_alone_median_ms=statistics.median(stage), half_blocks=g.fold_batch, samples_per_channel=n,
                   ns_per_sample=statistics.median(stage) * 1e6 / n)
    fe.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
