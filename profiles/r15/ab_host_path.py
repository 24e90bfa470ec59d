"""A/B of the C host path: hfdl_replay + libhfdl_host.so built from the parent commit's dumphfdl_amd/host (in PARENT_DIR, beside a
copy of the same libhfdl_gpu.so) against this tree's, run alternately on the recording bench.py's host_path leg writes, with that
leg's command line.  One process at a time; stops at the first failure.

    python profiles/r15/ab_host_path.py PARENT_DIR RUNS cfg2,cfg3 OUT.json
"""
import json
import os
import subprocess
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench
import dumphfdl_amd as hf

parent_dir, runs_each, workloads, out_path = sys.argv[1], int(sys.argv[2]), sys.argv[3].split(","), sys.argv[4]
exes = {"parent": os.path.join(parent_dir, "hfdl_replay"), "new": os.path.join(ROOT, "dumphfdl_amd", "hfdl_replay")}
results = {}
for name in workloads:
    w = bench.WORKLOADS[name]
    whole = int(np.floor(np.float32(w["fs"]) / np.float32(5400)))
    decim = 1 << (whole.bit_length() - 1)              # compute_fft_decimation_rate()
    g = hf.plan_geometry(decim, 250 / w["fs"])
    x, _ = bench.make_input(w, g.input_size, 0, 1)
    freqs = bench.channel_plan(w)
    path = "/dev/shm/hfdl_ab_%s.cf32" % name
    x.view(np.float32).tofile(path)
    loops = max(1, int(np.ceil(1.5 * 2.5e9 / len(x))))
    runs = {"parent": [], "new": []}
    try:
        for i in range(runs_each):
            for which in (("parent", "new") if i % 2 == 0 else ("new", "parent")):      # who goes first alternates
                cmd = ["timeout", "-k", "10", "120", exes[which], "--bench", "--loop", str(loops), "--iq-file", path, "--sample-rate", str(w["fs"]),
                       "--sample-format", "CF32", "--device", "0", "--centerfreq", "%.3f" % (w["centerfreq"] / 1e3)] + ["%.3f" % (f / 1e3) for f in freqs]
                out = subprocess.run(cmd, capture_output=True, text=True)
                line = [l for l in out.stdout.splitlines() if l.startswith("{")]
                if out.returncode != 0 or not line:
                    print("FAILED", name, which, i, out.returncode, out.stderr[-1000:], flush=True)
                    sys.exit(1)
                r = json.loads(line[-1])
                runs[which].append({k: r[k] for k in ("value", "blocks", "samples", "seconds", "pdus", "thread_s", "pipeline_drains", "zero_copy_ring")})
                print(name, which, i, r["value"], r["thread_s"], r["pipeline_drains"], r["pdus"], flush=True)
    finally:
        os.remove(path)
    results[name] = dict(input_size=g.input_size, blocks_in_file=len(x) // g.input_size, loops=loops, runs=runs)
    for which in ("parent", "new"):
        v = sorted(r["value"] for r in runs[which])
        print(name, which, "min %.0f median %.0f max %.0f" % (v[0], float(np.median(v)), v[-1]), flush=True)
    json.dump(results, open(out_path, "w"), indent=1)
