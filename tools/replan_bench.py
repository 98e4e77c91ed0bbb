#!/usr/bin/env python3
"""Warm-started replanning, timed: per-call latency of the deployed batch sizes under graph replay.

For each batch size B and each DDIM step count n it times, on one GPU,
  cold    LDPAgent.sample (the full n-step loop, from noise)
  warm    LDPAgent.sample_warm with warm_steps = n/10, n/5, n/2 (the last k steps from the shifted, noised previous plan)
  replanner  Replanner.act with warm_steps = n/5 and every row warm (the same call through the slot table, in place)
  init    the warm-init launch alone (HipEngine.plan_warm_init)
A figure is the median over `--repeats` windows of `--steps` calls each (every call waited for: host clock around enqueue + completion
point), with the lowest and highest window beside it; all shapes are warmed up (graphs captured) before the first window.  Prints ONE
JSON line.  `fixed_ms` / `per_step_ms` are the least-squares line through (executed steps, median ms) of the cold and warm calls of one
(B, n): the per-call cost that does not scale with k, and the cost of one more step.

  python tools/replan_bench.py
  python tools/replan_bench.py --lib /path/to/libldp_hip.so --cold-only     (another build's cold path on the same box: A/B)

Not the driver's bench line (bench.py is)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

NEW_SYMBOLS = ("ldp_plan_sample_range", "ldp_plan_warm_init", "ldp_agent_resample")


def windows(fn, steps, warmup, repeats):
    """ms per call: (median, min, max) over `repeats` windows of `steps` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / steps * 1e3)
    return [round(float(v), 4) for v in (np.median(out), min(out), max(out))]


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--batches", type=int, nargs="+", default=[1, 5, 16])
    p.add_argument("--n-steps", type=int, nargs="+", default=[50, 100])
    p.add_argument("--steps", type=int, default=20, help="calls per timed window")
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeats", type=int, default=7, help="timed windows per figure")
    p.add_argument("--cold-only", action="store_true", help="time the cold sample() alone (a build without the replanning entry points)")
    p.add_argument("--lib", default=None, metavar="PATH", help="load this build of libldp_hip instead of the in-tree one (same-box A/B)")
    a = p.parse_args()
    from latent_diffusion_planning_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
        if a.cold_only:                                    # the other build may predate the replanning symbols
            for s in NEW_SYMBOLS:
                _lib.SIGNATURES.pop(s, None)
    from latent_diffusion_planning_amd.agent import LDPAgent
    from tests import cfgs
    torch.cuda.set_device(0)
    data = cfgs.RM_LIFT
    ag = LDPAgent.create(0, None, data["shape_meta"], **cfgs.agent_kwargs(data))
    eng = ag._engine
    rows = []
    for B in a.batches:
        batch = cfgs.synth_latent_batch(data, B, 1, 3)
        for n in a.n_steps:
            def cold():
                act, _ = ag.sample(batch, 1, sampler="ddim", n_steps=n)
                act.complete()
            row = dict(B=B, n_steps=n, cold_ms=windows(cold, a.steps, a.warmup, a.repeats))
            if not a.cold_only:
                _, m = ag.sample_warm(batch, 1, None, None, sampler="ddim", n_steps=n)
                prev = m["x"].complete().tensor
                pts = [(n, row["cold_ms"][0])]
                for k in sorted({max(1, n // 10), n // 5, n // 2}):
                    def warm():
                        act, _ = ag.sample_warm(batch, 1, prev, k, sampler="ddim", n_steps=n)
                        act.complete()
                    row[f"warm{k}_ms"] = windows(warm, a.steps, a.warmup, a.repeats)
                    pts.append((k, row[f"warm{k}_ms"][0]))
                rp = ag.replanner(B, n // 5, sampler="ddim", n_steps=n)      # the same call through the slot table, in place (no copy of prev)
                rp.act(batch, 1, list(range(B)))[0].complete()

                def steady():
                    rp.act(batch, 1, list(range(B)))[0].complete()
                row[f"replanner{n // 5}_ms"] = windows(steady, a.steps, a.warmup, a.repeats)
                row["init_ms"] = windows(lambda: eng.plan_warm_init(prev, n - n // 5, sampler="ddim", n_steps=n), a.steps, a.warmup, a.repeats)
                slope, icpt = np.polyfit([q[0] for q in pts], [q[1] for q in pts], 1)
                row["per_step_ms"], row["fixed_ms"] = round(float(slope), 4), round(float(icpt), 4)
                row["speedup_n5"] = round(row["cold_ms"][0] / row[f"warm{n // 5}_ms"][0], 3)
            rows.append(row)
    eng.check_fault()
    print(json.dumps(dict(tool="replan_bench", config="rm_lift", sampler="ddim", figures="[median, min, max] ms per call", steps=a.steps,
                          repeats=a.repeats, lib=a.lib or "in-tree", version=_lib.load().ldp_version().decode(), rows=rows)), flush=True)


if __name__ == "__main__":
    main()
