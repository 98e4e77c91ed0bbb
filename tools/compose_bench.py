#!/usr/bin/env python3
"""Composed planning, timed: what a closed-loop control call costs under graph replay when it resumes from the last
plan, ends in a goal and follows a guide -- next to the calls the project already had.

For each batch size B it times, on one GPU and in ONE process,
  plan_ddim    LDPAgent.plan warm at k = n / 5 with a clamp goal and a guide (smoothness with the anchor, box bounds), DDIM-n
  plan_dpmpp   the same call under sampler "dpmpp" with --solver-steps steps (warm at a fifth of them)
  sample_warm  LDPAgent.sample_warm at k = n / 5, DDIM-n (the warm call without goal or guide)
  sample       LDPAgent.sample, DDIM-n (the cold call)
The calls are ALTERNATED: every repeat times one window of `--steps` calls of each, in turn, so drift of the clocks or of the box hits
all alike.  Every call is waited for (host clock around enqueue + completion point); all shapes are warmed up (graphs captured) before the
first window.  A figure is [median, min, max] ms per call over the `--repeats` windows.
Prints ONE JSON line.  Not the driver's bench line (bench.py is).  Control quality is not evaluated here (tools/toy_reach.py measures it on a toy task).

  python tools/compose_bench.py
  python tools/compose_bench.py --lib /path/to/libldp_hip.so     (another build on the same box: A/B)"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def window(fn, steps):
    """ms per call over one window of `steps` calls."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def stats(v):
    return [round(float(x), 4) for x in (np.median(v), min(v), max(v))]


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--batches", type=int, nargs="+", default=[1, 16])
    p.add_argument("--ddim-steps", type=int, default=50)
    p.add_argument("--solver-steps", type=int, default=10)
    p.add_argument("--steps", type=int, default=10, help="calls per timed window")
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeats", type=int, default=7, help="timed windows per figure")
    p.add_argument("--lib", default=None, metavar="PATH", help="load this build of libldp_hip instead of the in-tree one (same-box A/B)")
    a = p.parse_args()
    from latent_diffusion_planning_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    from latent_diffusion_planning_amd.agent import LDPAgent
    from tests import cfgs
    torch.cuda.set_device(0)
    data = cfgs.RM_LIFT
    ag = LDPAgent.create(0, None, data["shape_meta"], **cfgs.agent_kwargs(data))
    eng = ag._engine
    n, ns = a.ddim_steps, a.solver_steps
    k, ks = max(1, n // 5), max(1, ns // 5)
    rows = []
    for B in a.batches:
        batch = cfgs.synth_latent_batch(data, B, 1, 3)
        goal = ag._goal_embedding(cfgs.synth_latent_batch(data, B, 1, 4)["obs"], B)
        guide = ag.build_guide(B, smooth=0.1, anchor=True, bound_weight=0.5, lo=-0.9, hi=0.9)
        prev = ag.sample_warm(batch, 1, None, None, sampler="ddim", n_steps=n)[1]["x"].tensor

        def plan_ddim():
            ag.plan(batch, 1, guide=guide, goal=goal, mode="clamp", prev=prev, warm_steps=k, sampler="ddim", n_steps=n)[0].complete()

        def plan_dpmpp():
            ag.plan(batch, 1, guide=guide, goal=goal, mode="clamp", prev=prev, warm_steps=ks, sampler="dpmpp", n_steps=ns)[0].complete()

        def sample_warm():
            ag.sample_warm(batch, 1, prev, k, sampler="ddim", n_steps=n)[0].complete()

        def sample():
            ag.sample(batch, 1, sampler="ddim", n_steps=n)[0].complete()
        fns = dict(plan_ddim=plan_ddim, plan_dpmpp=plan_dpmpp, sample_warm=sample_warm, sample=sample)
        for fn in fns.values():
            for _ in range(a.warmup):
                fn()
        t = {name: [] for name in fns}
        for _ in range(a.repeats):                             # alternated: one window of each per repeat
            for name, fn in fns.items():
                t[name].append(window(fn, a.steps))
        row = dict(B=B, ddim_steps=n, ddim_warm_steps=k, solver_steps=ns, solver_warm_steps=ks)
        for name in fns:
            row[f"{name}_ms"] = stats(t[name])
        row["plan_ddim_extra_ms"] = stats(np.array(t["plan_ddim"]) - np.array(t["sample_warm"]))
        rows.append(row)
    eng.check_fault()
    print(json.dumps(dict(tool="compose_bench", config="rm_lift", figures="[median, min, max] ms per call", steps=a.steps,
                          repeats=a.repeats, lib=a.lib or "in-tree", version=_lib.load().ldp_version().decode(), rows=rows)), flush=True)


if __name__ == "__main__":
    main()
