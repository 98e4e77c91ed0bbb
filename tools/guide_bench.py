#!/usr/bin/env python3
"""Guided planning, timed: what the guided step costs per call under graph replay.

For each batch size B (DDIM-50 unless told otherwise) it times, on one GPU and in ONE process,
  free      LDPAgent.sample (the unguided call of the same build)
  guided    LDPAgent.sample_guided with a prebuilt guide: a soft goal at t = action_horizon - 1, smoothness with the anchor, box bounds
The two are ALTERNATED: every repeat times one window of `--steps` calls of each, in turn, so drift of the clocks or of the box hits
both alike.  Every call is waited for (host clock around enqueue + completion point); both shapes are warmed up (graphs captured)
before the first window.  A figure is [median, min, max] ms per call over the `--repeats` windows; `extra_ms` is the median of the
per-repeat differences to the free window of the same repeat (it holds the eager staging of the guide and the cost launch behind the
loop as well), `extra_us_per_step` that difference over the n guided steps.
Prints ONE JSON line.  Not the driver's bench line (bench.py is).

  python tools/guide_bench.py
  python tools/guide_bench.py --lib /path/to/libldp_hip.so     (another build on the same box: A/B)"""
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
    p.add_argument("--batches", type=int, nargs="+", default=[1, 256])
    p.add_argument("--schedules", nargs="+", default=["ddim:50"], help="sampler:steps")
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
    rows = []
    for B in a.batches:
        batch = cfgs.synth_latent_batch(data, B, 1, 3)
        goal = ag._goal_embedding(cfgs.synth_latent_batch(data, B, 1, 4)["obs"], B)
        guide = ag.build_guide(B, goal=goal, smooth=0.1, anchor=True, bound_weight=0.5, lo=-0.9, hi=0.9)
        for sched in a.schedules:
            sampler, n = sched.split(":")[0], int(sched.split(":")[1])
            kw = dict(sampler=sampler, n_steps=n)

            def free():
                ag.sample(batch, 1, **kw)[0].complete()

            def guided():
                ag.sample_guided(batch, 1, guide=guide, **kw)[0].complete()
            fns = dict(free=free, guided=guided)
            for fn in fns.values():
                for _ in range(a.warmup):
                    fn()
            t = {k: [] for k in fns}
            for _ in range(a.repeats):                         # alternated: one window of each per repeat
                for k, fn in fns.items():
                    t[k].append(window(fn, a.steps))
            row = dict(B=B, sampler=sampler, n_steps=n)
            for k in fns:
                row[f"{k}_ms"] = stats(t[k])
            d = np.array(t["guided"]) - np.array(t["free"])
            row["guided_extra_ms"] = stats(d)
            row["guided_extra_us_per_step"] = round(float(np.median(d)) / n * 1e3, 3)
            rows.append(row)
    eng.check_fault()
    print(json.dumps(dict(tool="guide_bench", config="rm_lift", figures="[median, min, max] ms per call", steps=a.steps,
                          repeats=a.repeats, lib=a.lib or "in-tree", version=_lib.load().ldp_version().decode(), rows=rows)), flush=True)


if __name__ == "__main__":
    main()
