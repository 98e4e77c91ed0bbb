#!/usr/bin/env python3
"""The DPM-Solver++(2M) sampler, measured: what a few-step solver call costs, and how far it lands from the finest DDIM
solution the engine has.  Two tables, ONE JSON line.  Measurements, nothing is asserted.  Not the driver's bench line (bench.py is).

latency   For each batch size B, on one GPU and in ONE process: LDPAgent.sample(sampler='dpmpp') at --dpmpp-steps and
          LDPAgent.sample(sampler='ddim') at --ddim-steps, ALTERNATED: every repeat times one window of `--steps` calls of each arm in
          turn, so drift of the clocks or of the box hits all arms alike.  Every call is waited for; all arms are warmed up (graphs
          captured) before the first window.  A figure is [median, min, max] ms per call over the `--repeats` windows.  The ddim arms
          are the cold path as it was before this sampler existed (it adds no launch to them): run the tool on two builds to compare.
error     On the real U-Net with random weights (tests.util.planner_params) and with the trained-like heavy-tailed set of
          test_hip_stress.py: the relative RMS deviation of dpmpp-10 / dpmpp-20 on both grids and of DDIM-10 / -20 / -50 from the
          reference solution -- DDIM-100 over the steps [step_of(t_first), 100) from the same x_T (plan_sample_range with x_init), the
          finest solution of the same ODE from the same starting level the engine has.  Each arm starts from x_T at ITS first timestep's
          level; x_T is one N(0, 1) draw, which is what every loop starts from.

  python tools/solver_bench.py
  python tools/solver_bench.py --lib /path/to/libldp_hip.so --skip error     (another build on the same box: A/B)"""
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


def rel_rms(a, b):
    return float(torch.sqrt(((a - b) ** 2).mean() / (b ** 2).mean()))


def latency(a):
    from latent_diffusion_planning_amd.agent import LDPAgent
    from tests import cfgs
    data = cfgs.RM_LIFT
    ag = LDPAgent.create(0, None, data["shape_meta"], **cfgs.agent_kwargs(data))
    arms = [("dpmpp", n) for n in a.dpmpp_steps] + [("ddim", n) for n in a.ddim_steps]
    rows = []
    for B in a.batches:
        batch = cfgs.synth_latent_batch(data, B, 1, 3)
        fns = {}
        for sampler, n in arms:
            # (the IDM loop is DDIM with idm_steps = n where n divides its 100 training steps: the same rule for both samplers)
            fns[f"{sampler}{n}"] = (lambda s=sampler, k=n: ag.sample(batch, 1, sampler=s, n_steps=k)[0].complete())
        for fn in fns.values():
            for _ in range(a.warmup):
                fn()
        t = {k: [] for k in fns}
        for _ in range(a.repeats):                             # alternated: one window of each arm per repeat
            for k, fn in fns.items():
                t[k].append(window(fn, a.steps))
        row = dict(B=B)
        for k in fns:
            row[f"{k}_ms"] = stats(t[k])
        rows.append(row)
    ag._engine.check_fault()
    ag._engine.close()
    return rows


def error(a):
    from latent_diffusion_planning_amd import schedule as S
    from latent_diffusion_planning_amd.engine import HipEngine
    from tests.util import planner_params, planner_params_heavy
    D, T, B, n_train = 25, 8, a.error_batch, 100
    rows = []
    for name, params in (("random", planner_params(D=D)), ("heavy", planner_params_heavy(D=D))):
        eng = HipEngine(obs_dim=D, action_dim=7, global_cond_dim=D, pred_horizon=T, action_horizon=4)
        eng.load_params(planner=params)
        g = torch.Generator(device="cpu").manual_seed(5)
        cond = (torch.rand((B, D), generator=g) * 2 - 1).cuda()
        x_t = torch.randn((B, T, D), generator=g).cuda()
        ref = {}

        def reference(t_first):                                # DDIM-100 from the level of t_first down
            if t_first not in ref:
                ref[t_first] = eng.plan_sample_range(cond, n_train - 1 - t_first, n_train, x_init=x_t, sampler="ddim", n_steps=n_train)
            return ref[t_first]
        row = dict(weights=name, B=B)
        for n in a.error_dpmpp_steps:
            for spacing in ("logsnr", "uniform"):
                ts = eng.set_solver_timesteps(S.solver_timesteps(n_train, n, spacing))
                got = eng.plan_sample(cond, x_init=x_t, sampler="dpmpp", n_steps=n)
                row[f"dpmpp{n}_{spacing}"] = round(rel_rms(got, reference(int(ts[0]))), 5)
        for n in a.error_ddim_steps:
            got = eng.plan_sample(cond, x_init=x_t, sampler="ddim", n_steps=n)
            row[f"ddim{n}"] = round(rel_rms(got, reference(n_train - n_train // n)), 5)
        eng.check_fault()
        eng.close()
        rows.append(row)
    return rows


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--batches", type=int, nargs="+", default=[1, 16, 256])
    p.add_argument("--dpmpp-steps", type=int, nargs="+", default=[5, 10, 20])
    p.add_argument("--ddim-steps", type=int, nargs="+", default=[10, 50, 100])
    p.add_argument("--steps", type=int, default=10, help="calls per timed window")
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeats", type=int, default=7, help="timed windows per figure")
    p.add_argument("--error-batch", type=int, default=64)
    p.add_argument("--error-dpmpp-steps", type=int, nargs="+", default=[10, 20])
    p.add_argument("--error-ddim-steps", type=int, nargs="+", default=[10, 20, 50])
    p.add_argument("--skip", choices=["latency", "error"], default=None)
    p.add_argument("--lib", default=None, metavar="PATH", help="load this build of libldp_hip instead of the in-tree one (same-box A/B)")
    a = p.parse_args()
    from latent_diffusion_planning_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    torch.cuda.set_device(0)
    out = dict(tool="solver_bench", config="rm_lift", figures="[median, min, max] ms per call", steps=a.steps, repeats=a.repeats,
               lib=a.lib or "in-tree", version=_lib.load().ldp_version().decode())
    if a.skip != "latency":
        out["latency"] = latency(a)
    if a.skip != "error":
        out["error"] = error(a)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
