#!/usr/bin/env python3
"""Generates tests/golden/dp_vae_*.npz (DPVAEAgent) from the CPU oracle of tests/dp_oracle.py.  Run from the repo root:

    python tests/golden/make_golden_dp.py            # all cases
    python tests/golden/make_golden_dp.py NAME ...   # selected cases

Each file holds the seeded float32 inputs (`in_*`), the seeds of what is regenerated (`seed_*`: the U-Net parameters through
weights.init_planner_params, the per-step DDPM noise through PCG64) and the float64 oracle outputs (`out_*`).  Training results are
stored as per-leaf digests (tests/util.py tree_digest), in the format of agent_update_rm.npz.
NOTE (parity unpinned): the outputs come from this repository's restatement of the reference algorithm (no JAX here).
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import cfgs, dp_oracle  # noqa: E402
from tests.util import rng, tree_digest  # noqa: E402

OH, T, AH = 2, 16, 8
DECAY = 0.99
N_UPDATE = 10


def step_noise(seed, n_steps, B, A):
    return rng(seed).standard_normal((n_steps, B, T, A)).astype(np.float32)


def sample_case(cfg, sampler, n_steps, B):
    data = cfgs.BY_NAME[cfg]
    A = data["shape_meta"]["ac_dim"]
    batch = cfgs.synth_latent_batch(data, B, OH, 710 + B)
    g = rng(720 + B)
    x_init = g.standard_normal((B, T, A)).astype(np.float32)
    seeds = dict(params=21, noise=730 + B)
    inp = {f"obs__{k}": v for k, v in batch["obs"].items()}
    inp["x_init"] = x_init

    def compute():
        p = dp_oracle.params(data, seeds["params"], OH)
        nz = step_noise(seeds["noise"], n_steps, B, A) if sampler == "ddpm" else None
        return dict(action=dp_oracle.sample(data, p, batch["obs"], x_init, nz, OH, AH, sampler, n_steps))
    return inp, seeds, compute


def update_case(cfg, B=4):
    data = cfgs.BY_NAME[cfg]
    A = data["shape_meta"]["ac_dim"]
    inp, steps = {}, []
    for s in range(N_UPDATE):
        batch = cfgs.synth_latent_batch(data, B, OH, 800 + s)
        g = rng(900 + s)
        act = g.uniform(-1, 1, size=(B, T, A)).astype(np.float32)
        t = g.integers(0, 100, B)
        noise = g.standard_normal((B, T, A)).astype(np.float32)
        for k, v in batch["obs"].items():
            inp[f"s{s}_obs__{k}"] = v
        inp[f"s{s}_actions"], inp[f"s{s}_t"], inp[f"s{s}_noise"] = act, t.astype(np.float32), noise
        steps.append((batch["obs"], act, t, noise))
    seeds = dict(params=31)

    def compute():
        from oracle import train as OT
        p0 = dp_oracle.params(data, seeds["params"], OH)
        sched = OT.warmup_cosine_decay_schedule(1e-6, 1e-4, 500, 100000, 1e-6)
        first = dp_oracle.loss_and_grads(data, p0, *steps[0], OH)
        p1, e1, _, _ = dp_oracle.train(data, p0, steps[:1], OH, DECAY, sched)
        pn, en, losses, norms = dp_oracle.train(data, p0, steps, OH, DECAY, sched)
        return dict(grads=tree_digest(first["grads"], 11), params_after_1=tree_digest(p1, 13), ema_after_1=tree_digest(e1, 17),
                    params_after_n=tree_digest(pn, 15), ema_after_n=tree_digest(en, 19), loss=np.asarray(losses), g_norm=np.asarray(norms),
                    lr=np.asarray([sched(i) for i in range(N_UPDATE)]))
    return inp, seeds, compute


CASES = {
    "dp_vae_sample_rm_ddpm100_b3": (sample_case, ("rm", "ddpm", 100, 3)),
    "dp_vae_sample_rm_ddim50_b5": (sample_case, ("rm", "ddim", 50, 5)),
    "dp_vae_sample_aloha_ddpm100_b2": (sample_case, ("aloha", "ddpm", 100, 2)),
    "dp_vae_sample_aloha_ddim50_b3": (sample_case, ("aloha", "ddim", 50, 3)),
    "dp_vae_update_rm": (update_case, ("rm",)),
}


def golden_path(name):
    return os.path.join(ROOT, "tests", "golden", f"{name}.npz")


def main():
    for name in sys.argv[1:] or list(CASES):
        fn, args = CASES[name]
        inp, seeds, compute = fn(*args)
        t0 = time.time()
        out = compute()
        np.savez_compressed(golden_path(name), **{f"in_{k}": np.asarray(v, np.float32) for k, v in inp.items()},
                            **{f"seed_{k}": np.asarray(v, np.int64) for k, v in seeds.items()},
                            **{f"out_{k}": np.asarray(v, np.float64) for k, v in out.items()})
        print(f"{name}: {time.time() - t0:.1f}s, {os.path.getsize(golden_path(name)) / 1024:.0f} KiB", flush=True)


if __name__ == "__main__":
    main()
