#!/usr/bin/env python3
"""Generates tests/golden/dp_resnet_*.npz (DPAgent and its ResNet-18 image encoder) from the CPU oracle of tests/dp_resnet_oracle.py.
Run from the repo root:

    python tests/golden/make_golden_dp_resnet.py            # all cases
    python tests/golden/make_golden_dp_resnet.py NAME ...   # selected cases

Each file holds the seeded inputs (`in_*`; frames as uint8), the seeds of what is regenerated (`seed_*`: encoder and U-Net parameters
through weights.init_resnet_params / init_planner_params, the per-step DDPM noise through PCG64), the float64 oracle outputs (`out_*`),
the float32 restatement's outputs (`out_*32`) and its error against float64 (`out_err32`).

The generator ASSERTS, on the CPU, the conditions the GPU tests rest on, and moves on to the next seed when one fails:
  * sampling goldens: the float32 restatement's actions are within ACTION_TOL = 5e-5 of the float64 ones -- half the project's 1e-4 bound,
    so the reference arithmetic alone stays inside it;
  * every golden: in the argmax-like regime (a softmax input of magnitude 16 or more) no two largest inputs of a (frame, channel) are
    closer than TIE_TOL = 1e-3 without being equal (dp_resnet_oracle.tie_gap).
tests/test_dp_agent_cpu.py recomputes both from the stored arrays.
NOTE (parity unpinned): the outputs come from this repository's restatement of the reference algorithm (no JAX here).
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import np64  # noqa: E402
from tests import dp_resnet_oracle as RO  # noqa: E402
from tests.util import rng  # noqa: E402

OH, T, AH = 2, 16, 8
ACTION_TOL, TIE_TOL = 5e-5, 1e-3
TRIES = 40
IMG_NORM = dict(min=0, max=255)


def step_noise(seed, n_steps, B, A):
    return rng(seed).standard_normal((n_steps, B, T, A)).astype(np.float32)


def rel_err(a, ref):
    ref = np.asarray(ref, np.float64)
    return float((np.abs(np.asarray(a, np.float64) - ref) / np.maximum(1.0, np.abs(ref))).max())


def frames_to_input(frames_u8):
    return np.asarray(np64.apply_norm(np.asarray(frames_u8, np.float32), IMG_NORM, True), np.float32)


def feature_params(kind, seed):
    return RO.heavy_params(seed) if kind == "heavy" else RO.W.init_resnet_params(RO.SPEC, seed=seed, perturb=True)


def features_case(kind, seed0, n=5):
    for seed in range(seed0, seed0 + TRIES):
        frames = RO.synth_frames(n, seed)
        p = feature_params(kind, seed)
        f64, logits = RO.encode(p, frames_to_input(frames), torch.float64, return_logits=True)
        if RO.tie_gap(logits) <= TIE_TOL:
            print(f"  seed {seed}: tie gap {RO.tie_gap(logits):.2e}, next seed", flush=True)
            continue
        f32 = RO.encode(p, frames_to_input(frames), torch.float32)
        return (dict(frames=frames), dict(params=seed),
                dict(features=f64, features32=np.asarray(f32, np.float64), err32=rel_err(f32, f64)))
    raise RuntimeError("no seed satisfies the conditions")


def _save_obs(batch):
    return {f"obs__{k}": v for k, v in batch["obs"].items()}


def sample_case(cfg, shared, sampler, n_steps, B, seed0):
    data = RO.BY_NAME[cfg]
    A = data["shape_meta"]["ac_dim"]
    for seed in range(seed0, seed0 + TRIES):
        batch = RO.synth_image_batch(data, B, OH, seed)
        x_init = rng(seed + 1000).standard_normal((B, T, A)).astype(np.float32)
        seeds = dict(params=seed + 1, encoder=seed + 2, noise=seed + 3)
        p = RO.planner_params(data, seeds["params"], OH)
        enc = RO.encoder_params(data, seeds["encoder"], shared)
        nz = step_noise(seeds["noise"], n_steps, B, A) if sampler == "ddpm" else None
        # the cheap condition first: the encoders alone
        _, logits = RO.obs_cond(data, enc, RO.normalized_obs(data, batch["obs"]), OH, shared, torch.float64, return_logits=True)
        gap = min(RO.tie_gap(v) for v in logits.values())
        if gap <= TIE_TOL:
            print(f"  seed {seed}: tie gap {gap:.2e}, next seed", flush=True)
            continue
        r64 = RO.sample(data, p, enc, batch["obs"], x_init, nz, OH, AH, shared, sampler, n_steps, torch.float64)
        r32 = RO.sample(data, p, enc, batch["obs"], x_init, nz, OH, AH, shared, sampler, n_steps, torch.float32)
        err = float(np.abs(np.asarray(r32["action"], np.float64) - r64["action"]).max())
        if err > ACTION_TOL:
            print(f"  seed {seed}: float32 actions off by {err:.2e}, next seed", flush=True)
            continue
        inp = _save_obs(batch)
        inp["x_init"] = x_init
        return inp, seeds, dict(action=r64["action"], action32=np.asarray(r32["action"], np.float64), cond=r64["cond"], err32=err)
    raise RuntimeError("no seed satisfies the conditions")


def metrics_case(cfg, B, seed0):
    data = RO.BY_NAME[cfg]
    A = data["shape_meta"]["ac_dim"]
    for seed in range(seed0, seed0 + TRIES):
        batch = RO.synth_image_batch(data, B, OH, seed, with_actions=True, T=T)
        g = rng(seed + 1000)
        t = g.integers(0, 100, B)
        noise = g.standard_normal((B, T, A)).astype(np.float32)
        seeds = dict(params=seed + 1, encoder=seed + 2)
        p = RO.planner_params(data, seeds["params"], OH)
        enc = RO.encoder_params(data, seeds["encoder"], False)
        _, logits = RO.obs_cond(data, enc, RO.normalized_obs(data, batch["obs"]), OH, False, torch.float64, return_logits=True)
        gap = min(RO.tie_gap(v) for v in logits.values())
        if gap <= TIE_TOL:
            print(f"  seed {seed}: tie gap {gap:.2e}, next seed", flush=True)
            continue
        r64 = RO.loss(data, p, enc, batch["obs"], batch["actions"], t, noise, OH, False, dtype=torch.float64)
        r32 = RO.loss(data, p, enc, batch["obs"], batch["actions"], t, noise, OH, False, dtype=torch.float32)
        inp = _save_obs(batch)
        inp.update(actions=batch["actions"], t=t.astype(np.float32), noise=noise)
        return inp, seeds, dict(loss=r64["loss"], loss32=r32["loss"], cond=r64["cond"], err32=abs(r32["loss"] - r64["loss"]) / r64["loss"])
    raise RuntimeError("no seed satisfies the conditions")


CASES = {
    "dp_resnet_features_perturbed": (features_case, ("perturbed", 100)),
    "dp_resnet_features_heavy": (features_case, ("heavy", 200)),
    "dp_resnet_sample_rm_img_ddpm100_b3": (sample_case, ("rm_img", False, "ddpm", 100, 3, 300)),
    "dp_resnet_sample_rm_img_ddim50_b2": (sample_case, ("rm_img", False, "ddim", 50, 2, 400)),
    "dp_resnet_sample_rm_img2_ddpm100_b2": (sample_case, ("rm_img2", False, "ddpm", 100, 2, 500)),
    "dp_resnet_sample_rm_img2_shared_ddim50_b2": (sample_case, ("rm_img2", True, "ddim", 50, 2, 600)),
    "dp_resnet_metrics_rm_img_b3": (metrics_case, ("rm_img", 3, 700)),
}


def golden_path(name):
    return os.path.join(ROOT, "tests", "golden", f"{name}.npz")


def main():
    for name in sys.argv[1:] or list(CASES):
        fn, args = CASES[name]
        t0 = time.time()
        inp, seeds, out = fn(*args)
        np.savez_compressed(golden_path(name),
                            **{f"in_{k}": (np.asarray(v) if np.asarray(v).dtype == np.uint8 else np.asarray(v, np.float32))
                               for k, v in inp.items()},
                            **{f"seed_{k}": np.asarray(v, np.int64) for k, v in seeds.items()},
                            **{f"out_{k}": np.asarray(v, np.float64) for k, v in out.items()})
        print(f"{name}: {time.time() - t0:.1f}s, {os.path.getsize(golden_path(name)) / 1024:.0f} KiB, err32 {float(out['err32']):.2e}",
              flush=True)


if __name__ == "__main__":
    main()
