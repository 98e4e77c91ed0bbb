#!/usr/bin/env python3
"""Generates tests/golden/vae_model_*.npz (StableVAEModel) from the float64 oracle of tests/vae_model_oracle.py.  Run from the repo root:

    python tests/golden/make_golden_vae_model.py            # all cases
    python tests/golden/make_golden_vae_model.py NAME ...   # selected cases

Nothing large is stored as input: parameters come from weights.init_vae_params(seed), raw frames and eps from PCG64 seeds, the latents of
`sample` from the Philox stream; each file holds the seeds (`seed_*`) and the float64 oracle outputs (`out_*`).
Fixture condition (asserted here): the unclamped log-variance of every parity fixture stays inside [-8, 4], so the clamp of the
posterior is not what these cases test (tests/test_hip_vae_model.py tests it on hand-made moments).
NOTE (parity unpinned): the outputs come from this repository's restatement of the reference algorithm (no JAX here).
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from latent_diffusion_planning_amd import weights as W  # noqa: E402
from tests import vae_model_oracle as VO  # noqa: E402
from tests.util import rng  # noqa: E402

KEY, KEY2 = "agentview_image", "robot0_eye_in_hand_image"
PARAMS_SEED, EMA_SEED = 2, 5             # two different weight sets: get_metrics reads `params`, reconstruct / sample `ema_params`
BETA = 1e-5                               # model/stable_vae_model.yaml:20
LOGVAR_RANGE = (-8.0, 4.0)


def raw_frames(seed, B, H=2, S=64):
    """(B, H, S, S, 3) float32 pixel values in [0, 255], as the dataloader yields them."""
    return rng(seed).integers(0, 256, (B, H, S, S, 3)).astype(np.float32)


def normalised(raw):
    """postprocess_batch with obs_normalization {min: 0, max: 255} (utils/data_utils.py:9-16), frame 0."""
    return np.asarray(raw, np.float64)[:, 0] / 255.0 * 2.0 - 1.0


def eps_of(seed, B, lc=4):
    return rng(seed).standard_normal((B, 2, 2, lc)).astype(np.float32)


def params(seed):
    return W.init_vae_params(seed=seed)


def metrics_case(B):
    seeds = dict(params=PARAMS_SEED, frames=4100 + B, eps=4200 + B)

    def compute():
        x = normalised(raw_frames(seeds["frames"], B))
        m, z, rec, mom = VO.loss(params(seeds["params"]), x, eps_of(seeds["eps"], B), True, BETA)
        lv = mom[..., mom.shape[-1] // 2:]
        assert LOGVAR_RANGE[0] <= lv.min() and lv.max() <= LOGVAR_RANGE[1], f"log-variance [{lv.min()}, {lv.max()}] leaves {LOGVAR_RANGE}"
        return dict(metrics=np.asarray([m[k] for k in VO.METRIC_KEYS]), z=z, rec=rec, moments=mom)
    return seeds, compute


def reconstruct_case(B):
    seeds = dict(params=EMA_SEED, frames=4300 + B)

    def compute():
        return dict(rec=VO.reconstruct(params(seeds["params"]), normalised(raw_frames(seeds["frames"], B))))
    return seeds, compute


def sample_latents(seed, lc=4):
    return VO.philox_eps(seed, 4, 2 * 2 * lc, stream=VO.STREAM_VAE_SAMPLE).reshape(4, 2, 2, lc)


def sample_case():
    seeds = dict(params=EMA_SEED, rng=77)

    def compute():
        return dict(img=VO.sample(params(seeds["params"]), sample_latents(seeds["rng"])))
    return seeds, compute


CASES = {
    "vae_model_metrics_b3": (metrics_case, (3,)),
    "vae_model_reconstruct_b2": (reconstruct_case, (2,)),
    "vae_model_sample": (sample_case, ()),
}


def golden_path(name):
    return os.path.join(ROOT, "tests", "golden", f"{name}.npz")


def main():
    for name in sys.argv[1:] or list(CASES):
        fn, args = CASES[name]
        seeds, compute = fn(*args)
        t0 = time.time()
        out = compute()
        np.savez_compressed(golden_path(name), **{f"seed_{k}": np.asarray(v, np.int64) for k, v in seeds.items()},
                            **{f"out_{k}": np.asarray(v, np.float64) for k, v in out.items()})
        print(f"{name}: {time.time() - t0:.1f}s, {os.path.getsize(golden_path(name)) / 1024:.0f} KiB", flush=True)


if __name__ == "__main__":
    main()
