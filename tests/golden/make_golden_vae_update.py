#!/usr/bin/env python3
"""Generates tests/golden/vae_update_*.npz (StableVAEModel.update) from the float64 autograd oracle of tests/vae_train_oracle.py.  Run from
the repo root:

    python tests/golden/make_golden_vae_update.py            # all cases
    python tests/golden/make_golden_vae_update.py NAME ...   # selected cases

A gradient tree of the VAE is 167 MB: the files keep per-leaf digests (tests/util.tree_digest: L2 norm, max |x|, a seeded projection and 64
seeded entries) and regenerate weights and frames from seeds.  Each holds the explicit eps, the step-0 loss metrics, the digests of the step-0
gradients, `err32` (each leaf's max |float32 autograd - float64|, the same chain run in float32: the reference's own error) and the float32
chain's errors of the moments and the reconstruction; the seeded B = 2 case also the parameters and EMA after 1 and 3 steps (train_vae.yaml's
schedule: lr 1e-4, end_lr 1e-6, warmup 1000; ema_decay 0.99) and the metrics of every step.
Fixture conditions (asserted here): every log-variance entry lies at least 1 inside [-30, 20], where the clamp's gradient is continuous; the
projection statistic of every parameter / EMA digest is at least 1e-2 of its leaf's RMS value.  The GPU keeps float32 master parameters (as
the reference does); their storage moves a projection by ~2^-24 of the RMS, i.e. at most 6e-6 of it relative under that condition -- inside
the 1e-4 relative rule for digest statistics.  DIGEST_SEED is the first seed whose projections meet it (seed 0 puts one of 332 at 7e-5 of
the RMS, where float32 rounding alone is 3e-4 relative).
NOTE (parity unpinned): the outputs come from this repository's restatement of the reference algorithm (no JAX here).
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from latent_diffusion_planning_amd import weights as W  # noqa: E402
from tests import vae_model_oracle as VO  # noqa: E402
from tests import vae_train_oracle as VT  # noqa: E402
from tests.util import rng, tree_digest  # noqa: E402

KEY = "agentview_image"
DIGEST_SEED = 3                 # see the fixture conditions above


def raw_frames(seed, B, S=64):
    """(B, 1, S, S, 3) float32 pixel values in [0, 255], as the dataloader yields them."""
    return rng(seed).integers(0, 256, (B, 1, S, S, 3)).astype(np.float32)


def normalised(raw):
    """postprocess_batch with obs_normalization {min: 0, max: 255}, frame 0, rounded to float32 as the device normalises."""
    return (np.asarray(raw, np.float32)[:, 0] / np.float32(255.0) * np.float32(2.0) - np.float32(1.0)).astype(np.float64)


def eps_of(seed, B, lc=4):
    return rng(seed).standard_normal((B, 2, 2, lc)).astype(np.float32)


def params_of(kind, seed):
    return W.init_vae_params(seed=seed) if kind == "seeded" else VO.trained_like_params(seed)[0]


def case(kind, pseed, B, use_kl=True, steps=1):
    seeds = dict(params=pseed, frames=[5100 + 7 * B + i for i in range(steps)], eps=[5200 + 7 * B + i for i in range(steps)])

    def compute():
        p = params_of(kind, pseed)
        data = [(normalised(raw_frames(f, B)), eps_of(e, B)) for f, e in zip(seeds["frames"], seeds["eps"])]
        torch.set_num_threads(16)
        run = VT.train(p, data, use_kl=use_kl)
        frames0, eps0 = data[0]
        m32, g32, mom32, rec32 = VT.loss_and_grads(p, frames0, eps0, use_kl, VT.BETA, torch.float32)
        _, _, mom64, rec64 = VT.loss_and_grads(p, frames0, eps0, use_kl, VT.BETA, torch.float64)
        g64 = run[0]["grads"]
        lc = VO.latent_channels(p)
        for r in run:
            lv = r["moments"][..., lc:]
            assert lv.min() >= -29.0 and lv.max() <= 19.0, f"log-variance [{lv.min()}, {lv.max()}] is within 1 of the clamp"
        out = dict(eps=np.stack([d[1] for d in data]), metrics=np.asarray([[r["metrics"][k] for k in VO.METRIC_KEYS] for r in run]),
                   lr=np.asarray([r["lr"] for r in run]), gdig=tree_digest(g64, DIGEST_SEED),
                   err32=np.asarray([float(np.abs(g32[k] - g64[k]).max()) for k in g64]),
                   mom_err32=float(np.abs(mom32 - mom64).max()), rec_err32=float(np.abs(rec32 - rec64).max()), moments=mom64,
                   metrics32=np.asarray([m32[k] for k in VO.METRIC_KEYS]))
        sizes = np.asarray([np.asarray(v).size for v in g64.values()], np.float64)
        for i in (1, 3):
            if steps >= 3:                          # the several-steps case
                for what, key in (("params", "pdig"), ("ema", "edig")):
                    d = tree_digest(run[i - 1][what], DIGEST_SEED)
                    cond = np.abs(d[:, 2]) / (d[:, 0] / np.sqrt(sizes))
                    assert cond.min() >= 1e-2, f"{key}{i}: a digest projection is {cond.min():.1e} of its leaf's RMS"
                    out[f"{key}{i}"] = d
        lvr = (float(mom64[..., lc:].min()), float(mom64[..., lc:].max()))
        rel = out["err32"] / np.maximum(out["gdig"][:, 1], 1e-300)
        print(f"  logvar range {lvr}; float32 autograd err / leafmax: median {np.median(rel):.2e}, above 1e-4: {(rel > 1e-4).sum()} of "
              f"{len(rel)}, worst {rel.max():.2e} ({list(g64)[int(rel.argmax())]})", flush=True)
        return out
    return dict(seeds, B=B, use_kl=int(use_kl), trained_like=int(kind != "seeded")), compute


CASES = {
    "vae_update_seeded_b2": lambda: case("seeded", 5, 2, steps=3),
    "vae_update_seeded_b33": lambda: case("seeded", 6, 33),
    "vae_update_trained_like_b2": lambda: case("trained_like", 2, 2),
    "vae_update_nokl_b2": lambda: case("seeded", 7, 2, use_kl=False),
}


def golden_path(name):
    return os.path.join(ROOT, "tests", "golden", f"{name}.npz")


def main():
    for name in sys.argv[1:] or list(CASES):
        seeds, compute = CASES[name]()
        t0 = time.time()
        out = compute()
        digs = {k: np.asarray(v, np.float32) for k, v in out.items() if "dig" in k}        # digests in float32: 1e-7 relative, far inside every bound
        rest = {k: np.asarray(v, np.float64) for k, v in out.items() if "dig" not in k}
        np.savez_compressed(golden_path(name), **{f"seed_{k}": np.asarray(v, np.int64) for k, v in seeds.items()},
                            **{f"out_{k}": v for k, v in {**digs, **rest}.items()})
        print(f"{name}: {time.time() - t0:.1f}s, {os.path.getsize(golden_path(name)) / 1024:.0f} KiB", flush=True)


if __name__ == "__main__":
    main()
