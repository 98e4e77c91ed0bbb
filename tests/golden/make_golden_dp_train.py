#!/usr/bin/env python3
"""Generates tests/golden/dp_train_update_*.npz (DPTrainAgent.update: the ResNet-18 encoders and the U-Net trained jointly) from the CPU
oracle of tests/dp_train_oracle.py.  Run from the repo root:

    python tests/golden/make_golden_dp_train.py            # all cases
    python tests/golden/make_golden_dp_train.py NAME ...   # selected cases

Each file holds the batch (`in_*`: uint8 frames, raw low-dim observations, actions, t, noise -- the same batch for each of the N_UPDATE
steps), the seeds of the regenerated parameters (`seed_*`), the float64 oracle's first step (`out_loss`, `out_cond`, `out_dcond`, the
gradient digests `out_gdig_<state>`), every step's lr / step metrics, the parameter / EMA digests after 1 and N_UPDATE steps
(`out_pdig<i>_<state>`, `out_edig<i>_<state>`), and the float32 restatement of the first step (`out_loss32`, per-leaf `out_err32_<state>`,
`out_err32_dcond`).  <state> is `planner` or an encoder key.  Trees are stored as tests.util.tree_digest rows cut to their first
DIGEST_SAMPLES sampled entries (a prefix of the 64: the same positions), in float32 -- 1e-7 relative, far inside every bound -- so that
a file with two encoders stays under 450 KiB.

The generator ASSERTS, on the CPU, the conditions the GPU tests rest on, and moves on to the next seed when one fails:
  * no max-pool window of the float64 or of the float32 stem map has a positive maximum attained twice (the backward's tie rule is never
    exercised: a tie at 0 gets no gradient through the ReLU);
  * dp_resnet_oracle.tie_gap > TIE_TOL, as the sampling goldens;
  * |loss32 - loss| <= 1e-5 * loss.
tests/test_dp_train_cpu.py recomputes all three from the stored arrays.
NOTE (parity unpinned): the outputs come from this repository's restatement of the reference algorithm (no JAX here).
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import dp_resnet_oracle as RO  # noqa: E402
from tests import dp_train_oracle as TO  # noqa: E402
from tests.golden.make_golden_dp_resnet import TIE_TOL  # noqa: E402
from tests.util import rng, tree_digest  # noqa: E402

OH, T, AH = 2, 16, 8
N_UPDATE = 3
LOSS_TOL = 1e-5
DIGEST_SAMPLES = 24
SEED_G, SEED_P, SEED_E = 31, 33, 37          # digest seeds: gradients, parameters, EMA
TRIES = 20
MAX_BYTES = 450 * 1024


def digest(tree, seed):
    return tree_digest(tree, seed)[:, :3 + DIGEST_SAMPLES]


def kwargs(cfg, shared):
    return RO.dp_kwargs(RO.BY_NAME[cfg], OH, T, AH, shared_encoder=shared)


def stem_ties(data, enc, obs, shared, dtype):
    nobs = RO.normalized_obs(data, obs)
    n = 0
    for k, x in RO.encoder_inputs(data, nobs, OH, shared).items():
        _, stem, _ = TO.encode_t(TO.leaves_of(enc[k], dtype), torch.as_tensor(np.asarray(x), dtype=dtype), return_maps=True)
        n += TO.pool_ties(stem)
    return n


def conditions(data, p, enc, batch, t, noise, shared):
    """-> (pool ties in float64, in float32, tie gap, loss64, loss32) of a batch: what the generator asserts and the CPU test recomputes."""
    _, logits = RO.obs_cond(data, enc, RO.normalized_obs(data, batch["obs"]), OH, shared, torch.float64, return_logits=True)
    gap = min(RO.tie_gap(v) for v in logits.values())
    l64 = RO.loss(data, p, enc, batch["obs"], batch["actions"], t, noise, OH, shared, dtype=torch.float64)["loss"]
    l32 = RO.loss(data, p, enc, batch["obs"], batch["actions"], t, noise, OH, shared, dtype=torch.float32)["loss"]
    return stem_ties(data, enc, batch["obs"], shared, torch.float64), stem_ties(data, enc, batch["obs"], shared, torch.float32), gap, l64, l32


def update_case(cfg, shared, B, seed0):
    data = RO.BY_NAME[cfg]
    A = data["shape_meta"]["ac_dim"]
    kw = kwargs(cfg, shared)
    for seed in range(seed0, seed0 + TRIES):
        batch = RO.synth_image_batch(data, B, OH, seed, with_actions=True, T=T)
        g = rng(seed + 1000)
        t = g.integers(0, 100, B)
        noise = g.standard_normal((B, T, A)).astype(np.float32)
        seeds = dict(params=seed + 1, encoder=seed + 2)
        p = RO.planner_params(data, seeds["params"], OH)
        enc = RO.encoder_params(data, seeds["encoder"], shared)
        t64, t32, gap, l64, l32 = conditions(data, p, enc, batch, t, noise, shared)
        if t64 or t32 or gap <= TIE_TOL or abs(l32 - l64) > LOSS_TOL * l64:
            print(f"  seed {seed}: pool ties {t64} / {t32}, tie gap {gap:.2e}, loss32 off by {abs(l32 - l64) / l64:.2e}: next seed", flush=True)
            continue
        orc = TO.DPTrainOracle(data, kw, p, enc)
        out = {}
        lr, steps = [], []
        for i in range(N_UPDATE):
            r, m = orc.update(batch["obs"], batch["actions"], t, noise)
            names = ["planner"] + [f"enc_{k}" for k in orc.enc]
            lr.append([m[f"{n}_lr"] for n in names])
            steps.append([m[f"{n}_step"] for n in names])
            if i == 0:
                r32 = TO.loss_and_grads(data, p, enc, batch["obs"], batch["actions"], t, noise, OH, shared, dtype=torch.float32)
                out.update(loss=r["loss"], loss32=r32["loss"], cond=r["cond"].astype(np.float32), dcond=r["dcond"].astype(np.float32),
                           err32_dcond=float(np.abs(r32["dcond"] - r["dcond"]).max()), gdig_planner=digest(r["g_planner"], SEED_G),
                           err32_planner=np.asarray([np.abs(r32["g_planner"][k] - v).max() for k, v in r["g_planner"].items()]))
                for key in orc.enc:
                    out[f"gdig_{key}"] = digest(r["g_enc"][key], SEED_G)
                    out[f"err32_{key}"] = np.asarray([np.abs(r32["g_enc"][key][k] - v).max() for k, v in r["g_enc"][key].items()])
            if i + 1 in (1, N_UPDATE):
                out[f"pdig{i + 1}_planner"], out[f"edig{i + 1}_planner"] = digest(orc.p, SEED_P), digest(orc.p_ema, SEED_E)
                for key in orc.enc:
                    out[f"pdig{i + 1}_{key}"], out[f"edig{i + 1}_{key}"] = digest(orc.enc[key], SEED_P), digest(orc.enc_ema[key], SEED_E)
        out.update(lr=np.asarray(lr, np.float64), steps=np.asarray(steps, np.float64))
        inp = {f"obs__{k}": v for k, v in batch["obs"].items()}
        inp.update(actions=batch["actions"], t=t.astype(np.float32), noise=noise)
        return inp, seeds, out
    raise RuntimeError("no seed satisfies the conditions")


CASES = {
    "dp_train_update_rm_img_b3": ("rm_img", False, 3, 800),
    "dp_train_update_rm_img2_b2": ("rm_img2", False, 2, 820),
    "dp_train_update_rm_img2_shared_b2": ("rm_img2", True, 2, 840),
}


def golden_path(name):
    return os.path.join(ROOT, "tests", "golden", f"{name}.npz")


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for name in sys.argv[1:] or list(CASES):
        t0 = time.time()
        inp, seeds, out = update_case(*CASES[name])
        f32 = lambda k: "dig" in k or k in ("cond", "dcond")
        np.savez_compressed(golden_path(name),
                            **{f"in_{k}": (np.asarray(v) if np.asarray(v).dtype == np.uint8 else np.asarray(v, np.float32)) for k, v in inp.items()},
                            **{f"seed_{k}": np.asarray(v, np.int64) for k, v in seeds.items()},
                            **{f"out_{k}": np.asarray(v, np.float32 if f32(k) else np.float64) for k, v in out.items()})
        size = os.path.getsize(golden_path(name))
        assert size < MAX_BYTES, f"{name}: {size} bytes"
        print(f"{name}: {time.time() - t0:.1f}s, {size / 1024:.0f} KiB, loss {out['loss']:.6f}, loss32 off by "
              f"{abs(out['loss32'] - out['loss']) / out['loss']:.2e}", flush=True)


if __name__ == "__main__":
    main()
