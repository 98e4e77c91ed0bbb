"""StableVAEModel timings on one GPU: ms per `get_metrics` and per `reconstruct` at 256 frames of 64 x 64, and -- in the same process --
ms of `vae_encode` + `vae_decode` alone on the same frames, so that what the loss head (moments' second half, posterior, loss / statistics
reductions, the final merge) and the model's own pre-processing cost on top of the two networks can be read off.

    python tools/vae_model_bench.py [--iters N] [--frames B]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from latent_diffusion_planning_amd.vae_model import StableVAEModel  # noqa: E402

KEY = "agentview_image"


def _ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, default=256)
    a = ap.parse_args()
    B = a.frames
    model = StableVAEModel.create(0, None, dict(all_shapes={KEY: [64, 64, 3]}), name="stable_vae_model", vae=dict(latent_channels=4),
                                  rgb_obs=[KEY], obs_normalization={"obs": {KEY: dict(min=0, max=255)}}, lr=1e-4, end_lr=1e-6,
                                  warmup_steps=10, decay_steps=100, ema_decay=0.99, use_kl=True, beta=1e-5, data_name="bench")
    raw = np.random.Generator(np.random.PCG64(1)).integers(0, 256, (B, 1, 64, 64, 3)).astype(np.float32)
    batch = {"obs": {KEY: torch.tensor(raw).cuda()}}                 # frames already on the device: no host copy in the timed region
    eng = model._engine
    out = {"frames": B, "iters": a.iters}
    out["get_metrics_ms"] = round(_ms(lambda: float(model.get_metrics(batch, 1)["loss"]), a.iters), 3)
    img = model._frames(batch, [KEY])
    out["vae_metrics_call_ms"] = round(_ms(lambda: eng.vae_metrics(img, True, 1e-5, seed=1), a.iters), 3)
    out["encode_plus_decode_ms"] = round(_ms(lambda: eng.vae_decode(eng.vae_encode(img)), a.iters), 3)
    out["encode_ms"] = round(_ms(lambda: eng.vae_encode(img), a.iters), 3)
    out["loss_head_ms"] = round(out["vae_metrics_call_ms"] - out["encode_plus_decode_ms"], 3)
    out["reconstruct_ms"] = round(_ms(lambda: np.asarray(model.reconstruct(batch, 1, KEY)), a.iters), 3)   # (the 12.6 MB result is read back)
    out["uploads"] = model.uploads
    print(json.dumps(out))


if __name__ == "__main__":
    main()
