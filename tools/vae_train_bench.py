"""StableVAEModel.update timings on one GPU: ms per `update` at 128 and 256 frames of 64 x 64 (warm, one process), TF/s against the fp32
MFMA peak counting 3 x flops.vae_forward_flops per frame (forward + data gradient + weight gradient, live taps only), the HBM footprint the
training tape allocates (device memory in use after the first step minus before it: the workspace, the column-sum and split-K buffers of
the VAE lane; the four arenas are counted apart), and `get_metrics` on the same batch in the same process as context.

    python tools/vae_train_bench.py [--iters N] [--frames B [B ...]] [--runs R] [--chunk C]

--chunk C times `update(..., chunk=C)`: the batch differentiated C frames at a time into one gradient arena (ldp_train_vae_grad_part); the tape's
footprint is then that of C frames plus the second gradient arena, and `used_gb` (device memory in use after the first step) shows it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from latent_diffusion_planning_amd import flops, weights as W  # noqa: E402
from latent_diffusion_planning_amd.vae_model import StableVAEModel  # noqa: E402

KEY = "agentview_image"


def _used():
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    return total - free


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--frames", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=None)
    a = ap.parse_args()
    fwd = flops.vae_forward_flops(W.VAESpec(), 64)["total"]
    kw = {} if a.chunk is None else {"chunk": a.chunk}
    for B in a.frames:
        model = StableVAEModel.create(0, None, dict(all_shapes={KEY: [64, 64, 3]}), name="stable_vae_model", vae=dict(latent_channels=4),
                                      rgb_obs=[KEY], obs_normalization={"obs": {KEY: dict(min=0, max=255)}}, lr=1e-4, end_lr=1e-6,
                                      warmup_steps=1000, decay_steps=300000, ema_decay=0.99, use_kl=True, beta=1e-5, data_name="bench")
        raw = np.random.Generator(np.random.PCG64(1)).integers(0, 256, (B, 1, 64, 64, 3)).astype(np.float32)
        batch = {"obs": {KEY: torch.tensor(raw).cuda()}}             # frames already on the device: no host copy in the timed region
        out = {"frames": B, "iters": a.iters, "chunk": a.chunk}
        out["get_metrics_ms"] = None
        m0 = _used()
        model._train_sync(model.vae_state)
        m1 = _used()
        model, met = model.update(batch, 0, 0, **kw)                     # first step: launch tables, workspace
        float(met["loss"])
        m2 = _used()
        out["arenas_gb"] = round((m1 - m0) / 1e9, 3)
        out["tape_hbm_gb"] = round((m2 - m1) / 1e9, 3)
        out["used_gb"] = round(m2 / 1e9, 3)
        runs = []
        for r in range(a.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.iters):
                model, met = model.update(batch, i + 1, i + 1, **kw)
            float(met["loss"])
            runs.append((time.perf_counter() - t0) / a.iters * 1e3)
        out["update_ms"] = [round(v, 2) for v in runs]
        best = min(runs)
        out["tflops"] = round(3 * fwd * B / (best * 1e-3) / 1e12, 2)
        out["fraction_of_fp32_mfma_peak"] = round(out["tflops"] / flops.FP32_MFMA_PEAK_TFLOPS, 4)
        model.get_metrics(batch, 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.iters):
            g = model.get_metrics(batch, 1)
        float(g["loss"])
        out["get_metrics_ms"] = round((time.perf_counter() - t0) / a.iters * 1e3, 2)
        print(json.dumps(out), flush=True)
        model._engine.close()
        del model, batch
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
