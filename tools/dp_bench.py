"""DPVAEAgent timings on one GPU: ms per `sample` (DDPM-100, captured graph) at 5 and 256 rows, ms per `update` at 256 rows.
Latent batches (no StableVAE encode), rm_lift shapes, obs_horizon 2, pred_horizon 16, action_horizon 8.

    python tools/dp_bench.py [--iters N]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from latent_diffusion_planning_amd import weights as W  # noqa: E402
from latent_diffusion_planning_amd.dp_vae_agent import DPVAEAgent  # noqa: E402
from tests import cfgs, dp_oracle  # noqa: E402


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
    a = ap.parse_args()
    data = cfgs.BY_NAME["rm"]
    ag = DPVAEAgent.create(0, None, data["shape_meta"], **dp_oracle.dp_kwargs(data, 2, 16, 8))
    n_params = sum(int(np.prod(s)) for s in W.planner_shapes(ag._planner_spec).values())
    out = {"unet_params": n_params}
    for B in (5, 256):
        batch = {"obs": cfgs.synth_latent_batch(data, B, 2, B)["obs"]}
        out[f"sample_ms_b{B}_ddpm100"] = round(_ms(lambda: np.asarray(ag.sample(batch, 1)[0]), a.iters), 3)
    b = cfgs.synth_latent_batch(data, 256, 2, 7)
    b["actions"] = np.random.Generator(np.random.PCG64(8)).uniform(-1, 1, (256, 16, 7)).astype(np.float32)
    state = {"ag": ag, "i": 0}

    def step():
        state["ag"], _ = state["ag"].update(b, state["i"], state["i"])
        state["i"] += 1
    out["update_ms_b256"] = round(_ms(step, a.iters), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
