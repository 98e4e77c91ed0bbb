"""DPAgent timings on one GPU: ms per `resnet_encode` at 256 frames and per `DPAgent.sample` at 256 rows (one camera, obs_horizon 1,
pred_horizon 16, DDPM-100), frames already on the device, a warm-up call, a host clock around a device synchronise, two runs.  Also
what a sampling call spends before its first denoising step -- the FiLM projection of the condition (dense_kernel with K = G = 1033 and
14336 columns) and the loop's set-up -- as 2 t(DDIM-1) - t(DDIM-2) of the eager loop, and the encoder's share of the `sample` call.

    python tools/dp_agent_bench.py [--iters N] [--rows B]

--train: DPTrainAgent instead -- ms per `update` at B rows (default 256), obs_horizon 2, one camera (512 frames through the encoder),
after a warm-up step, two runs, and the split of one step taken from events around its four parts: encoder forward / U-Net tape (with
the gradient of the condition) / encoder backward / the two Adam + EMA launches.

    python tools/dp_agent_bench.py --train [--iters N] [--rows B]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from latent_diffusion_planning_amd.dp_agent import DPAgent, ENCODER_FIELDS  # noqa: E402

KEY = "agentview_image"
LOW = dict(robot0_eef_pos=3, robot0_eef_quat=4, robot0_gripper_qpos=2)


def _ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def _events_ms(parts, iters):
    """Mean ms of each callable of `parts` (run in order, once per iteration) from events on the current stream."""
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(parts) + 1)] for _ in range(iters)]
    for it in range(iters):
        ev[it][0].record()
        for j, fn in enumerate(parts):
            fn()
            ev[it][j + 1].record()
    torch.cuda.synchronize()
    return [sum(ev[it][j].elapsed_time(ev[it][j + 1]) for it in range(iters)) / iters for j in range(len(parts))]


def train(a):
    from latent_diffusion_planning_amd.dp_train_agent import DPTrainAgent, dp_image_cond_inverse
    from latent_diffusion_planning_amd.dp_agent import dp_image_cond
    B, OH, T = a.rows, 2, 16
    norm = {"obs": {KEY: dict(min=0, max=255), **{k: dict(min=[-1.0] * n, max=[1.0] * n) for k, n in LOW.items()}},
            "actions": dict(clip_min=-1, clip_max=1)}
    meta = dict(ac_dim=7, all_shapes={KEY: [64, 64, 3], **{k: [n] for k, n in LOW.items()}})
    agent = DPTrainAgent.create(0, None, meta, name="dp_agent", planner=dict(down_dims=[256, 512, 1024]), encoder=dict(ENCODER_FIELDS),
                                lowdim_obs=list(LOW), rgb_obs=[KEY], obs_normalization=norm, obs_horizon=OH, pred_horizon=T,
                                action_horizon=8, n_diffusion_steps=100, lr=1e-4, end_lr=1e-6, warmup_steps=500, decay_steps=100000,
                                shared_encoder=False, planner_ema_decay=0.99, encoder_ema_decay=0.99)
    g = np.random.Generator(np.random.PCG64(1))
    obs = {KEY: torch.tensor(g.integers(0, 256, (B, OH, 64, 64, 3)).astype(np.float32)).cuda()}
    obs.update({k: torch.tensor(g.uniform(-1, 1, (B, OH, n)).astype(np.float32)).cuda() for k, n in LOW.items()})
    batch = {"obs": obs, "actions": torch.tensor(g.uniform(-1, 1, (B, T, 7)).astype(np.float32)).cuda()}
    eng = agent._engine
    out = {"rows": B, "frames": B * OH, "iters": a.iters, "cond_width": eng.G}
    state = {"agent": agent, "step": 0}

    def step():
        state["agent"], m = state["agent"].update(batch, state["step"], state["step"])
        state["step"] += 1
        return m
    m = step()                                          # warm-up: arenas, workspaces, launch tables
    out["first_loss"] = float(m["loss"])
    nb = agent._postprocess(batch)
    frames = nb["obs"][KEY][:, :OH].reshape(-1, 64, 64, 3).contiguous()
    low = torch.cat([nb["obs"][k][:, :OH] for k in LOW], dim=-1)
    action = nb["actions"].contiguous()
    eps = torch.randn_like(action)
    t = g.integers(0, 100, B)
    box = {}

    def fwd():
        box["cond"] = dp_image_cond([eng.train_encoder_forward(0, frames)], low)

    def tape():
        box["dcond"] = eng.train_planner_grad_cond(action, eps, t, box["cond"])[1]

    def bwd():
        eng.train_encoder_backward(0, dp_image_cond_inverse(box["dcond"], [OH])[0])

    def apply():
        eng.train_apply("planner", 1e-6)
        eng.train_apply("encoder0", 1e-6)
    for run in (1, 2):
        r = {"update_ms": round(_ms(step, a.iters), 3)}
        parts = _events_ms([fwd, tape, bwd, apply], a.iters)
        for k, v in zip(("encoder_forward_ms", "unet_tape_ms", "encoder_backward_ms", "apply_ms"), parts):
            r[k] = round(v, 3)
        r["unet_tape_share"] = round(parts[1] / sum(parts), 4)
        out[f"run{run}"] = r
    out["last_loss"] = float(step()["loss"])
    out["device_memory_mb"] = round(torch.cuda.mem_get_info()[1] / 2**20 - torch.cuda.mem_get_info()[0] / 2**20, 1)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--train", action="store_true", help="time DPTrainAgent.update instead of sampling")
    a = ap.parse_args()
    if a.train:
        return train(a)
    B = a.rows
    norm = {"obs": {KEY: dict(min=0, max=255), **{k: dict(min=[-1.0] * n, max=[1.0] * n) for k, n in LOW.items()}},
            "actions": dict(clip_min=-1, clip_max=1)}
    meta = dict(ac_dim=7, all_shapes={KEY: [64, 64, 3], **{k: [n] for k, n in LOW.items()}})
    agent = DPAgent.create(0, None, meta, name="dp_agent", planner=dict(down_dims=[256, 512, 1024]), encoder=dict(ENCODER_FIELDS),
                           lowdim_obs=list(LOW), rgb_obs=[KEY], obs_normalization=norm, obs_horizon=1, pred_horizon=16, action_horizon=8,
                           n_diffusion_steps=100, lr=1e-4, end_lr=1e-6, warmup_steps=10, decay_steps=100, shared_encoder=False,
                           planner_ema_decay=0.99, encoder_ema_decay=0.99)
    g = np.random.Generator(np.random.PCG64(1))
    obs = {KEY: torch.tensor(g.integers(0, 256, (B, 1, 64, 64, 3)).astype(np.float32)).cuda()}
    obs.update({k: torch.tensor(g.uniform(-1, 1, (B, 1, n)).astype(np.float32)).cuda() for k, n in LOW.items()})
    batch = {"obs": obs}
    eng = agent._engine
    agent._sync_weights()
    nb = agent._postprocess(batch)
    frames = nb["obs"][KEY].reshape(-1, 64, 64, 3).contiguous()
    cond = agent.get_obs_cond(nb["obs"])
    out = {"rows": B, "iters": a.iters, "cond_width": int(cond.shape[1])}
    for run in (1, 2):
        r = {}
        r["resnet_encode_ms"] = round(_ms(lambda: eng.resnet_encode(0, frames), a.iters), 3)
        r["sample_ms"] = round(_ms(lambda: np.asarray(agent.sample(batch, 1)[0]), a.iters), 3)
        r["plan_sample_ms"] = round(_ms(lambda: eng.plan_sample(cond, seed=1), a.iters), 3)
        t1 = _ms(lambda: eng.plan_sample(cond, seed=1, sampler="ddim", n_steps=1, use_graph=False), a.iters)
        t2 = _ms(lambda: eng.plan_sample(cond, seed=1, sampler="ddim", n_steps=2, use_graph=False), a.iters)
        r["condition_prep_ms"] = round(2 * t1 - t2, 3)
        r["unet_step_ms"] = round(t2 - t1, 3)
        r["encoder_share_of_sample"] = round(r["resnet_encode_ms"] / r["sample_ms"], 4)
        out[f"run{run}"] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
