"""Test helper (not a product path): DPVAEAgent's sampling step, loss, gradients, Adam and EMA restated on the oracles of oracle/ --
oracle.torch32.unet_forward / planner_sample (float64), oracle.np64's normalisation, oracle.train's Adam -- imported as they are.

What is restated (agent/dp_repr_agent.py):
  * get_obs_cond (:76-85): [image latents of frames 0..oh-1, low-dim vectors of frames 0..oh-1]
  * loss (:101-133): mean((unet(add_noise(a, noise, t), t, cond) - noise)^2), t and noise explicit
  * update_step (:146-158): adam, then TrainStateEMA.apply_ema: ema = ema * d + p_new * (1 - d)   (utils/flax_utils.py:22-27)
  * sample_step (:169-201): the DDPM / DDIM loop from x_T, then unnormalize(x[:, :action_horizon])
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import torch

from latent_diffusion_planning_amd import weights as W
from oracle import np64, torch32
from oracle import train as OT

F64 = np.float64

# the DP flavour of the two data configurations of tests/cfgs.py: T = 16, obs_horizon 2 (agent/dp_repr_agent.yaml + train_bc.yaml)
DP_KW = dict(name="dp_vae_agent",
             planner=dict(diffusion_step_embed_dim=256, down_dims=[256, 512, 1024], kernel_size=5, n_groups=8, downsample=True),
             n_diffusion_steps=100, lr=1e-4, end_lr=1e-6, warmup_steps=500, decay_steps=100000, random_shift=0, use_ema=False,
             planner_ema_decay=0.99, vae_pretrain_path=None, vae_feature_dim=16)


def dp_kwargs(data, obs_horizon=2, pred_horizon=16, action_horizon=8, **over):
    kw = dict(DP_KW)
    kw.update({k: data[k] for k in ("lowdim_obs", "rgb_obs", "obs_normalization")})
    kw.update(obs_horizon=obs_horizon, pred_horizon=pred_horizon, action_horizon=action_horizon)
    kw.update(over)
    return kw


def spec(data, obs_horizon=2, vae_feature_dim=16):
    lowdim = sum(int(np.prod(data["shape_meta"]["all_shapes"][k])) for k in data["lowdim_obs"])
    E = lowdim + vae_feature_dim * len(data["rgb_obs"])
    return W.PlannerSpec(input_dim=int(data["shape_meta"]["ac_dim"]), global_cond_dim=obs_horizon * E), E


def params(data, seed, obs_horizon=2):
    return W.init_planner_params(spec(data, obs_horizon)[0], seed=seed, perturb=True)


def normalized_obs(data, obs):
    """postprocess_batch on the observation dict (float64 of the reference's float32 arithmetic; the HIP path normalises in float32)."""
    table = data["obs_normalization"]["obs"]
    return {k: np.asarray(np64.apply_norm(np.asarray(v, np.float32), table[k], True), np.float32) for k, v in obs.items()}


def obs_cond(data, nobs, obs_horizon):
    """agent/dp_repr_agent.py:76-85, verbatim in numpy."""
    low = np.concatenate([nobs[k][:, :obs_horizon] for k in data["lowdim_obs"]], axis=-1).astype(np.float32)
    B = low.shape[0]
    low = low.reshape(B, -1)
    img = np.concatenate([nobs[k][:, :obs_horizon] for k in data["rgb_obs"]], axis=1).reshape(B, -1)
    return np.concatenate([img, low], axis=-1)


def sample(data, p, obs, x_init, step_noise, obs_horizon, action_horizon, sampler="ddpm", n_steps=100):
    """sample_step with explicit noise -> (B, action_horizon, A) float64, un-normalised."""
    cond = obs_cond(data, normalized_obs(data, obs), obs_horizon)
    P = torch32.TorchParams(p, dtype=torch.float64)
    x = torch32.planner_sample(P, torch.tensor(cond, dtype=torch.float64), torch.tensor(np.asarray(x_init), dtype=torch.float64),
                               None if step_noise is None else torch.tensor(np.asarray(step_noise), dtype=torch.float64),
                               n_steps=n_steps, sampler=sampler).numpy()
    return np64.apply_norm(x[:, :action_horizon], data["obs_normalization"]["actions"], False)


def loss_and_grads(data, p, obs, actions, t, noise, obs_horizon, n_train=100):
    """jax.grad(loss) (:146-150) in float64 autograd -> dict(loss, grads, g_norm)."""
    cond = torch.tensor(obs_cond(data, normalized_obs(data, obs), obs_horizon), dtype=torch.float64)
    a = np64.apply_norm(np.asarray(actions, np.float32), data["obs_normalization"]["actions"], True).astype(np.float32)
    GP = OT.GradParams(p)
    nz = torch.tensor(np.asarray(noise, F64))
    noisy = OT._add_noise(torch.tensor(a.astype(F64)), nz, t, n_train)
    pred = torch32.unet_forward(GP, noisy, torch.as_tensor(np.asarray(t).reshape(-1)), cond)
    loss = ((pred - nz) ** 2).mean()
    loss.backward()
    g = GP.grads()
    return dict(loss=float(loss.detach()), grads=g, g_norm=float(np.sqrt(sum(float((v ** 2).sum()) for v in g.values()))))


def ema_update(ema, new_params, decay):
    """TrainStateEMA.apply_ema on the parameters AFTER apply_gradients (:154-155)."""
    return OrderedDict((k, np.asarray(ema[k], F64) * decay + np.asarray(new_params[k], F64) * (1.0 - decay)) for k in ema)


def train(data, p0, steps, obs_horizon, decay, lr_schedule):
    """`steps` = [(obs, actions, t, noise)]: adam (oracle.train.adam_apply) then the EMA per step -> (params, ema, losses, g_norms)."""
    p = OrderedDict((k, np.asarray(v, F64)) for k, v in p0.items())
    ema = OrderedDict(p)
    st = OT.adam_init(p)
    losses, norms = [], []
    for obs, actions, t, noise in steps:
        r = loss_and_grads(data, p, obs, actions, t, noise, obs_horizon)
        losses.append(r["loss"])
        norms.append(r["g_norm"])
        p, st = OT.adam_apply(p, r["grads"], st, lr_schedule)
        ema = ema_update(ema, p, decay)
    return p, ema, losses, norms
