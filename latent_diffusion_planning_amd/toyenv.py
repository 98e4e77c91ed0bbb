"""`reach2d`: a device-resident control task (defined by this repository -- the reference evaluates in robosuite and
dm_control, which are simulators on the host).

A point in the square [-1, 1]^2 starts on the left, its goal lies on the right and a blocking disc sits in the middle; the scripted expert
passes the disc on a random side, so its demonstrations are bimodal.  State, dynamics, observations and the scripted policies of N
environments live on the GPU (csrc/env.hip -> libldp_env.so: `ldp_env_reset` / `ldp_env_observe` / `ldp_env_step`); one control cycle is one launch and
nothing crosses to the host between a policy call and the step that executes its actions.  The task is specified operation by operation
in include/ldp_env.h; tests/toyenv_oracle.py restates it in NumPy and the kernels match it bit for bit.

It is a TOY: two degrees of freedom, no contact dynamics, a 16-number "image" that is a fixed polynomial of the state.  What it gives is
the first closed-loop measurement of the planner calls of this package (tools/toy_reach.py, harness.run_device_eval).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _envlib as _lib
from .data import DeviceDataset

EPISODE_LEN = _lib.ENV_EPISODE_LEN
OBS_KEYS = ("pos", "goal", "latent_image")                  # lowdim, lowdim, rgb (a `latent_` key passes vae_encode untouched: no VAE)
OBS_DIMS = {"pos": 2, "goal": 2, "latent_image": _lib.ENV_LATENT}


class Reach2DEnv:
    """n_envs reach2d environments in lockstep on one device.  Environment i of a reset(seed, episode0) is the global episode
    episode0 + i: its start, goal, side and the scripted policies' noise do not depend on how episodes are split over objects or calls.
    Every method enqueues one launch on the current stream and returns device tensors; none synchronises."""
    episode_len = EPISODE_LEN

    def __init__(self, n_envs: int, device=None, action_dim: int = 2):
        if int(n_envs) < 1:
            raise ValueError(f"n_envs must be >= 1, got {n_envs}")
        if int(action_dim) < 2:
            raise ValueError(f"action_dim must be >= 2 (the task reads two action components), got {action_dim}")
        self.n_envs, self.action_dim = int(n_envs), int(action_dim)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.state = torch.zeros((self.n_envs, _lib.ENV_STATE), dtype=torch.float32, device=self.device)
        self.seed = self.episode0 = 0

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _empty(self, frames, width):
        return torch.empty((self.n_envs, frames, width), dtype=torch.float32, device=self.device)

    def reset(self, seed: int, episode0: int = 0) -> None:
        self.seed, self.episode0 = int(seed) & (2**64 - 1), int(episode0)
        _lib.check(_lib.load().ldp_env_reset(self.state.data_ptr(), self.n_envs, C.c_uint64(self.seed), C.c_int64(self.episode0), self._stream()))

    def observe(self) -> dict:
        """-> {'obs': {'pos' (N, 1, 2), 'goal' (N, 1, 2), 'latent_image' (N, 1, 16)}}: what a DeviceDataset batch looks like at
        obs_horizon 1, ready for LDPAgent.sample and its relatives."""
        pos, goal, lat = self._empty(1, 2), self._empty(1, 2), self._empty(1, _lib.ENV_LATENT)
        _lib.check(_lib.load().ldp_env_observe(self.state.data_ptr(), self.n_envs, pos.data_ptr(), goal.data_ptr(), lat.data_ptr(), self._stream()))
        return {"obs": {"pos": pos, "goal": goal, "latent_image": lat}}

    def goal_observation(self) -> dict:
        """The observation every environment would make AT its goal (p = g), as an observation dict (N, 1, .) per key: what
        `goal=` of sample_best_of / build_guide / plan embeds.  Two device copies and one launch; the state is not touched."""
        at_goal = self.state.clone()
        at_goal[:, 0:2] = self.state[:, 2:4]
        pos, goal, lat = self._empty(1, 2), self._empty(1, 2), self._empty(1, _lib.ENV_LATENT)
        _lib.check(_lib.load().ldp_env_observe(at_goal.data_ptr(), self.n_envs, pos.data_ptr(), goal.data_ptr(), lat.data_ptr(), self._stream()))
        return {"pos": pos, "goal": goal, "latent_image": lat}

    def _step(self, n_sub, actions, A, policy, noise, seed, record):
        out = dict(actions=self._empty(n_sub, A), pos=self._empty(n_sub, 2), goal=self._empty(n_sub, 2),
                   latent_image=self._empty(n_sub, _lib.ENV_LATENT)) if record else None
        ptr = (lambda k: out[k].data_ptr()) if record else (lambda k: None)
        _lib.check(_lib.load().ldp_env_step(self.state.data_ptr(), self.n_envs, int(n_sub), None if actions is None else actions.data_ptr(), int(A),
                                            int(policy), C.c_float(float(noise)), C.c_uint64(int(seed) & (2**64 - 1)), C.c_int64(self.episode0),
                                            ptr("actions"), ptr("pos"), ptr("goal"), ptr("latent_image"), self._stream()))
        return out

    def step(self, actions, record: bool = False) -> Optional[dict]:
        """Execute actions (N, n_sub, A): a device tensor (a DeviceArray's `.tensor`), taken as it is -- no host copy.  record=True ->
        {'actions' (N, n_sub, A) as taken, 'pos', 'goal', 'latent_image' (N, n_sub, .): the observation in front of every sub-step}."""
        a = getattr(actions, "tensor", actions)
        if not isinstance(a, torch.Tensor) or a.device != self.device:
            raise ValueError(f"actions must be a tensor on {self.device}")
        if a.dim() != 3 or a.shape[0] != self.n_envs or a.shape[1] < 1 or a.shape[2] < 2:
            raise ValueError(f"actions must have shape ({self.n_envs}, n_sub >= 1, A >= 2), got {tuple(a.shape)}")
        a = a.to(torch.float32).contiguous()
        return self._step(a.shape[1], a, a.shape[2], 0, 0.0, 0, record)

    def step_scripted(self, policy: str, noise: float = 0.0, seed: Optional[int] = None, n_sub: int = 1, record: bool = False) -> Optional[dict]:
        """n_sub sub-steps under a scripted policy ('expert', 'straight', 'random'); seed: of the policy's noise (default: the reset's)."""
        if policy not in _lib.ENV_POLICIES:
            raise ValueError(f"policy must be one of {sorted(_lib.ENV_POLICIES)}, got {policy!r}")
        return self._step(n_sub, None, self.action_dim, _lib.ENV_POLICIES[policy], noise, self.seed if seed is None else seed, record)

    def first_success(self) -> torch.Tensor:
        """(N,) int32: the step at which each episode first reached its goal, 0 while it has not."""
        return self.state[:, 6].to(torch.int32)

    def success(self) -> torch.Tensor:
        return self.state[:, 6] != 0

    def blocked(self) -> torch.Tensor:
        """(N,) int32: moves the disc refused so far."""
        return self.state[:, 7].to(torch.int32)


def collect_demos(n_episodes: int, seed: int, noise: float = 0.1, episode0: int = 0, device=None, action_dim: int = 2, pred_horizon: int = 8,
                  obs_horizon: int = 1) -> DeviceDataset:
    """Roll the expert out for n_episodes whole episodes (ONE launch) and weld what it saw and did into a DeviceDataset, on the device:
    EPISODE_LEN rows per episode, row t = (the observation in front of step t, the action taken at step t).  Windows are
    obs_horizon + pred_horizon observations and pred_horizon + 1 actions: what LDPAgent.update reads."""
    env = Reach2DEnv(n_episodes, device, action_dim)
    env.reset(seed, episode0)
    rec = env.step_scripted("expert", noise, n_sub=EPISODE_LEN, record=True)
    T, n = EPISODE_LEN, int(n_episodes)
    tables = {k: v.reshape(n * T, v.shape[-1]) for k, v in rec.items()}
    start = torch.arange(n, device=env.device, dtype=torch.int32).repeat_interleave(T) * T
    bounds = torch.stack([start, start + T], dim=1).contiguous()
    torch.cuda.current_stream(env.device).synchronize()       # construction: the tables are complete before any stream samples them
    return DeviceDataset(tables, bounds, OBS_KEYS, ("actions",), obs_horizon, pred_horizon + 1, [0], [n * T], [1.0], n,
                         env_meta=dict(env_name="reach2d", seed=int(seed), noise=float(noise), episode0=int(episode0)))


def reach2d_config(action_dim: int = 2, pred_horizon: int = 8, action_horizon: int = 4, planner_n_diffusion_steps: int = 100,
                   idm_n_diffusion_steps: int = 100, lr: float = 1e-4, end_lr: float = 1e-6, warmup_steps: int = 500,
                   decay_steps: int = 20000, **overrides) -> dict:
    """-> dict(shape_meta=..., obs_normalization=..., agent_kwargs=...): `LDPAgent.create(rng, None, cfg['shape_meta'],
    **cfg['agent_kwargs'])` is the agent of the task -- obs_horizon 1, the 16 Chebyshev features in the place of the VAE latent (no VAE),
    pos and goal as low-dim keys, obs_dim 20, every normalisation bound (-1, 1) (the identity map)."""
    unit = dict(min=-1.0, max=1.0)
    shape_meta = dict(ac_dim=int(action_dim), all_shapes={k: [d] for k, d in OBS_DIMS.items()}, use_images=False)
    norm = dict(obs={k: dict(unit) for k in OBS_KEYS}, actions=dict(unit))
    kw = dict(name="ldp_agent",
              planner=dict(diffusion_step_embed_dim=256, down_dims=[256, 512, 1024], kernel_size=5, n_groups=8, downsample=True),
              idm_net=dict(n_blocks=3, dropout_rate=None, use_layer_norm=True, hidden_dim=256),
              preprocess_time=dict(output_size=256, learnable=False),
              cond_encoder=dict(hidden_dims=[256, 256], activations="mish", activate_final=False),
              vae_pretrain_path=None, vae_feature_dim=_lib.ENV_LATENT, use_planner=True, use_idm=True,
              lowdim_obs=["pos", "goal"], rgb_obs=["latent_image"], obs_normalization=norm, data_name="reach2d",
              obs_horizon=1, pred_horizon=int(pred_horizon), action_horizon=int(action_horizon),
              planner_n_diffusion_steps=int(planner_n_diffusion_steps), idm_n_diffusion_steps=int(idm_n_diffusion_steps),
              lr=lr, end_lr=end_lr, idm_lr=lr, idm_end_lr=end_lr, warmup_steps=int(warmup_steps), decay_steps=int(decay_steps), grad_clip=100)
    kw.update(overrides)
    return dict(shape_meta=shape_meta, obs_normalization=norm, agent_kwargs=kw)
