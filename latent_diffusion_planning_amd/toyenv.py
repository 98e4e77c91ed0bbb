"""`reach2d`: a device-resident control task (defined by this repository -- the reference evaluates in robosuite and
dm_control, which are simulators on the host).

A point in the square [-1, 1]^2 starts on the left, its goal lies on the right and a blocking disc sits in the middle; the scripted expert
passes the disc on a random side, so its demonstrations are bimodal.  State, dynamics, observations and the scripted policies of N
environments live on the GPU (csrc/env.hip -> libldp_env.so: `ldp_env_reset` / `ldp_env_observe` / `ldp_env_step`); one control cycle is one launch and
nothing crosses to the host between a policy call and the step that executes its actions.  The task is specified operation by operation
in include/ldp_env.h; tests/toyenv_oracle.py restates it in NumPy and the kernels match it bit for bit.

It is a TOY: two degrees of freedom, no contact dynamics, a 16-number "image" that is a fixed polynomial of the state.  What it gives is
the first closed-loop measurement of the planner calls of this package (tools/toy_reach.py, harness.run_device_eval).

The pixel-observed form replaces that polynomial with a camera: `Reach2DPixelEnv` renders the scene to 64 x 64 x 3 uint8
frames on the device (csrc/pix.hip -> libldp_pix.so: `ldp_pix_render`, specified in include/ldp_pix.h, restated in tests/pix_oracle.py) and
shows the goal in the frame only; `collect_pixel_demos` records the expert's frames, `encode_demos` turns them into the StableVAE's latents,
`reach2d_vae_config` / `reach2d_pixel_config` hold the arguments of the VAE and of the agent that plans on them (tools/toy_reach_pixels.py).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _envlib as _lib
from . import _pixlib
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


def _render(pos_ptr: int, pos_stride: int, goal_ptr: int, goal_stride: int, M: int, device) -> torch.Tensor:
    """ONE ldp_pix_render launch on the current stream -> frames (M, 64, 64, 3) uint8."""
    frames = torch.empty((int(M), _pixlib.PIX_SIZE, _pixlib.PIX_SIZE, 3), dtype=torch.uint8, device=device)
    _pixlib.check(_pixlib.load().ldp_pix_render(pos_ptr, pos_stride, goal_ptr, goal_stride, int(M), frames.data_ptr(),
                                                C.c_void_p(torch.cuda.current_stream(device).cuda_stream)))
    return frames


class Reach2DPixelEnv(Reach2DEnv):
    """reach2d seen through a camera: the agent gets its own position as numbers and a 64 x 64 x 3 uint8 frame -- R the
    point, G the goal, B the disc.  The goal is NOT a low-dimensional key: it can be found in the G channel only, as a robot knows its
    proprioception and sees the object.  Dynamics, scripted policies and the success criterion are Reach2DEnv's, untouched."""

    def observe(self) -> dict:
        """-> {'obs': {'pos' (N, 1, 2) float32, 'image' (N, 1, 64, 64, 3) uint8}}: ldp_env_observe for pos and one ldp_pix_render
        straight from the live state (pos = state, goal = state + 2, strides 8)."""
        pos = self._empty(1, 2)
        _lib.check(_lib.load().ldp_env_observe(self.state.data_ptr(), self.n_envs, pos.data_ptr(), None, None, self._stream()))
        p = self.state.data_ptr()
        return {"obs": {"pos": pos, "image": _render(p, _lib.ENV_STATE, p + 8, _lib.ENV_STATE, self.n_envs, self.device).unsqueeze(1)}}

    def goal_observation(self) -> dict:
        """The observation every environment would make AT its goal (p = g): the R blob on the G blob.  The state is not touched: the
        renderer reads the goal's two floats in the place of the point's (pos pointer = state + 2)."""
        g = self.state.data_ptr() + 8
        return {"pos": self.state[:, 2:4].reshape(self.n_envs, 1, 2).clone(),
                "image": _render(g, _lib.ENV_STATE, g, _lib.ENV_STATE, self.n_envs, self.device).unsqueeze(1)}


PIXEL_OBS_KEYS = ("pos", "image")                           # what Reach2DPixelEnv observes and collect_pixel_demos records
LATENT_OBS_KEYS = ("pos", "latent_image")                   # what encode_demos makes of it: the agent's training keys


def _episode_bounds(n: int, device) -> torch.Tensor:
    T = EPISODE_LEN
    start = torch.arange(n, device=device, dtype=torch.int32).repeat_interleave(T) * T
    return torch.stack([start, start + T], dim=1).contiguous()


def collect_pixel_demos(n_episodes: int, seed: int, noise: float = 0.1, episode0: int = 0, device=None, action_dim: int = 2,
                        pred_horizon: int = 0, obs_horizon: int = 1) -> DeviceDataset:
    """collect_demos with a camera: the same expert rollout (ONE ldp_env_step launch that records), then every recorded (pos, goal) row
    rendered by ONE ldp_pix_render launch (stride 2) -> a DeviceDataset with the tables pos (n * 48, 2) float32, image (n * 48, 64, 64, 3)
    uint8 and actions: the StableVAE's training set (12 288 bytes a row; 2048 episodes are 1.2 GB).  The default window is a single frame,
    what StableVAEModel.update reads."""
    env = Reach2DEnv(n_episodes, device, action_dim)
    env.reset(seed, episode0)
    rec = env.step_scripted("expert", noise, n_sub=EPISODE_LEN, record=True)
    n, rows = int(n_episodes), int(n_episodes) * EPISODE_LEN
    pos, goal = rec["pos"].reshape(rows, 2), rec["goal"].reshape(rows, 2)
    tables = dict(pos=pos, image=_render(pos.data_ptr(), 2, goal.data_ptr(), 2, rows, env.device), actions=rec["actions"].reshape(rows, -1))
    bounds = _episode_bounds(n, env.device)
    torch.cuda.current_stream(env.device).synchronize()       # construction: the tables are complete before any stream samples them
    return DeviceDataset(tables, bounds, PIXEL_OBS_KEYS, ("actions",), obs_horizon, pred_horizon + 1, [0], [rows], [1.0], n,
                         env_meta=dict(env_name="reach2d_pixels", seed=int(seed), noise=float(noise), episode0=int(episode0)))


def encode_frames(frames: torch.Tensor, agent_or_engine, chunk: int = 256) -> torch.Tensor:
    """frames (n, 64, 64, 3) uint8 on the device -> the StableVAE's raw latent means (n, 16), `chunk` frames per encode call.  The bytes are
    normalised as preencode does, (x / 255 - 0.5) / 0.5, by the engine's own kernel; an agent's VAE weights are uploaded first, an engine
    is taken as loaded.  Every chunk goes through the range guard of the fp16-plane convs (vae_encode_checked)."""
    if int(chunk) < 1:
        raise ValueError(f"chunk must be >= 1, got {chunk}")
    eng = agent_or_engine
    if hasattr(agent_or_engine, "_sync_weights"):
        agent_or_engine._sync_weights(need_vae=True)
        eng = agent_or_engine._engine
    out = []
    for i in range(0, frames.shape[0], int(chunk)):
        x = eng.normalize_bounds(frames[i:i + int(chunk)], [0.0], [255.0], True)
        out.append(eng.vae_encode_checked(x).reshape(x.shape[0], -1))
    return torch.cat(out, dim=0)


def encode_demos(dataset: DeviceDataset, agent_or_engine, chunk: int = 256, pred_horizon: int = 8, obs_horizon: int = 1):
    """The device counterpart of preencode.encode_hdf5: the `image` table of a collect_pixel_demos dataset through the agent's own
    StableVAE encoder (encode_frames) -> (DeviceDataset with the tables pos, latent_image (raw latent means, 16 a row) and actions, windowed
    for LDPAgent.update; (lo, hi): the per-component min and max of the latents as float32 arrays (16,), for `obs_normalization` -- the
    reference takes these bounds from the dataset too)."""
    z = encode_frames(dataset.tables["image"], agent_or_engine, chunk).contiguous()
    tables = dict(pos=dataset.tables["pos"], latent_image=z, actions=dataset.tables["actions"])
    lo, hi = z.min(dim=0).values.cpu().numpy(), z.max(dim=0).values.cpu().numpy()
    ds = DeviceDataset(tables, dataset.bounds, LATENT_OBS_KEYS, ("actions",), obs_horizon, pred_horizon + 1, dataset.set_base, dataset.set_total,
                       dataset.split, dataset.n_demos, env_meta=dataset.env_meta)
    return ds, (lo, hi)


def with_latent_bounds(agent, latent_bounds):
    """The agent with `latent_image` normalised from latent_bounds = (lo, hi) of encode_demos: the same engine and weights (LDPAgent.replace),
    so the agent that encoded the demonstrations goes on to train on them."""
    from .agent import _norm_entry
    lo, hi = latent_bounds
    norm = dict(agent.obs_normalization)
    norm["obs"] = dict(norm["obs"], latent_image=_norm_entry(dict(min=lo, max=hi)))
    return agent.replace(obs_normalization=norm)


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


def reach2d_vae_config(lr: float = 1e-4, end_lr: float = 1e-6, warmup_steps: int = 100, decay_steps: int = 2000, ema_decay: float = 0.99,
                       use_kl: bool = True, beta: float = 1e-5, **overrides) -> dict:
    """-> dict(shape_meta=..., vae_kwargs=...): `StableVAEModel.create(rng, None, cfg['shape_meta'], **cfg['vae_kwargs'])` is the VAE of
    the pixel task -- one 64 x 64 x 3 camera `image`, bytes normalised from (0, 255), four latent channels (a 2 x 2 x 4 = 16-number latent)."""
    shape_meta = dict(ac_dim=2, all_shapes={"pos": [2], "image": [_pixlib.PIX_SIZE, _pixlib.PIX_SIZE, 3]}, use_images=True)
    norm = dict(obs=dict(image=dict(min=0.0, max=255.0), pos=dict(min=-1.0, max=1.0)), actions=dict(min=-1.0, max=1.0))
    kw = dict(name="stable_vae_model", vae=dict(latent_channels=4), rgb_obs=["image"], obs_normalization=norm, lr=lr, end_lr=end_lr,
              warmup_steps=int(warmup_steps), decay_steps=int(decay_steps), ema_decay=ema_decay, use_kl=use_kl, beta=beta, data_name="reach2d_pixels")
    kw.update(overrides)
    return dict(shape_meta=shape_meta, vae_kwargs=kw)


def reach2d_pixel_config(latent_bounds=None, **kwargs) -> dict:
    """reach2d_config for the pixel task: `LDPAgent.create(rng, None, cfg['shape_meta'], vae_params=..., **cfg['agent_kwargs'])` plans on the
    StableVAE latent of the camera frame.  lowdim_obs is pos alone -- the goal is in the frame only -- so obs_dim is 16 + 2 = 18.
    latent_bounds: (lo, hi) of encode_demos (scalars or 16 numbers each; default the unit map) for `latent_image`; `image` is normalised
    from (0, 255) and `pos` by the unit map.  Other arguments as reach2d_config."""
    cfg = reach2d_config(**kwargs)
    lo, hi = (-1.0, 1.0) if latent_bounds is None else latent_bounds
    unit = dict(min=-1.0, max=1.0)
    shape_meta = dict(ac_dim=cfg["shape_meta"]["ac_dim"], use_images=True,
                      all_shapes={"pos": [2], "image": [_pixlib.PIX_SIZE, _pixlib.PIX_SIZE, 3], "latent_image": [_lib.ENV_LATENT]})
    norm = dict(obs=dict(image=dict(min=0.0, max=255.0), pos=dict(unit), latent_image=dict(min=lo, max=hi)), actions=dict(unit))
    kw = dict(cfg["agent_kwargs"])
    if "lowdim_obs" not in kwargs:
        kw["lowdim_obs"] = ["pos"]
    if "obs_normalization" not in kwargs:
        kw["obs_normalization"] = norm
    if "data_name" not in kwargs:
        kw["data_name"] = "reach2d_pixels"
    return dict(shape_meta=shape_meta, obs_normalization=kw["obs_normalization"], agent_kwargs=kw)
