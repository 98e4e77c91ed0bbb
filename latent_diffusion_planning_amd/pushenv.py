"""`push2d`: a device-resident pushing task (defined by this repository, like `reach2d` of toyenv.py).

A point in the square [-1, 1]^2 pushes a disc to a goal.  The goal lies on the left or on the right; the point starts on the left, so in
half of the episodes it starts on the wrong side of the disc and has to go round it before it can push.  Contact is a projection along the
contact normal, so an oblique push sends the disc sideways: a plan can be wrong in more than one way.  State, dynamics, observations and the
scripted policies of N environments live on the GPU (csrc/push.hip -> libldp_push.so: `ldp_push_reset` / `ldp_push_observe` /
`ldp_push_step`); one control cycle is one launch and nothing crosses to the host between a policy call and the step that executes its
actions.  The task is specified operation by operation in include/ldp_push.h; tests/pushenv_oracle.py restates it in NumPy and the
kernels match it bit for bit.

Still a TOY: two degrees of freedom, a frictionless disc, a 16-number "image" that is a fixed polynomial of the state.  The disc's position
is in that latent only; `pos` and `goal` are the low-dimensional keys, as in reach2d, so the agent of `push2d_config` has reach2d's shapes.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _pushlib as _lib
from .data import DeviceDataset
from .toyenv import OBS_KEYS, reach2d_config

EPISODE_LEN = _lib.PUSH_EPISODE_LEN
OBS_DIMS = {"pos": 2, "goal": 2, "latent_image": _lib.PUSH_LATENT}
_FIRST, _BLOCKED, _PUSHED = 8, 9, 10                        # columns of the state (include/ldp_push.h)


class Push2DEnv:
    """n_envs push2d environments in lockstep on one device, with the interface of toyenv.Reach2DEnv.  Environment i of a
    reset(seed, episode0) is the global episode episode0 + i: its start, disc, goal, side and the scripted policies' noise do not depend on
    how episodes are split over objects or calls.  Every method enqueues one launch on the current stream and returns device tensors;
    none synchronises."""
    episode_len = EPISODE_LEN

    def __init__(self, n_envs: int, device=None, action_dim: int = 2):
        if int(n_envs) < 1:
            raise ValueError(f"n_envs must be >= 1, got {n_envs}")
        if int(action_dim) < 2:
            raise ValueError(f"action_dim must be >= 2 (the task reads two action components), got {action_dim}")
        self.n_envs, self.action_dim = int(n_envs), int(action_dim)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.state = torch.zeros((self.n_envs, _lib.PUSH_STATE), dtype=torch.float32, device=self.device)
        self.seed = self.episode0 = 0

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _empty(self, frames, width):
        return torch.empty((self.n_envs, frames, width), dtype=torch.float32, device=self.device)

    def reset(self, seed: int, episode0: int = 0) -> None:
        self.seed, self.episode0 = int(seed) & (2**64 - 1), int(episode0)
        _lib.check(_lib.load().ldp_push_reset(self.state.data_ptr(), self.n_envs, C.c_uint64(self.seed), C.c_int64(self.episode0), self._stream()))

    def observe(self) -> dict:
        """-> {'obs': {'pos' (N, 1, 2), 'goal' (N, 1, 2), 'latent_image' (N, 1, 16)}}: what a DeviceDataset batch looks like at
        obs_horizon 1, ready for LDPAgent.sample and its relatives."""
        pos, goal, lat = self._empty(1, 2), self._empty(1, 2), self._empty(1, _lib.PUSH_LATENT)
        _lib.check(_lib.load().ldp_push_observe(self.state.data_ptr(), self.n_envs, pos.data_ptr(), goal.data_ptr(), lat.data_ptr(), self._stream()))
        return {"obs": {"pos": pos, "goal": goal, "latent_image": lat}}

    def _step(self, n_sub, actions, A, policy, noise, seed, record):
        out = dict(actions=self._empty(n_sub, A), pos=self._empty(n_sub, 2), goal=self._empty(n_sub, 2),
                   latent_image=self._empty(n_sub, _lib.PUSH_LATENT)) if record else None
        ptr = (lambda k: out[k].data_ptr()) if record else (lambda k: None)
        _lib.check(_lib.load().ldp_push_step(self.state.data_ptr(), self.n_envs, int(n_sub), None if actions is None else actions.data_ptr(), int(A),
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
        if policy not in _lib.PUSH_POLICIES:
            raise ValueError(f"policy must be one of {sorted(_lib.PUSH_POLICIES)}, got {policy!r}")
        return self._step(n_sub, None, self.action_dim, _lib.PUSH_POLICIES[policy], noise, self.seed if seed is None else seed, record)

    def first_success(self) -> torch.Tensor:
        """(N,) int32: the step at which each episode's disc first reached its goal, 0 while it has not."""
        return self.state[:, _FIRST].to(torch.int32)

    def success(self) -> torch.Tensor:
        return self.state[:, _FIRST] != 0

    def blocked(self) -> torch.Tensor:
        """(N,) int32: moves refused so far (a push that would take the disc out of its square)."""
        return self.state[:, _BLOCKED].to(torch.int32)

    def pushed(self) -> torch.Tensor:
        """(N,) int32: moves that moved the disc so far."""
        return self.state[:, _PUSHED].to(torch.int32)

    def goal_side(self) -> torch.Tensor:
        """(N,) bool: the goal lies on the left (the point starts on the wrong side of the disc)."""
        return self.state[:, 4] < 0


def collect_push_demos(n_episodes: int, seed: int, noise: float = 0.1, episode0: int = 0, policy: str = "expert", device=None,
                       action_dim: int = 2, pred_horizon: int = 8, obs_horizon: int = 1) -> DeviceDataset:
    """Roll `policy` out for n_episodes whole episodes (ONE launch) and weld what it saw and did into a DeviceDataset, on the device:
    EPISODE_LEN rows per episode, row t = (the observation in front of step t, the action taken at step t).  policy='random' (or
    'straight') is how suboptimal data is made.  Windows are obs_horizon + pred_horizon observations and pred_horizon + 1 actions: what
    LDPAgent.update reads."""
    env = Push2DEnv(n_episodes, device, action_dim)
    env.reset(seed, episode0)
    rec = env.step_scripted(policy, noise, n_sub=EPISODE_LEN, record=True)
    T, n = EPISODE_LEN, int(n_episodes)
    tables = {k: v.reshape(n * T, v.shape[-1]) for k, v in rec.items()}
    start = torch.arange(n, device=env.device, dtype=torch.int32).repeat_interleave(T) * T
    bounds = torch.stack([start, start + T], dim=1).contiguous()
    torch.cuda.current_stream(env.device).synchronize()       # construction: the tables are complete before any stream samples them
    return DeviceDataset(tables, bounds, OBS_KEYS, ("actions",), obs_horizon, pred_horizon + 1, [0], [n * T], [1.0], n,
                         env_meta=dict(env_name="push2d", seed=int(seed), noise=float(noise), episode0=int(episode0), policy=str(policy)))


def without_actions(dataset: DeviceDataset) -> DeviceDataset:
    """The same demonstrations as action-free data: every table shared but `actions`, which is all zeros.  What the planner's side of
    LDPAgent.update_mixed is trained on when only the IDM's data carries labels."""
    tables = dict(dataset.tables, actions=torch.zeros_like(dataset.tables["actions"]))
    if dataset.device.type == "cuda":                         # construction: the table is complete before any stream samples it
        torch.cuda.current_stream(dataset.device).synchronize()
    return DeviceDataset(tables, dataset.bounds, dataset.obs_keys, dataset.dataset_keys, dataset.frame_stack, dataset.seq_length, dataset.set_base,
                         dataset.set_total, dataset.split, dataset.n_demos, env_meta=dict(dataset.env_meta or {}, action_free=True))


def push2d_config(**kw) -> dict:
    """reach2d_config for push2d: the same networks and shapes (obs_dim 20: pos, goal and the 16-number latent, every bound (-1, 1)),
    `data_name="push2d"`.  Arguments as reach2d_config."""
    kw.setdefault("data_name", "push2d")
    return reach2d_config(**kw)
