"""Constrained planning: the host side of LDPAgent.sample_constrained -- the level coefficients and the assembly of a
caller's goals and waypoints into the (target, mask) pair the engine inpaints in its loop.  No kernel of its own: csrc/constrain.hip
does the work, through HipEngine.plan_constrain / plan_sample_constrained / agent_sample_constrained."""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np

from . import schedule

MODES = ("clamp", "repaint")


def level_timestep(level: int, n_train: int, n_steps: int) -> int:
    """The training timestep of level j < n_steps, the state in front of executed step j: (n_steps - 1 - j) * (n_train // n_steps) for
    both samplers (DDPM has n_steps == n_train)."""
    if n_steps <= 0 or n_train % n_steps != 0:
        raise ValueError(f"n_steps {n_steps} must divide the {n_train} training steps")
    if not 0 <= int(level) < n_steps:
        raise ValueError(f"level {level} has no timestep: levels 0..n_steps-1 = {n_steps - 1} do (level n_steps is the result)")
    return (n_steps - 1 - int(level)) * (n_train // n_steps)


def level_coefs(n_train: int, n_steps: int) -> np.ndarray:
    """(n_steps + 1, 2) float32: row j = (a_j, s_j) = (sqrt(abar_t_j), sqrt(1 - abar_t_j)), evaluated in float64 from the float32 abar
    table and cast to float32 (the warm start's convention, csrc/replan.hip warm_coefs); row n_steps is exactly (1, 0)."""
    acp = schedule.make_schedule(n_train).alphas_cumprod
    out = np.empty((n_steps + 1, 2), np.float32)
    for j in range(n_steps):
        a_t = float(np.float32(acp[level_timestep(j, n_train, n_steps)]))
        out[j] = (math.sqrt(a_t), math.sqrt(1.0 - a_t))
    out[n_steps] = (1.0, 0.0)
    return out


def table_level_coefs(n_train: int, timesteps) -> np.ndarray:
    """level_coefs over a timestep table (sampler "dpmpp", csrc/constrain.hip table_level_coefs): (n + 1, 2) float32 for the n entries of
    `timesteps` (first executed step first): row j < n = (sqrt(abar_ts[j]), sqrt(1 - abar_ts[j])), float64 from the float32 abar table and
    cast once; row n is exactly (1, 0)."""
    ts = [int(t) for t in np.asarray(timesteps).reshape(-1)]
    if any(not 0 <= t < n_train for t in ts):
        raise ValueError(f"timesteps must lie in 0..{n_train - 1}, got {ts}")
    acp = schedule.make_schedule(n_train).alphas_cumprod
    out = np.empty((len(ts) + 1, 2), np.float32)
    for j, t in enumerate(ts):
        a_t = float(np.float32(acp[t]))
        out[j] = (math.sqrt(a_t), math.sqrt(1.0 - a_t))
    out[len(ts)] = (1.0, 0.0)
    return out


def _is_torch(a) -> bool:
    return type(a).__module__.split(".")[0] == "torch"


def _host(a):
    return a.detach().cpu().numpy() if _is_torch(a) else np.asarray(a)


def latent_width(cfg) -> int:
    """Columns of get_obs_cond's layout that hold image latents: vae_feature_dim per camera, in front of the low-dimensional ones."""
    return int(cfg["vae_feature_dim"]) * max(1, len(cfg.get("rgb_obs", ()) or ()))


def _columns(cfg, goal_dims) -> np.ndarray:
    """goal_dims -> bool (D,)."""
    D = int(cfg["obs_dim"])
    cols = np.zeros(D, bool)
    if goal_dims is None or (isinstance(goal_dims, str) and goal_dims == "all"):
        cols[:] = True
    elif isinstance(goal_dims, str):
        w = latent_width(cfg)
        if goal_dims == "latent":
            cols[:w] = True
        elif goal_dims == "lowdim":
            cols[w:] = True
        else:
            raise ValueError(f"goal_dims must be None, 'all', 'latent', 'lowdim', an index list or a bool ({D},) array, got {goal_dims!r}")
    else:
        g = _host(goal_dims)
        if g.dtype == bool:
            if g.shape != (D,):
                raise ValueError(f"goal_dims as a bool array must have shape {(D,)}, got {g.shape}")
            cols = g.copy()
        else:
            if g.ndim != 1 or g.size == 0 or not np.issubdtype(g.dtype, np.integer):
                raise ValueError(f"goal_dims as an index list must be a non-empty 1-D list of integers, got {goal_dims!r}")
            if g.min() < 0 or g.max() >= D:
                raise ValueError(f"goal_dims index outside 0..obs_dim-1 = {D - 1}: {g.tolist()}")
            cols[g] = True
    return cols


def _steps(cfg, t_goal) -> list:
    T = int(cfg["pred_horizon"])
    if t_goal is None:
        t_goal = int(cfg["action_horizon"]) - 1
    if isinstance(t_goal, (int, np.integer)):
        ts = [t_goal]
    elif isinstance(t_goal, (list, tuple, np.ndarray)):
        ts = list(t_goal)
    else:
        raise ValueError(f"t_goal must be an int or a list of ints, got {t_goal!r}")
    if not ts:
        raise ValueError("t_goal must name at least one step")
    for t in ts:
        if isinstance(t, bool) or not isinstance(t, (int, np.integer)):
            raise ValueError(f"t_goal must be an int or a list of ints, got {t_goal!r}")
        if not 0 <= int(t) < T:
            raise ValueError(f"t_goal {int(t)} outside 0..pred_horizon-1 = {T - 1}")
    return [int(t) for t in ts]


def build_constraint(cfg, B: int, target=None, mask=None, goal=None, t_goal=None, goal_dims=None):
    """-> (target (B, T, D) float32, mask (B, T, D) uint8) for the engine's constrained calls.  Two forms, which may be combined (the
    masks are or-ed; where both name an element the goal's value is written):
      * target (B, T, D) with mask broadcast from (D,), (T, D) or (B, T, D) -- bool, or integers (non-zero = constrained);
      * goal (B, D) embeddings written at step(s) t_goal (an int or a list of ints; default action_horizon - 1, as in sample_best_of)
        into the columns goal_dims: None / 'all', 'latent' (the image latents in front of get_obs_cond's layout), 'lowdim' (the rest),
        an index list, or a bool (D,) array.
    Neither form given: the empty constraint (all-zero mask).  Values are in the normalised embedding units of the plan itself; the
    scheduler clips its own x0 estimate to [-1, 1], so targets belong there (not checked).
    target comes back as a torch tensor on the input's device when `target` or `goal` is one (no host round trip), else as a NumPy
    array; mask is always a NumPy array.  Shape, range and type errors are ValueErrors that name the argument."""
    B = int(B)
    if B < 1:
        raise ValueError(f"B must be >= 1, got {B}")
    T, D = int(cfg["pred_horizon"]), int(cfg["obs_dim"])
    if (target is None) != (mask is None):
        raise ValueError("target and mask go together: give both or neither")
    if goal is None and (t_goal is not None or goal_dims is not None):
        raise ValueError("t_goal and goal_dims describe `goal`: give goal too")
    use_torch = _is_torch(target) or _is_torch(goal)
    if use_torch:
        import torch
        dev = (target if _is_torch(target) else goal).device
    m = np.zeros((B, T, D), np.uint8)
    if target is not None:
        if tuple(target.shape if hasattr(target, "shape") else np.shape(target)) != (B, T, D):
            raise ValueError(f"target must have shape {(B, T, D)}, got {tuple(np.shape(target))}")
        mk = _host(mask)
        if mk.dtype != bool and not np.issubdtype(mk.dtype, np.integer):
            raise ValueError(f"mask must be bool or integer, got {mk.dtype}")
        if mk.shape not in ((D,), (T, D), (B, T, D)):
            raise ValueError(f"mask must have shape {(D,)}, {(T, D)} or {(B, T, D)}, got {mk.shape}")
        m |= np.broadcast_to(mk != 0, (B, T, D)).astype(np.uint8)
        if use_torch:
            tg = (target if _is_torch(target) else torch.as_tensor(np.asarray(target, np.float32))).to(device=dev, dtype=torch.float32).clone()
        else:
            tg = np.array(target, np.float32)
    else:
        tg = torch.zeros((B, T, D), device=dev, dtype=torch.float32) if use_torch else np.zeros((B, T, D), np.float32)
    if goal is not None:
        if tuple(goal.shape if hasattr(goal, "shape") else np.shape(goal)) != (B, D):
            raise ValueError(f"goal must have shape {(B, D)}, got {tuple(np.shape(goal))}")
        cols = np.flatnonzero(_columns(cfg, goal_dims))
        if use_torch:
            g = (goal if _is_torch(goal) else torch.as_tensor(np.asarray(goal, np.float32))).to(device=dev, dtype=torch.float32)
            ci = torch.as_tensor(cols, device=dev)
        else:
            g = np.asarray(goal, np.float32)
        for t in _steps(cfg, t_goal):
            if use_torch:
                tg[:, t, ci] = g[:, ci]
            else:
                tg[:, t, cols] = g[:, cols]
            m[:, t, cols] = 1
    return tg, m
