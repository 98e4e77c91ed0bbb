"""Guided planning: the host side of LDPAgent.sample_guided -- the assembly of a caller's soft goals, smoothness and
box bounds into a Guide, its step-size table and the descent bound.  The kernels are csrc/guide.hip's, through
HipEngine.plan_guide_step / plan_guide_cost / plan_sample_guided / agent_sample_guided.

The cost of sample b on the clipped data prediction y (T, D), all weights >= 0:
    J_b(y) = 1/2 sum_{t,c} weight[b,t,c] (y[t,c] - target[b,t,c])^2
           + 1/2 sum_c lam[c] ( sum_{t < T-1} (y[t+1,c] - y[t,c])^2 + [anchor] (y[0,c] - anchor[b,c])^2 )
           + 1/2 sum_{t,c} beta[c] ( max(y - hi[c], 0)^2 + max(lo[c] - y, 0)^2 )
Step i of a guided loop replaces the data prediction y by clip(y - rho[i] grad J(y), -1, 1).  grad J is Lipschitz with a constant below
L = max weight + 4 max lam + max beta (the path-graph Laplacian's eigenvalues lie below 4), so rho[i] L <= 1 makes every such step a
descent step of J; step_sizes refuses anything larger."""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import schedule
from .constrain import _columns, _host, _is_torch, _steps

SCHEDULES = ("sigma2", "constant")


def _vector(name: str, v, D: int, default: float) -> np.ndarray:
    """A scalar or a (D,) vector -> float32 (D,)."""
    a = np.asarray(default if v is None else _host(v), dtype=np.float64)
    if a.ndim == 0:
        a = np.full(D, float(a))
    if a.shape != (D,):
        raise ValueError(f"{name} must be a scalar or have shape {(D,)}, got {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError(f"{name} must be finite")
    return a.astype(np.float32)


def _weights(name: str, v, D: int) -> np.ndarray:
    a = _vector(name, v, D, 0.0)
    if (a < 0).any():
        raise ValueError(f"{name} must be >= 0 (a negative weight turns the cost upside down), got min = {float(a.min())}")
    return a


class Guide:
    """A trajectory cost for B plans and the step sizes it is descended with.  Fields: target, weight (B, T, D) -- torch tensors when
    the caller gave one, else NumPy float32 --, anchor (B, D), None, or True (LDPAgent.sample_guided puts the batch's own last
    observation embedding there), lam, beta, lo, hi (D,) float32, and (scale, schedule) for step_sizes.  With an engine bound to it a
    Guide is a cost function on candidate plans: guide(candidates (B, N, T, D)) -> (B, N) device costs, the `score=` of
    LDPAgent.sample_best_of."""

    def __init__(self, cfg, B, target, weight, anchor, lam, beta, lo, hi, scale, schedule, engine=None, wmax=None):
        self.cfg, self.B = cfg, int(B)
        self.wmax = wmax                                     # max weight, when the builder knows it on the host (else read from `weight`)
        self.target, self.weight, self.anchor = target, weight, anchor
        self.lam, self.beta, self.lo, self.hi = lam, beta, lo, hi
        self.scale, self.schedule, self.engine = scale, schedule, engine

    @property
    def lipschitz(self) -> float:
        """L = max weight + 4 max lam + max beta: an upper bound of the Lipschitz constant of grad J."""
        wmax = float(self.weight.max()) if self.wmax is None else float(self.wmax)
        return wmax + 4.0 * float(self.lam.max()) + float(self.beta.max())

    def step_sizes(self, n_steps: int, sampler: str = "ddim", n_train: Optional[int] = None) -> np.ndarray:
        """rho (n_steps,) float32 for a loop of n_steps executed steps: schedule "sigma2" -> scale (1 - abar_t_i) with t_i the timestep of
        executed step i (guidance fades as the noise does), "constant" -> scale, an explicit sequence -> itself (scale ignored).  scale
        None is 1 / L, the largest constant step the descent bound allows (0 for the empty guide).  ValueError when max rho * L > 1."""
        n_steps = int(n_steps)
        n_train = int(self.cfg.get("planner_n_diffusion_steps", 100) if n_train is None else n_train)
        if isinstance(self.schedule, str) and self.schedule == "sigma2":
            if sampler not in ("ddpm", "ddim"):
                raise NotImplementedError(f'guidance under sampler="{sampler}" is not built: it runs under "ddpm" and "ddim"')
            ts = schedule.step_timesteps(n_train, n_steps, schedule.SAMPLER_DDPM if sampler == "ddpm" else schedule.SAMPLER_DDIM)
        else:
            ts = np.zeros(n_steps, np.int64)                   # (a constant or explicit table does not read the timesteps)
        return self._step_sizes(ts, n_train)

    def step_sizes_on(self, timesteps, n_train: Optional[int] = None) -> np.ndarray:
        """step_sizes at the entries of a timestep table (first executed step first), for loops that do not run on the uniform grid
        (sampler "dpmpp" through LDPAgent.plan): "sigma2" -> scale (1 - abar_ts[i]), "constant" and explicit tables as in step_sizes,
        with the same descent-bound refusal."""
        n_train = int(self.cfg.get("planner_n_diffusion_steps", 100) if n_train is None else n_train)
        ts = np.asarray(_host(timesteps), dtype=np.int64).reshape(-1)
        if len(ts) and (ts.min() < 0 or ts.max() >= n_train):
            raise ValueError(f"timesteps must lie in 0..{n_train - 1}, got {ts.tolist()}")
        return self._step_sizes(ts, n_train)

    def _step_sizes(self, ts: np.ndarray, n_train: int) -> np.ndarray:
        """rho at the timesteps ts of the executed steps (step_sizes / step_sizes_on)."""
        n_steps = len(ts)
        L = self.lipschitz
        if self.scale is None:                                 # the largest float32 with scale * L <= 1
            scale = np.float32(1.0 / L if L > 0 else 0.0)
            while float(scale) * L > 1.0:
                scale = np.nextafter(scale, np.float32(0.0))
            scale = float(scale)
        else:
            scale = float(self.scale)
        if isinstance(self.schedule, str):
            if self.schedule == "constant":
                rho = np.full(n_steps, scale, np.float64)
            elif self.schedule == "sigma2":
                acp = schedule.make_schedule(n_train).alphas_cumprod.astype(np.float64)
                rho = scale * (1.0 - acp[ts])
            else:
                raise ValueError(f"schedule must be one of {SCHEDULES} or a sequence of n_steps step sizes, got {self.schedule!r}")
        else:
            rho = np.asarray(_host(self.schedule), dtype=np.float64).reshape(-1)
            if len(rho) != n_steps:
                raise ValueError(f"schedule holds {len(rho)} step sizes: a loop of n_steps = {n_steps} needs one per step")
        if not np.isfinite(rho).all() or (rho < 0).any():
            raise ValueError("step sizes (scale / schedule) must be finite and >= 0")
        rho = rho.astype(np.float32)
        worst = float(rho.max()) if n_steps else 0.0
        if worst * L > 1.0:
            raise ValueError(f"step size too large for a descent step: max rho = {worst:.6g} times L = max weight + 4 max smooth + max "
                             f"bound_weight = {L:.6g} is {worst * L:.6g} > 1 (lower scale below {1.0 / L:.6g})")
        return rho

    def __call__(self, candidates):
        """candidates (B, N, T, D) -> J (B, N) on the device (one launch of csrc/guide.hip's cost kernel)."""
        if self.engine is None:
            raise ValueError("this Guide has no engine: build it with engine= (or through LDPAgent.build_guide) to use it as a cost")
        if candidates.ndim != 4 or candidates.shape[0] != self.B:
            raise ValueError(f"candidates must have shape (B = {self.B}, N, T, D), got {tuple(candidates.shape)}")
        B, N = int(candidates.shape[0]), int(candidates.shape[1])
        return self.engine.plan_guide_cost(candidates.reshape(B * N, *candidates.shape[2:]), self, n_per=N).reshape(B, N)


def build_guide(cfg, B: int, target=None, weight=None, goal=None, t_goal=None, goal_dims=None, goal_weight=None, smooth=None, anchor=None,
                lo=None, hi=None, bound_weight=None, scale=None, schedule="sigma2", engine=None) -> Guide:
    """-> Guide for B plans.  The soft goals take constrain.build_constraint's two forms, which may be combined (the goal's entries win):
      * target (B, T, D) with weight broadcast from a scalar, (D,), (T, D) or (B, T, D), >= 0;
      * goal (B, D) embeddings pulled towards at step(s) t_goal (an int or a list; default action_horizon - 1) in the columns goal_dims
        (None / 'all', 'latent', 'lowdim', an index list, a bool (D,) array) with goal_weight (a scalar or (D,), default 1).
    smooth: lam, a scalar or (D,) (default 0); anchor: None, (B, D) embeddings, or True (sample_guided: the batch's last observation);
    lo / hi: the box, scalars or (D,) (default -1 / 1); bound_weight: beta, a scalar or (D,) (default 0).
    scale / schedule: Guide.step_sizes (scale None: 1 / L).  A constant or explicit schedule is checked against the descent bound here,
    "sigma2" when the step count is known (step_sizes).  Shape, sign and range errors are ValueErrors that name the argument."""
    B = int(B)
    if B < 1:
        raise ValueError(f"B must be >= 1, got {B}")
    T, D = int(cfg["pred_horizon"]), int(cfg["obs_dim"])
    if (target is None) != (weight is None):
        raise ValueError("target and weight go together: give both or neither")
    if goal is None and (t_goal is not None or goal_dims is not None or goal_weight is not None):
        raise ValueError("t_goal, goal_dims and goal_weight describe `goal`: give goal too")
    use_torch = _is_torch(target) or _is_torch(goal)
    if use_torch:
        import torch
        dev = (target if _is_torch(target) else goal).device
    wg = np.zeros((B, T, D), np.float32)
    if target is not None:
        if tuple(target.shape if hasattr(target, "shape") else np.shape(target)) != (B, T, D):
            raise ValueError(f"target must have shape {(B, T, D)}, got {tuple(np.shape(target))}")
        w = np.asarray(_host(weight), dtype=np.float64)
        if w.shape not in ((), (D,), (T, D), (B, T, D)):
            raise ValueError(f"weight must be a scalar or have shape {(D,)}, {(T, D)} or {(B, T, D)}, got {w.shape}")
        if not np.isfinite(w).all() or (w < 0).any():
            raise ValueError("weight must be finite and >= 0 (a negative weight turns the cost upside down)")
        wg[:] = np.broadcast_to(w, (B, T, D))
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
        gw = _weights("goal_weight", 1.0 if goal_weight is None else goal_weight, D)
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
            wg[:, t, cols] = gw[cols]
    if anchor is not None and anchor is not True:
        if tuple(anchor.shape if hasattr(anchor, "shape") else np.shape(anchor)) != (B, D):
            raise ValueError(f"anchor must be True or have shape {(B, D)}, got {tuple(np.shape(anchor))}")
        anchor = anchor if _is_torch(anchor) else np.array(anchor, np.float32)
    lam, beta = _weights("smooth", smooth, D), _weights("bound_weight", bound_weight, D)
    lo_v, hi_v = _vector("lo", lo, D, -1.0), _vector("hi", hi, D, 1.0)
    if (lo_v > hi_v).any():
        c = int(np.flatnonzero(lo_v > hi_v)[0])
        raise ValueError(f"lo must not exceed hi: lo[{c}] = {float(lo_v[c])} > hi[{c}] = {float(hi_v[c])}")
    if not isinstance(schedule, str):
        schedule = np.asarray(_host(schedule), dtype=np.float64).reshape(-1)
    elif schedule not in SCHEDULES:
        raise ValueError(f"schedule must be one of {SCHEDULES} or a sequence of n_steps step sizes, got {schedule!r}")
    if scale is not None and not (np.isfinite(scale) and scale >= 0):
        raise ValueError(f"scale must be finite and >= 0, got {scale}")
    w_out = torch.as_tensor(wg).to(dev) if use_torch else wg
    guide = Guide(cfg, B, tg, w_out, anchor, lam, beta, lo_v, hi_v, scale, schedule, engine, wmax=float(wg.max()))
    if not isinstance(schedule, str):
        guide.step_sizes(len(schedule))                        # an explicit table: its own length, so only the bound can fail here
    elif schedule == "constant":
        guide.step_sizes(1)
    return guide
