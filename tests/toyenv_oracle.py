"""ORACLE (test infrastructure, NOT a product path) -- the reach2d task of csrc/env.hip (include/ldp_env.h) restated in
NumPy float32: every operation rounded once, fused multiply-adds through guide_oracle.fma32, the draws from oracle/philox.py.  The kernels must reproduce every output of this file bit for bit.

`NumpyReach2DEnv` has the interface of toyenv.Reach2DEnv on host arrays: harness.run_device_eval runs on it without a GPU."""
from __future__ import annotations

import numpy as np

from oracle import philox
from tests.guide_oracle import fma32 as _fma32

F32 = np.float32


def fma32(a, b, c):
    """guide_oracle.fma32 (rn(a * b + c), exactly) for scalars too."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    return _fma32(a.reshape(-1), b.reshape(-1), c.reshape(-1)).reshape(a.shape)



R, DT, TOL, WY, H = F32(0.3), F32(0.08), F32(0.08), F32(0.65), 48
R2, TOL2 = F32(R * R), F32(TOL * TOL)
INV_DT = F32(12.5)
STREAM_ENV = 13
GIVEN, EXPERT, STRAIGHT, RANDOM = 0, 1, 2, 3
POLICIES = {"expert": EXPERT, "straight": STRAIGHT, "random": RANDOM}
PX, PY, GX, GY, SIDE, T, FIRST, BLOCKED = range(8)
ONE, TWO, HALF = F32(1), F32(2), F32(0.5)


def uniform(w):
    """u(w) = (w >> 8) * 2^-24, exact in float32."""
    return ((np.asarray(w, np.uint32) >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)).astype(F32)


def reset(n, seed, episode0=0):
    """-> state (n, 8) float32."""
    w = philox.words(int(seed), int(episode0), 0, STREAM_ENV, n)
    s = np.zeros((n, 8), F32)
    s[:, PX], s[:, PY] = F32(-0.8), F32(-0.5) + uniform(w[:, 0])
    s[:, GX], s[:, GY] = F32(0.8), F32(-0.5) + uniform(w[:, 1])
    s[:, SIDE] = np.where(w[:, 2] & 1, ONE, -ONE)
    return s


def chebyshev(u):
    """T1..T4 of u -> (..., 4)."""
    u = np.asarray(u, F32)
    u2 = (u + u).astype(F32)
    t2 = fma32(u2, u, -ONE)
    t3 = fma32(u2, t2, -u)
    t4 = fma32(u2, t3, -t2)
    return np.stack([u, t2, t3, t4], -1)


def observe(s):
    """-> pos (n, 2), goal (n, 2), latent (n, 16)."""
    pos, goal = s[:, [PX, PY]].copy(), s[:, [GX, GY]].copy()
    rel = ((goal - pos).astype(F32) * HALF).astype(F32)
    lat = np.concatenate([chebyshev(pos[:, 0]), chebyshev(pos[:, 1]), chebyshev(rel[:, 0]), chebyshev(rel[:, 1])], -1)
    return pos, goal, lat.astype(F32)


def clamp1(a):
    return np.minimum(np.maximum(np.asarray(a, F32), -ONE), ONE).astype(F32)


def scripted_action(s, policy, noise, seed, episode0=0):
    """The action (n, 2) of a scripted policy at the state's own time t (the draws of step 1 + t)."""
    n = s.shape[0]
    w = np.empty((n, 4), np.uint32)
    for t in np.unique(s[:, T]):                                                    # (lockstep: one value)
        m = s[:, T] == t
        w[m] = philox.words(int(seed), int(episode0), 1 + int(t), STREAM_ENV, n)[m]
    r = np.stack([fma32(TWO, uniform(w[:, 0]), -ONE), fma32(TWO, uniform(w[:, 1]), -ONE)], -1)    # 2u - 1
    if policy == RANDOM:
        return r
    p, g = s[:, [PX, PY]], s[:, [GX, GY]]
    tgt = g.copy()
    if policy == EXPERT:
        left = s[:, PX] < 0
        tgt[left, 0], tgt[left, 1] = F32(0), (s[left, SIDE] * WY).astype(F32)
    elif policy != STRAIGHT:
        raise ValueError(f"unknown policy {policy}")
    d = ((tgt - p).astype(F32) * INV_DT).astype(F32)
    m = np.maximum(np.maximum(np.abs(d[:, 0]), np.abs(d[:, 1])), ONE)
    a = (d / m[:, None]).astype(F32)
    return clamp1(fma32(F32(noise), r, a))


def sanitize(a):
    """NaN reads as 0; clamp to [-1, 1] (the first two components)."""
    a = np.asarray(a, F32)[..., :2]
    return clamp1(np.where(np.isnan(a), F32(0), a))


def advance(s, a):
    """One sub-step with the sanitized action a (n, 2), in place."""
    p = s[:, [PX, PY]]
    q = clamp1(fma32(DT, a, p))
    blocked = fma32(q[:, 0], q[:, 0], (q[:, 1] * q[:, 1]).astype(F32)) < R2
    p = np.where(blocked[:, None], p, q)
    s[:, PX], s[:, PY] = p[:, 0], p[:, 1]
    s[:, BLOCKED] += blocked.astype(F32)
    s[:, T] += ONE
    d = (p - s[:, [GX, GY]]).astype(F32)
    hit = (s[:, FIRST] == 0) & (fma32(d[:, 0], d[:, 0], (d[:, 1] * d[:, 1]).astype(F32)) <= TOL2)
    s[hit, FIRST] = s[hit, T]


def step(s, n_sub, actions=None, policy=GIVEN, noise=0.0, seed=0, episode0=0, A=2):
    """n_sub sub-steps in place -> (actions taken (n, n_sub, A), pos (n, n_sub, 2), goal (n, n_sub, 2), latent (n, n_sub, 16)): the
    observation in front of every sub-step.  Components from 2 up of the actions taken are 0."""
    n = s.shape[0]
    if policy == GIVEN:
        A = np.asarray(actions).shape[-1]
    taken = np.zeros((n, n_sub, A), F32)
    pos, goal, lat = np.zeros((n, n_sub, 2), F32), np.zeros((n, n_sub, 2), F32), np.zeros((n, n_sub, 16), F32)
    for j in range(n_sub):
        pos[:, j], goal[:, j], lat[:, j] = observe(s)
        a = sanitize(np.asarray(actions, F32)[:, j]) if policy == GIVEN else scripted_action(s, policy, noise, seed, episode0)
        taken[:, j, :2] = a
        advance(s, a)
    return taken, pos, goal, lat


def rollout(n, policy, noise, seed, episode0=0, steps=H):
    """A whole scripted episode -> (state, actions (n, steps, 2), pos, goal, latent)."""
    s = reset(n, seed, episode0)
    return (s,) + step(s, steps, policy=policy, noise=noise, seed=seed, episode0=episode0)


class NumpyReach2DEnv:
    """toyenv.Reach2DEnv on the host (same methods, NumPy arrays for device tensors)."""
    episode_len = H

    def __init__(self, n_envs, action_dim=2):
        self.n_envs, self.action_dim = int(n_envs), int(action_dim)
        self.seed = self.episode0 = 0
        self.state = np.zeros((self.n_envs, 8), F32)

    def reset(self, seed, episode0=0):
        self.seed, self.episode0 = int(seed), int(episode0)
        self.state = reset(self.n_envs, seed, episode0)

    def observe(self):
        pos, goal, lat = observe(self.state)
        return {"obs": {"pos": pos[:, None], "goal": goal[:, None], "latent_image": lat[:, None]}}

    def step(self, actions):
        a = np.asarray(actions, F32)
        step(self.state, a.shape[1], actions=a)

    def step_scripted(self, policy, noise=0.0, seed=None, n_sub=1):
        step(self.state, n_sub, policy=POLICIES[policy], noise=noise, seed=self.seed if seed is None else seed, episode0=self.episode0)

    def success(self):
        return self.state[:, FIRST] != 0

    def first_success(self):
        return self.state[:, FIRST].astype(np.int32)

    def blocked(self):
        return self.state[:, BLOCKED].astype(np.int32)
