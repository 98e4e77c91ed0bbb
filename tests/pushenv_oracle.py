"""ORACLE (test infrastructure, NOT a product path) -- the push2d task of csrc/push.hip (include/ldp_push.h) restated in
NumPy float32: every operation rounded once, fused multiply-adds through guide_oracle.fma32, NumPy's correctly rounded float32 sqrt and
divide, the draws from oracle/philox.py.  The kernels must reproduce every output of this file bit for bit.

Every function takes `episode0` as a number (environment i is the global episode episode0 + i) or as an array of one global episode per
row, so that a handful of rows of a very large batch can be computed alone.
`NumpyPush2DEnv` has the interface of pushenv.Push2DEnv on host arrays: harness.run_device_eval runs on it without a GPU."""
from __future__ import annotations

import numpy as np

from oracle import philox
from tests.guide_oracle import fma32 as _fma32

F32 = np.float32


def fma32(a, b, c):
    """guide_oracle.fma32 (rn(a * b + c), exactly) for scalars too."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    return _fma32(a.reshape(-1), b.reshape(-1), c.reshape(-1)).reshape(a.shape)


C, DT, TOL, LIM, H = F32(0.2), F32(0.08), F32(0.1), F32(0.85), 48
C2, TOL2 = F32(C * C), F32(TOL * TOL)
INV_DT = F32(12.5)
STREAM_PUSH = 14
STATE, LATENT = 12, 16
GIVEN, EXPERT, STRAIGHT, RANDOM = 0, 1, 2, 3
POLICIES = {"expert": EXPERT, "straight": STRAIGHT, "random": RANDOM}
PX, PY, OX, OY, GX, GY, SIDE, T, FIRST, BLOCKED, PUSHED, PAD = range(12)
ZERO, ONE, TWO, HALF = F32(0), F32(1), F32(2), F32(0.5)
# the expert's own constants
APPR, PUSH, WIDE, DEAD, BEHIND, CONE, AHEAD, NEAR, EPS = F32(0.3), F32(0.1), F32(0.39), F32(0.05), F32(-0.1), F32(0.6), F32(-0.25), F32(0.3), F32(1e-6)


def uniform(w):
    """u(w) = (w >> 8) * 2^-24, exact in float32."""
    return ((np.asarray(w, np.uint32) >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)).astype(F32)


def episodes(n, episode0):
    """The global episode of every row: episode0 + i, or episode0 itself when it is an array."""
    if np.ndim(episode0):
        e = np.asarray(episode0, np.uint64)
        assert e.shape == (n,)
        return e
    return np.uint64(int(episode0)) + np.arange(n, dtype=np.uint64)


def words(seed, eps, step):
    """(n, 4) Philox words of (seed, element = eps[i], step[i] (or one step), STREAM_PUSH)."""
    eps = np.asarray(eps, np.uint64)
    n = eps.shape[0]
    st = np.broadcast_to(np.asarray(step, np.uint64), (n,))
    ctr = np.stack([eps & philox.MASK, eps >> np.uint64(32), st, np.full(n, STREAM_PUSH, np.uint64)], -1)
    seed = int(seed) & (2**64 - 1)
    return philox.philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))


def reset(n, seed, episode0=0):
    """-> state (n, 12) float32."""
    w = words(seed, episodes(n, episode0), 0)
    s = np.zeros((n, STATE), F32)
    s[:, PX], s[:, PY] = F32(-0.8), F32(-0.5) + uniform(w[:, 0])
    s[:, OX], s[:, OY] = fma32(F32(0.6), uniform(w[:, 1]), F32(-0.3)), fma32(F32(0.8), uniform(w[:, 2]), F32(-0.4))
    s[:, GX], s[:, GY] = np.where(w[:, 0] & 1, F32(-0.6), F32(0.6)), F32(-0.5) + uniform(w[:, 3])
    s[:, SIDE] = np.where(w[:, 1] & 1, ONE, -ONE)
    return s


def cheb2(x):
    """T1, T2 of x -> (..., 2)."""
    x = np.asarray(x, F32)
    return np.stack([x, fma32((x + x).astype(F32), x, -ONE)], -1)


def half_diff(a, b):
    return ((a - b).astype(F32) * HALF).astype(F32)


def observe(s):
    """-> pos (n, 2), goal (n, 2), latent (n, 16)."""
    pos, goal = s[:, [PX, PY]].copy(), s[:, [GX, GY]].copy()
    feats = [s[:, PX], s[:, PY], s[:, OX], s[:, OY], half_diff(s[:, GX], s[:, OX]), half_diff(s[:, GY], s[:, OY]),
             half_diff(s[:, OX], s[:, PX]), half_diff(s[:, OY], s[:, PY])]
    return pos, goal, np.concatenate([cheb2(f) for f in feats], -1).astype(F32)


def clamp1(a):
    return np.minimum(np.maximum(np.asarray(a, F32), -ONE), ONE).astype(F32)


def dot2(ax, ay, bx, by):
    """fma(ax, bx, rn(ay * by))."""
    return fma32(ax, bx, (ay * by).astype(F32))


def expert_target(s):
    """The expert's target (n, 2): behind the disc it pushes, beside or ahead of it it goes round on the side it is on."""
    p, o, g = s[:, [PX, PY]], s[:, [OX, OY]], s[:, [GX, GY]]
    v = (g - o).astype(F32)
    L = np.sqrt(dot2(v[:, 0], v[:, 1], v[:, 0], v[:, 1])).astype(F32)
    u = (v / np.maximum(L, EPS)[:, None]).astype(F32)
    nh = np.stack([-u[:, 1], u[:, 0]], -1)
    rr = (p - o).astype(F32)
    along = dot2(rr[:, 0], rr[:, 1], u[:, 0], u[:, 1])
    lat = dot2(rr[:, 0], rr[:, 1], nh[:, 0], nh[:, 1])
    sgn = np.where(np.abs(lat) > DEAD, np.where(lat > 0, ONE, -ONE), s[:, SIDE]).astype(F32)
    appr = fma32(-APPR, u, o)
    push = fma32(-PUSH, u, o)
    w = (WIDE * sgn).astype(F32)[:, None]
    wp = fma32(w, nh, fma32(clamp1(along)[:, None], u, o))
    corner = fma32(w, nh, appr)
    behind = (along < BEHIND) & (np.abs(lat) < (CONE * np.abs(along)).astype(F32))
    ahead = along > AHEAD
    near = np.abs(lat) < NEAR
    return np.where(behind[:, None], push, np.where(ahead[:, None], np.where(near[:, None], wp, corner), appr)).astype(F32)


def scripted_action(s, policy, noise, seed, episode0=0):
    """The action (n, 2) of a scripted policy at the state's own time t (the draws of step 1 + t)."""
    n = s.shape[0]
    w = words(seed, episodes(n, episode0), 1 + s[:, T].astype(np.uint64))
    r = np.stack([fma32(TWO, uniform(w[:, 0]), -ONE), fma32(TWO, uniform(w[:, 1]), -ONE)], -1)    # 2u - 1
    if policy == RANDOM:
        return r
    if policy == EXPERT:
        tgt = expert_target(s)
    elif policy == STRAIGHT:
        tgt = s[:, [OX, OY]]
    else:
        raise ValueError(f"unknown policy {policy}")
    d = ((tgt - s[:, [PX, PY]]).astype(F32) * INV_DT).astype(F32)
    m = np.maximum(np.maximum(np.abs(d[:, 0]), np.abs(d[:, 1])), ONE)
    return clamp1(fma32(F32(noise), r, (d / m[:, None]).astype(F32)))


def sanitize(a):
    """NaN reads as 0; clamp to [-1, 1] (the first two components)."""
    a = np.asarray(a, F32)[..., :2]
    return clamp1(np.where(np.isnan(a), ZERO, a))


def advance(s, a):
    """One sub-step with the sanitized action a (n, 2), in place."""
    p, o = s[:, [PX, PY]], s[:, [OX, OY]]
    q = clamp1(fma32(DT, a, p))
    d = (o - q).astype(F32)
    d2 = dot2(d[:, 0], d[:, 1], d[:, 0], d[:, 1])
    touch = d2 < C2
    dist = np.sqrt(d2).astype(F32)
    pos = dist > 0
    safe = np.where(pos, dist, ONE)
    nrm = np.where(pos[:, None], (d / safe[:, None]).astype(F32), np.array([1, 0], F32))
    o2 = fma32(C, nrm, q)
    refused = touch & ((np.abs(o2[:, 0]) > LIM) | (np.abs(o2[:, 1]) > LIM))
    moved = touch & ~refused
    p = np.where(refused[:, None], p, q)
    o = np.where(moved[:, None], o2, o)
    s[:, PX], s[:, PY], s[:, OX], s[:, OY] = p[:, 0], p[:, 1], o[:, 0], o[:, 1]
    s[:, BLOCKED] += refused.astype(F32)
    s[:, PUSHED] += moved.astype(F32)
    s[:, T] += ONE
    e = (o - s[:, [GX, GY]]).astype(F32)
    hit = (s[:, FIRST] == 0) & (dot2(e[:, 0], e[:, 1], e[:, 0], e[:, 1]) <= TOL2)
    s[hit, FIRST] = s[hit, T]


def step(s, n_sub, actions=None, policy=GIVEN, noise=0.0, seed=0, episode0=0, A=2):
    """n_sub sub-steps in place -> (actions taken (n, n_sub, A), pos (n, n_sub, 2), goal (n, n_sub, 2), latent (n, n_sub, 16)): the
    observation in front of every sub-step.  Components from 2 up of the actions taken are 0."""
    n = s.shape[0]
    if policy == GIVEN:
        A = np.asarray(actions).shape[-1]
    taken = np.zeros((n, n_sub, A), F32)
    pos, goal, lat = np.zeros((n, n_sub, 2), F32), np.zeros((n, n_sub, 2), F32), np.zeros((n, n_sub, LATENT), F32)
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


class NumpyPush2DEnv:
    """pushenv.Push2DEnv on the host (same methods, NumPy arrays for device tensors)."""
    episode_len = H

    def __init__(self, n_envs, action_dim=2):
        self.n_envs, self.action_dim = int(n_envs), int(action_dim)
        self.seed = self.episode0 = 0
        self.state = np.zeros((self.n_envs, STATE), F32)

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

    def pushed(self):
        return self.state[:, PUSHED].astype(np.int32)
