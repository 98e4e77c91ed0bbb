"""float64 restatement of guided planning on oracle.np64's pieces: the cost J, its gradient g, the guided step and the
guided loop over a range of executed steps; next to it the float32 emulation of csrc/guide.hip's arithmetic, rounding for rounding, and
the error bounds its spelled roundings imply.

A guide is a dict: target, wg (B, T, D), anchor (B, D) or None, lam, beta, lo, hi (D,).  Layout (B, T, D) throughout."""
import math

import numpy as np

from oracle import np64
from tests import replan_oracle as RO

F64, F32 = np.float64, np.float32
U = 2.0 ** -24                # unit round-off of float32


def make(B, T, D, target=None, wg=None, anchor=None, lam=0.0, beta=0.0, lo=-1.0, hi=1.0):
    vec = lambda v: np.broadcast_to(np.asarray(v, F32), (D,)).copy()           # noqa: E731
    return dict(target=np.zeros((B, T, D), F32) if target is None else np.asarray(target, F32),
                wg=np.zeros((B, T, D), F32) if wg is None else np.asarray(wg, F32),
                anchor=None if anchor is None else np.asarray(anchor, F32), lam=vec(lam), beta=vec(beta), lo=vec(lo), hi=vec(hi))


def lipschitz(G):
    return float(G["wg"].max()) + 4.0 * float(G["lam"].max()) + float(G["beta"].max())


def _g64(G):
    return {k: (None if v is None else np.asarray(v, F64)) for k, v in G.items()}


def cost(y, G):
    """J_b(y) -> (B,), float64."""
    y, G = np.asarray(y, F64), _g64(G)
    J = 0.5 * (G["wg"] * (y - G["target"]) ** 2).sum(axis=(1, 2))
    sm = ((y[:, 1:] - y[:, :-1]) ** 2).sum(axis=1)                             # (B, D)
    if G["anchor"] is not None:
        sm = sm + (y[:, 0] - G["anchor"]) ** 2
    J += 0.5 * (G["lam"] * sm).sum(axis=1)
    J += 0.5 * (G["beta"] * (np.maximum(y - G["hi"], 0.0) ** 2 + np.maximum(G["lo"] - y, 0.0) ** 2)).sum(axis=(1, 2))
    return J


def grad(y, G):
    """g = dJ/dy (B, T, D), float64: elementwise plus the three-point stencil along T."""
    y, G = np.asarray(y, F64), _g64(G)
    g = G["wg"] * (y - G["target"])
    s = np.zeros_like(y)
    s[:, :-1] += y[:, :-1] - y[:, 1:]
    s[:, 1:] += y[:, 1:] - y[:, :-1]
    if G["anchor"] is not None:
        s[:, 0] += y[:, 0] - G["anchor"]
    g += G["lam"] * s
    g += G["beta"] * (np.maximum(y - G["hi"], 0.0) - np.maximum(G["lo"] - y, 0.0))
    return g


def project(y, G, rho):
    """One projected gradient step on the clipped data prediction."""
    y = np.asarray(y, F64)
    return np.clip(y - rho * grad(y, G), -1.0, 1.0)


def step_coefs(i, n_train, n_steps, sampler, cast32=False):
    """Row i of the scheduler's coefficients in float64 (cast32: rounded to float32 first, as the kernel holds them):
    (t, inv_sqrt_ab, sqrt_1mab, c_x0, c_x, c_eps, sigma)."""
    betas, alphas, acp = np64.ddpm_tables(n_train)
    t = RO.step_timestep(i, n_train, n_steps, sampler)
    a_t = F64(acp[t])
    row = [float(t), 1.0 / math.sqrt(a_t), math.sqrt(1.0 - a_t), 0.0, 0.0, 0.0, 0.0]
    if sampler == "ddpm":
        a_prev = F64(acp[t - 1]) if t > 0 else 1.0
        beta, alpha = F64(betas[t]), F64(alphas[t])
        row[3] = math.sqrt(a_prev) * beta / (1.0 - a_t)
        row[4] = math.sqrt(alpha) * (1.0 - a_prev) / (1.0 - a_t)
        row[6] = math.sqrt(max((1.0 - a_prev) / (1.0 - a_t) * beta, 1e-20)) if t > 0 else 0.0
    else:
        tp = t - n_train // n_steps
        a_prev = F64(acp[tp]) if tp >= 0 else 1.0
        row[3], row[5] = math.sqrt(a_prev), math.sqrt(1.0 - a_prev)
    return [float(F32(v)) for v in row] if cast32 else row


def guided_step(x, eps, G, rho, k, z=None):
    """x' of one guided step in float64 with the coefficient row k (step_coefs) and the step size rho; z: the step's noise (sigma != 0)."""
    x, eps = np.asarray(x, F64), np.asarray(eps, F64)
    _, inv_a, sg, c_x0, c_x, c_eps, sigma = k
    y = np.clip((x - sg * eps) * inv_a, -1.0, 1.0)
    out = c_x0 * project(y, G, rho) + c_x * x + c_eps * eps
    if sigma != 0.0:
        out = out + sigma * np.asarray(z, F64)
    return out


def planner_range_guided(params, cond, x, begin, end, G, rho, step_noise=None, n_train=100, n_steps=100, sampler="ddim", **unet_kw):
    """The guided loop over the executed steps [begin, end) on np64's U-Net; step_noise (n_steps, B, T, D) for DDPM."""
    x = np.asarray(x, F64)
    for i in range(begin, end):
        k = step_coefs(i, n_train, n_steps, sampler)
        eps = np64.unet_forward(params, x, int(k[0]), cond, **unet_kw)
        x = guided_step(x, eps, G, float(rho[i]), k, None if step_noise is None else step_noise[i])
    return x


# ---- the kernel's arithmetic in float32, rounding for rounding ------------------------------------------------------------------------------
def fma32(a, b, c):
    """rn(a * b + c) for float32 arrays, exactly: the product of two float32 numbers is exact in float64; the float64 sum is rounded to
    ODD (TwoSum gives its error exactly: when it is not zero and the sum's last bit is even, the sum moves one ulp towards the error), and
    a value rounded to odd at 53 bits rounds to 24 bits like the exact one."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    p, c = a.astype(F64) * b.astype(F64), c.astype(F64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    si = s.copy().view(np.int64)
    fix = (err != 0) & ((si & 1) == 0) & np.isfinite(s)
    up = (err > 0) == (s > 0)                                                  # towards the larger magnitude: the integer form grows
    si[fix & up] += 1
    si[fix & ~up] -= 1
    return si.view(F64).astype(F32)


def emulate_step(x, eps, G, rho, k, z=None):
    """plan_compose_step_kernel<0, true, false>'s result (the guided step) bit for bit: x, eps, z float32 (B, T, D); k: the float32
    coefficient row; rho: the float32 step."""
    x, eps = np.asarray(x, F32), np.asarray(eps, F32)
    _, inv_a, sg, c_x0, c_x, c_eps, sigma = (F32(v) for v in k)
    one = F32(1.0)
    y = np.clip(fma32(-sg, eps, x) * inv_a, -one, one)                         # (float32 * float32 rounds once)
    g = G["wg"] * (y - G["target"])
    dn, dp = np.zeros_like(y), np.zeros_like(y)
    dn[:, :-1] = y[:, :-1] - y[:, 1:]
    dp[:, 1:] = y[:, 1:] - y[:, :-1]
    if G["anchor"] is not None:
        dp[:, 0] = y[:, 0] - G["anchor"]
    g = fma32(G["lam"], dn + dp, g)
    hu, hl = np.maximum(y - G["hi"], F32(0)), np.maximum(G["lo"] - y, F32(0))
    g = fma32(G["beta"], hu - hl, g)
    yg = np.clip(fma32(-F32(rho), g, y), -one, one)
    v = fma32(c_eps, eps, fma32(c_x, x, c_x0 * yg))
    if sigma != 0:
        v = fma32(sigma, np.asarray(z, F32), v)
    assert v.dtype == F32 and y.dtype == F32 and g.dtype == F32
    return v


def step_bound(x, eps, G, rho, k, z=None):
    """|kernel - guided_step(float32 coefficients)| <= this, elementwise, from the kernel's spelled roundings (first order in u = 2^-24,
    times 1 + 2^-10 for the higher orders).  clip and max(., 0) are 1-Lipschitz, so an error passes through them undiminished at worst:
      y:   two roundings, e_y = 2u |(x - sg eps) inv_a|
      g:   goal  wg e_y + 2u |wg (y - target)|;  stencil  lam (e_dn + e_dp + u |dn + dp|) with e_dn = e_y + e_y(t+1) + u |dn| and
           likewise e_dp (the anchor is exact);  hinge  beta (2 e_y + u |y - hi|+ + u |lo - y|+ + u |h|);  plus u |g| for each of the two fma
      y':  rho e_g + e_y + u |y - rho g|
      x':  |c_x0| e_y' + u (|m1| + |m2| + |m3| + |m4|), the partial sums of the update in the kernel's order."""
    x, eps, G = np.asarray(x, F64), np.asarray(eps, F64), _g64(G)
    _, inv_a, sg, c_x0, c_x, c_eps, sigma = k
    raw = (x - sg * eps) * inv_a
    y = np.clip(raw, -1.0, 1.0)
    e_y = 2.0 * U * np.abs(raw)
    gg = G["wg"] * (y - G["target"])
    e_g = G["wg"] * e_y + 2.0 * U * np.abs(gg)
    dn, dp, e_dn, e_dp = (np.zeros_like(y) for _ in range(4))
    dn[:, :-1] = y[:, :-1] - y[:, 1:]
    e_dn[:, :-1] = e_y[:, :-1] + e_y[:, 1:] + U * np.abs(dn[:, :-1])
    dp[:, 1:] = y[:, 1:] - y[:, :-1]
    e_dp[:, 1:] = e_y[:, 1:] + e_y[:, :-1] + U * np.abs(dp[:, 1:])
    if G["anchor"] is not None:
        dp[:, 0] = y[:, 0] - G["anchor"]
        e_dp[:, 0] = e_y[:, 0] + U * np.abs(dp[:, 0])
    g2 = gg + G["lam"] * (dn + dp)
    e_g = e_g + G["lam"] * (e_dn + e_dp + U * np.abs(dn + dp)) + U * np.abs(g2)
    hu, hl = np.maximum(y - G["hi"], 0.0), np.maximum(G["lo"] - y, 0.0)
    g3 = g2 + G["beta"] * (hu - hl)
    e_g = e_g + G["beta"] * (2.0 * e_y + U * (hu + hl) + U * np.abs(hu - hl)) + U * np.abs(g3)
    pre = y - rho * g3
    e_yg = rho * e_g + e_y + U * np.abs(pre)
    yg = np.clip(pre, -1.0, 1.0)
    m1 = c_x0 * yg
    m2 = m1 + c_x * x
    m3 = m2 + c_eps * eps
    m4 = m3 + (sigma * np.asarray(z, F64) if sigma != 0.0 else 0.0)
    return (abs(c_x0) * e_yg + U * (np.abs(m1) + np.abs(m2) + np.abs(m3) + (np.abs(m4) if sigma != 0.0 else 0.0))) * (1.0 + 2.0 ** -10)


def cost_bound(y, G):
    """|kernel J - cost| <= this (B,).  Every part of an element's term is >= 0, so relative errors add up without cancellation: a rounded
    difference that is squared carries 2u, the square (or the fma that adds it) u, the product with the weight (or its fma) u, and each
    later fma of the running value u more -- the goal part reaches 6u (4u, then the fma with lam and the fma with beta), the stencil part
    6u (the anchor's fma, the fma with lam, the fma with beta), the hinge part 5u: 8u bounds them all.  The additions are ceil(T D / 64)
    per lane plus the 6 levels of the butterfly, each one rounding of a partial sum of non-negative terms; the halving is exact.  First
    order in u, times 1 + 2^-10."""
    T, D = y.shape[1], y.shape[2]
    depth = -(-T * D // 64) + 6
    return (8 + depth) * U * cost(y, G) * (1.0 + 2.0 ** -10)
