"""float64 restatement of composed planning on the pieces of tests/guide_oracle.py, tests/solver_oracle.py and
tests/constrain_oracle.py: the composed step -- data prediction, guide, scheduler or solver update, constraint, in that order -- and the
composed loop over a range of executed steps; next to it the float32 emulation of csrc/compose.hip's arithmetic, rounding for rounding
(on guide_oracle's exact fma), and the error bound its spelled roundings imply.

A coefficient row is a dict(t, s, inv_a, c_y, c_x, c_eps, sigma, w): s / inv_a of the data prediction; DDPM / DDIM: c_y = c_x0, c_x,
c_eps, sigma; "dpmpp": c_y = c_D, c_x, w.  A guide is guide_oracle's dict (or None).  A constraint is dict(target, mask (B, T, D), a, s,
z (B, T, D) or None): the values of level i + 1 -- z None means the select writes target itself (clamp, and every mode at level n).
Layout (B, T, D) throughout."""
import numpy as np

from latent_diffusion_planning_amd import schedule
from oracle import np64
from tests import constrain_oracle as CO, guide_oracle as GO, replan_oracle as RO, solver_oracle as SO
from tests.guide_oracle import F32, F64, U, fma32

KEYS = ("t", "s", "inv_a", "c_y", "c_x", "c_eps", "sigma", "w")


def step_row(sampler, i, n_train, n_steps, ts=None, cast32=False, quotient=True):
    """The coefficient row of executed step i.  DDPM / DDIM: guide_oracle.step_coefs.  "dpmpp" over the table ts: the rows of
    schedule.solver_coefficients (quotient=True: what the kernel holds, in float64 or cast to float32) or solver_oracle.coefficients (the
    exp(-h) form the float64 loops use)."""
    if sampler == "dpmpp":
        if quotient:
            r = schedule.solver_coefficients(schedule.make_schedule(n_train), ts, dtype=np.float32 if cast32 else np.float64)[i]
        else:
            r = SO.coefficients(ts, n_train)[i]
        return dict(t=float(r[0]), s=float(r[2]), inv_a=float(r[1]), c_y=float(r[4]), c_x=float(r[3]), c_eps=0.0, sigma=0.0, w=float(r[5]))
    t, inv_a, sg, c_x0, c_x, c_eps, sigma = GO.step_coefs(i, n_train, n_steps, sampler, cast32=cast32)
    return dict(t=t, s=sg, inv_a=inv_a, c_y=c_x0, c_x=c_x, c_eps=c_eps, sigma=sigma, w=0.0)


def level_coefs(level, sampler, n_train, n_steps, ts=None):
    """(a_j, s_j) of constraint level j in float64: constrain_oracle.level_coefs on the uniform grid, the entry ts[j] of the table under
    "dpmpp"; level n is exactly (1, 0)."""
    if sampler != "dpmpp":
        return CO.level_coefs(level, n_train, n_steps, sampler)
    assert 0 <= level <= len(ts)
    return (1.0, 0.0) if level == len(ts) else RO.warm_coefs(int(ts[level]), n_train)


def constraint(target, mask, mode, level, sampler, n_train, n_steps, ts=None, z=None, cast32=False):
    """The constraint dict of `level` (= executed step + 1): z is read only under 'repaint' below level n."""
    a, s = level_coefs(level, sampler, n_train, n_steps, ts)
    if cast32:
        a, s = float(F32(a)), float(F32(s))
    noisy = mode == "repaint" and level < n_steps
    return dict(target=target, mask=np.asarray(mask) != 0, a=a, s=s, z=z if noisy else None)


def compose_step(x, eps, k, G=None, rho=0.0, z=None, h_prev=None, second=False, cons=None, solver=False):
    """One composed step in float64 -> (x', y'): y' is the guided data prediction (the solver's next history)."""
    x, eps = np.asarray(x, F64), np.asarray(eps, F64)
    y = np.clip((x - k["s"] * eps) * k["inv_a"], -1.0, 1.0)
    yg = y if G is None else GO.project(y, G, rho)
    if solver:
        d = yg + k["w"] * (yg - np.asarray(h_prev, F64)) if second else yg
        out = k["c_x"] * x + k["c_y"] * d
    else:
        out = k["c_y"] * yg + k["c_x"] * x + k["c_eps"] * eps
        if k["sigma"] != 0.0:
            out = out + k["sigma"] * np.asarray(z, F64)
    if cons is not None:
        tg = np.asarray(cons["target"], F64)
        v = tg if cons["z"] is None else cons["a"] * tg + cons["s"] * np.asarray(cons["z"], F64)
        out = np.where(cons["mask"], v, out)                # a select
    return out, yg


def emulate_step(x, eps, k, G=None, rho=0.0, z=None, h_prev=None, second=False, cons=None, solver=False):
    """plan_compose_step_kernel's (x', y') bit for bit: every input float32, k the float32 coefficient row."""
    x, eps = np.asarray(x, F32), np.asarray(eps, F32)
    c = {n: F32(k[n]) for n in KEYS}
    one = F32(1.0)
    y = np.clip(fma32(-c["s"], eps, x) * c["inv_a"], -one, one)
    yg = y
    if G is not None:
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
    if solver:
        d = fma32(c["w"], yg - np.asarray(h_prev, F32), yg) if second else yg
        v = fma32(c["c_x"], x, c["c_y"] * d)
    else:
        v = fma32(c["c_eps"], eps, fma32(c["c_x"], x, c["c_y"] * yg))
        if c["sigma"] != 0:
            v = fma32(c["sigma"], np.asarray(z, F32), v)
    if cons is not None:
        tg = np.asarray(cons["target"], F32)
        w = tg if cons["z"] is None else fma32(F32(cons["a"]), tg, F32(cons["s"]) * np.asarray(cons["z"], F32))
        v = np.where(cons["mask"], w, v)
    assert v.dtype == F32 and yg.dtype == F32
    return v, yg


def step_bound(x, eps, k, G=None, rho=0.0, z=None, h_prev=None, second=False, cons=None, solver=False):
    """|kernel - compose_step(the float32 coefficients)| <= (bound of x', bound of y'), elementwise, from the kernel's spelled roundings:
    first order in u = 2^-24, times 1 + 2^-10 for the higher orders.  clip and max(., 0) are 1-Lipschitz.
      y:    two roundings, e_y = 2u |(x - s eps) inv_a|
      y':   guide_oracle.step_bound's chain: rho e_g + e_y + u |y - rho g|;  without a guide y' = y and e_y' = e_y
      DDPM / DDIM:  |c_y| e_y' + u (|m1| + |m2| + |m3| + |m4|), the partial sums of the update in the kernel's order
      "dpmpp":      e_D = second ? |w| (e_y' + u |y' - h|) + e_y' + u |Dv| : e_y'   (the history is an input: exact);
                    |c_y| e_D + u |c_y Dv| + u |x'|
      constraint:   clamp writes target itself: 0;  repaint: u (|s z| + |a target + s z|)."""
    x, eps = np.asarray(x, F64), np.asarray(eps, F64)
    raw = (x - k["s"] * eps) * k["inv_a"]
    y = np.clip(raw, -1.0, 1.0)
    e_y = 2.0 * U * np.abs(raw)
    if G is None:
        yg, e_yg = y, e_y
    else:
        G = GO._g64(G)
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
    if solver:
        if second:
            diff = yg - np.asarray(h_prev, F64)
            d = yg + k["w"] * diff
            e_d = abs(k["w"]) * (e_yg + U * np.abs(diff)) + e_yg + U * np.abs(d)
        else:
            d, e_d = yg, e_yg
        m1 = k["c_y"] * d
        out = abs(k["c_y"]) * e_d + U * (np.abs(m1) + np.abs(m1 + k["c_x"] * x))
    else:
        m1 = k["c_y"] * yg
        m2 = m1 + k["c_x"] * x
        m3 = m2 + k["c_eps"] * eps
        m4 = m3 + (k["sigma"] * np.asarray(z, F64) if k["sigma"] != 0.0 else 0.0)
        out = abs(k["c_y"]) * e_yg + U * (np.abs(m1) + np.abs(m2) + np.abs(m3) + (np.abs(m4) if k["sigma"] != 0.0 else 0.0))
    if cons is not None:
        if cons["z"] is None:
            b = np.zeros_like(out)
        else:
            sz = cons["s"] * np.asarray(cons["z"], F64)
            b = U * (np.abs(sz) + np.abs(cons["a"] * np.asarray(cons["target"], F64) + sz))
        out = np.where(cons["mask"], b, out)
    hi = 1.0 + 2.0 ** -10
    return out * hi, e_yg * hi


def composed_loop(eps_fn, x, begin, end, sampler="ddim", n_train=100, n_steps=100, ts=None, G=None, rho=None, target=None, mask=None,
                  mode="repaint", step_noise=None, seed=0, row_offset=0, dp=CO.DP):
    """The composed loop over the executed steps [begin, end) in float64: eps_fn(x, t) -> eps.  x <- C_begin(x) with a constraint; then
    the composed step per executed step.  Under "dpmpp" (table ts, the exp(-h) rows of solver_oracle) the history is empty at `begin`:
    step i is second order iff i > begin and i < n - 1."""
    x = np.asarray(x, F64)
    solver = sampler == "dpmpp"
    B, T, D = x.shape

    def cons_at(level):
        if target is None:
            return None
        z = CO.level_noise(seed, row_offset, B, T, D, level, dp) if mode == "repaint" and level < n_steps else None
        return constraint(target, mask, mode, level, sampler, n_train, n_steps, ts, z)
    if target is not None:
        c = cons_at(begin)
        tg = np.asarray(target, F64)
        x = np.where(c["mask"], tg if c["z"] is None else c["a"] * tg + c["s"] * c["z"], x)
    h = None
    for i in range(begin, end):
        k = step_row(sampler, i, n_train, n_steps, ts, quotient=False)
        eps = eps_fn(x, int(k["t"]))
        x, h = compose_step(x, eps, k, G, 0.0 if rho is None else float(rho[i]), None if step_noise is None else step_noise[i], h,
                            solver and i > begin and i < n_steps - 1, cons_at(i + 1), solver)
    return x


def planner_range_composed(params, cond, x, begin, end, **kw):
    """composed_loop on np64's U-Net."""
    return composed_loop(lambda xx, t: np64.unet_forward(params, xx, t, cond), x, begin, end, **kw)
