"""float64 restatement of constrained planning, built from oracle.np64's pieces, oracle.philox and tests/replan_oracle:
the level coefficients, the constraint operation C_j and the constrained loop over a range of executed steps.

A loop of n executed steps has the levels 0 .. n: level j is the state in front of executed step j, level n the result.  C_j replaces
x[b, t, c] where mask != 0 -- by target (clamp, and every mode at level n) or by a_j target + s_j z_j (repaint) -- and the loop over
[begin, end) is  x <- C_begin(x);  for i in begin .. end-1:  x <- C_{i+1}(step_i(x))."""
import numpy as np

from oracle import np64, philox
from tests import replan_oracle as RO

F64 = np.float64
STREAM_CONSTRAIN = 12         # include/ldp_hip.h LDP_PHILOX_STREAM_CONSTRAIN
DP = 32                       # the padded row width the element index of a draw is stated in (rm_lift: D = 25 -> 32)


def level_coefs(level, n_train, n_steps, sampler):
    """(a_j, s_j) in float64 from the float32 abar table; level n_steps is exactly (1, 0)."""
    assert 0 <= level <= n_steps
    if level == n_steps:
        return 1.0, 0.0
    return RO.warm_coefs(RO.step_timestep(level, n_train, n_steps, sampler), n_train)


def level_noise(seed, row_offset, B, T, D, level, dp=DP):
    """z_j (B, T, D): element ((row_offset + b) * T + t) * dp + c, step = level, stream 12 -- float64 Box-Muller of the same words."""
    z = philox.normal(seed, row_offset * T * dp, level, STREAM_CONSTRAIN, B * T * dp)
    return z.reshape(B, T, dp)[:, :, :D]


def constrain(x, target, mask, level, mode, n_train=100, n_steps=100, sampler="ddpm", seed=0, row_offset=0, z=None, cast32=False):
    """C_level(x).  z: the draws to use (e.g. read back from the device), else level_noise.  cast32: the coefficients cast to float32
    first, as the kernel holds them."""
    x = np.asarray(x, F64)
    on = np.asarray(mask) != 0
    tg = np.asarray(target, F64)
    if mode == "clamp" or level == n_steps:
        v = tg
    elif mode == "repaint":
        a, s = level_coefs(level, n_train, n_steps, sampler)
        if cast32:
            a, s = float(np.float32(a)), float(np.float32(s))
        if z is None:
            z = level_noise(seed, row_offset, x.shape[0], x.shape[1], x.shape[2], level)
        v = a * tg + s * np.asarray(z, F64)
    else:
        raise ValueError(mode)
    return np.where(on, v, x)                       # a select: a NaN in target under a zero mask never reaches the state


def planner_range_constrained(params, cond, x, begin, end, target, mask, mode, step_noise=None, n_train=100, n_steps=100, sampler="ddpm",
                              seed=0, row_offset=0, **unet_kw):
    """The constrained loop over the executed steps [begin, end): replan_oracle.planner_range one step at a time, C behind each."""
    kw = dict(n_train=n_train, n_steps=n_steps, sampler=sampler)
    x = constrain(x, target, mask, begin, mode, seed=seed, row_offset=row_offset, **kw)
    for i in range(begin, end):
        x = RO.planner_range(params, cond, x, i, i + 1, step_noise=step_noise, **kw, **unet_kw)
        x = constrain(x, target, mask, i + 1, mode, seed=seed, row_offset=row_offset, **kw)
    return x
