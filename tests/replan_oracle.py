"""float64 restatement of warm-started replanning, built from oracle.np64's own pieces: the planner loop over a range of
executed steps and the warm initial state.  Step i of a range is step i of np64.planner_sample -- the same timestep, the same noise row."""
import math

import numpy as np

from oracle import np64

F64 = np.float64


def step_timestep(i, n_train, n_steps, sampler):
    """The training timestep executed step i visits (np64.planner_sample's k)."""
    return n_train - 1 - i if sampler == "ddpm" else (n_steps - 1 - i) * (n_train // n_steps)


def planner_range(params, cond, x, begin, end, step_noise=None, n_train=100, n_steps=100, sampler="ddpm", **unet_kw):
    """np64.planner_sample restricted to the executed steps [begin, end): x is the state in front of step `begin`."""
    assert 0 <= begin <= end <= n_steps
    tables = np64.ddpm_tables(n_train)
    x = np.asarray(x, F64)
    stride = n_train // n_steps
    for i in range(begin, end):
        k = step_timestep(i, n_train, n_steps, sampler)
        eps = np64.unet_forward(params, x, k, cond, **unet_kw)
        if sampler == "ddpm":
            assert n_steps == n_train
            x = np64.ddpm_step(eps, k, x, step_noise[i] if k > 0 else 0.0, tables)
        elif sampler == "ddim":
            x = np64.ddim_step(eps, k, k - stride, x, tables)
        else:
            raise ValueError(sampler)
    return x


def shift_hold(x_prev, shift):
    """xs[b, j] = x_prev[b, min(j + shift, T-1)]: the plan moved by `shift` positions, its last state held."""
    x_prev = np.asarray(x_prev)
    T = x_prev.shape[1]
    return x_prev[:, np.minimum(np.arange(T) + int(shift), T - 1)]


def warm_coefs(t, n_train=100):
    """(sqrt(abar_t), sqrt(1 - abar_t)) in float64 from the float32 abar table (ddpm_add_noise's coefficients)."""
    a_t = F64(np64.ddpm_tables(n_train)[2][t])
    return math.sqrt(a_t), math.sqrt(1.0 - a_t)


def warm_init(x_prev, shift, t, eps, n_train=100):
    """sqrt(abar_t) * shift_hold(x_prev) + sqrt(1 - abar_t) * eps, through np64.ddpm_add_noise."""
    xs = np.asarray(shift_hold(x_prev, shift), F64)
    return np64.ddpm_add_noise(xs, np.asarray(eps, F64), np.full(xs.shape[0], int(t)), np64.ddpm_tables(n_train))
