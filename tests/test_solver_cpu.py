"""The host side of the DPM-Solver++(2M) sampler: schedule.solver_timesteps / solver_coefficients, and the float64 oracle
tests/solver_oracle.py on the analytic Gaussian experiment the sampler's case rests on.  No GPU."""
import math

import numpy as np
import pytest

from latent_diffusion_planning_amd import schedule as S
from tests import solver_oracle as SO

N_TRAIN = 100


def test_known_tables():
    assert S.solver_timesteps(100, 10).tolist() == [90, 82, 70, 51, 32, 17, 9, 4, 1, 0]
    assert S.solver_timesteps(100, 5).tolist() == [80, 48, 16, 4, 0]
    assert S.solver_timesteps(100, 10).dtype == np.int64
    assert S.solver_timesteps(100, 10, "uniform").tolist() == [90, 80, 70, 60, 50, 40, 30, 20, 10, 0]
    assert S.solver_timesteps(100, 100).tolist() == list(range(99, -1, -1))
    assert S.solver_timesteps(100, 4, t_first=3).tolist() == [3, 2, 1, 0]


def test_value_errors():
    with pytest.raises(ValueError, match="uniform"):
        S.solver_timesteps(100, 7, "uniform")
    with pytest.raises(ValueError, match="spacing"):
        S.solver_timesteps(100, 10, "cosine")
    with pytest.raises(ValueError, match="t_first"):
        S.solver_timesteps(100, 10, t_first=8)              # ten distinct timesteps do not fit into 8 .. 0
    with pytest.raises(ValueError, match="t_first"):
        S.solver_timesteps(100, 10, t_first=100)
    with pytest.raises(ValueError, match="n_steps"):
        S.solver_timesteps(100, 0)
    with pytest.raises(ValueError):
        S.solver_timesteps(100, 101)


@pytest.mark.parametrize("n", range(1, 92))
def test_table_properties(n):
    ts = S.solver_timesteps(N_TRAIN, n)
    assert ts.shape == (n,) and ts[0] == N_TRAIN - max(1, N_TRAIN // n) and ts[-1] == 0
    assert (np.diff(ts) < 0).all()


@pytest.mark.parametrize("n,spacing", [(5, "logsnr"), (10, "logsnr"), (20, "logsnr"), (91, "logsnr"), (10, "uniform"), (1, "logsnr")])
def test_coefficients_against_the_exponential_form(n, spacing):
    """schedule.solver_coefficients (quotients of alpha and sigma) against tests/solver_oracle.coefficients (-alpha_s expm1(-h)): two float64
    evaluations that agree far below the float32 cast, so the cast rows are within half a float32 ulp (2^-24 relative) of the oracle's."""
    sched = S.make_schedule(N_TRAIN)
    ts = S.solver_timesteps(N_TRAIN, n, spacing)
    got, got64, want = S.solver_coefficients(sched, ts), S.solver_coefficients(sched, ts, dtype=np.float64), SO.coefficients(ts, N_TRAIN)
    assert got.dtype == np.float32 and got.shape == (n, 8) and (got[:, 6:] == 0).all()
    assert np.allclose(got64[:, :6], want, rtol=1e-12, atol=0)
    assert (np.abs(got[:, :6].astype(np.float64) - want) <= 2.0 ** -24 * np.abs(want) * (1 + 1e-9)).all()
    assert np.array_equal(got[:, 0], ts.astype(np.float32))
    assert got[0, 5] == 0 and got[-1, 5] == 0 and got[-1, 3] == 0 and got[-1, 4] == 1
    if n > 2:
        assert (got[1:-1, 5] > 0).all()


def test_first_order_row_is_ddim():
    """c_x x + c_D x0 with eps re-derived from an unclipped x0 is DDIM's sqrt(abar_s) x0 + sqrt(1 - abar_s) eps, to 1e-12; on the uniform grid
    the pair (sqrt(abar_s), sqrt(1 - abar_s)) is what schedule.step_coefficients holds in float32."""
    sched = S.make_schedule(N_TRAIN)
    ac = sched.alphas_cumprod.astype(np.float64)
    g = np.random.default_rng(5)
    x, x0 = g.standard_normal(64), g.uniform(-3, 3, 64)
    for spacing in ("logsnr", "uniform"):
        ts = S.solver_timesteps(N_TRAIN, 10, spacing)
        rows = S.solver_coefficients(sched, ts, dtype=np.float64)
        for i, t in enumerate(ts):
            a_s = ac[ts[i + 1]] if i + 1 < len(ts) else 1.0
            eps = (x - math.sqrt(ac[t]) * x0) / math.sqrt(1.0 - ac[t])
            want = math.sqrt(a_s) * x0 + math.sqrt(1.0 - a_s) * eps
            assert np.abs(rows[i, 3] * x + rows[i, 4] * x0 - want).max() <= 1e-12, (spacing, i)
    ddim = S.step_coefficients(sched, 10, S.SAMPLER_DDIM).astype(np.float64)
    assert np.allclose(rows[:, 3] * rows[:, 2], ddim[:, 5], rtol=1e-7, atol=1e-9)                 # sigma_s
    assert np.allclose(rows[:, 4] + rows[:, 3] / rows[:, 1], ddim[:, 3], rtol=1e-7)               # alpha_s = c_D + c_x alpha_t


# figures of the experiment (data N(0, 0.3^2), x_T uniform in [-2, 2], relative RMS error against the closed-form solution)
FIGURES = {5: (0.259, 0.0150), 10: (0.147, 0.0157), 20: (0.084, 0.0013)}


@pytest.mark.parametrize("n", [5, 10, 20])
def test_gaussian_experiment(n):
    ts = S.solver_timesteps(N_TRAIN, n)
    x_t = np.random.default_rng(0).uniform(-2.0, 2.0, (3, 8, 25))
    ddim, two_m = SO.gaussian_errors(ts, 0.3, x_t)
    print(f"n = {n}: DDIM {ddim:.4f}, 2M {two_m:.4f}, ratio {two_m / ddim:.3f}")
    assert f"{ddim:.2g}" == f"{FIGURES[n][0]:.2g}" and f"{two_m:.2g}" == f"{FIGURES[n][1]:.2g}"
    assert two_m <= 0.25 * ddim                                      # the condition the GPU test asserts on the same grid
    # the x0 clip is never active in this experiment
    f = SO.gaussian_eps(0.3)
    assert np.abs(SO.solve(f, x_t, ts) - SO.solve(f, x_t, ts, clip=False)).max() == 0
    # and the solver's gain needs the grid: on the uniform one it does not reach the condition
    if N_TRAIN % n == 0:
        d_u, m_u = SO.gaussian_errors(S.solver_timesteps(N_TRAIN, n, "uniform"), 0.3, x_t)
        assert m_u > 0.25 * d_u and two_m < 0.25 * m_u
