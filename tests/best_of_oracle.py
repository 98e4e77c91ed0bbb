"""Best-of-N planning as DESIGN.md 4.14 defines it, in numpy float64: the oracle of tests/test_best_of_cpu.py and tests/test_hip_best_of.py.
One observation at a time: x (N, K) are its N candidates; candidate-major rows of B observations are row(c, b, B) = c * B + b."""
import numpy as np


def row(c, b, B):
    return c * B + b


def of_observation(x_all, b, B):
    """The (N, ...) candidates of observation b out of candidate-major rows (N * B, ...)."""
    return np.asarray(x_all)[b::B]


def mean_sq_distance(x):
    """m_b = 2 sum_k Var_k (biased) = the mean of d2 over all N^2 ordered pairs."""
    x = np.asarray(x, np.float64).reshape(len(x), -1)
    return 2.0 * x.var(axis=0).sum()


def density_costs(x, bandwidth=0.5):
    x = np.asarray(x, np.float64).reshape(len(x), -1)
    m = mean_sq_distance(x)
    if m == 0:
        return np.full(len(x), -float(len(x)))
    d2 = np.stack([((xi - x) ** 2).sum(-1) for xi in x])            # direct differences, row by row (N x N, never N x N x K at once)
    return -np.exp(-d2 / (2.0 * bandwidth ** 2 * m)).sum(-1)


def goal_costs(x, goal, weight=None, t_goal=-1):
    """x (N, T, D), goal (D,), weight (D,) -> (N,)."""
    x, goal = np.asarray(x, np.float64), np.asarray(goal, np.float64)
    w = np.ones_like(goal) if weight is None else np.asarray(weight, np.float64)
    return (w * (x[:, t_goal] - goal) ** 2).sum(-1)


def argmin(costs):
    """Lowest cost, ties to the lowest index, NaN as +inf (all NaN: 0)."""
    c = np.asarray(costs, np.float64)
    return int(np.argmin(np.where(np.isnan(c), np.inf, c)))


def two_modes(K=200, seed=0):
    """27 candidates around one plan, 18 around another, 5 half way between them (each with isotropic noise): (x (50, K), labels) with
    label 0 = majority mode, 1 = minority mode, 2 = midpoint."""
    g = np.random.Generator(np.random.PCG64(seed))
    u = g.standard_normal(K)
    u /= np.linalg.norm(u)
    centre = np.concatenate([np.full(27, 1.0), np.full(18, -1.0), np.zeros(5)])
    labels = np.concatenate([np.zeros(27, int), np.ones(18, int), np.full(5, 2)])
    x = centre[:, None] * u[None, :] * TWO_MODES_HALF_GAP + TWO_MODES_SIGMA * g.standard_normal((50, K))
    p = g.permutation(50)
    return x[p], labels[p]


TWO_MODES_HALF_GAP, TWO_MODES_SIGMA = 1.0, 0.05
