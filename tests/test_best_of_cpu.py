"""Best-of-N planning without a GPU: the float64 oracle (tests/best_of_oracle.py) against hand-computed cases, the candidate-major
index arithmetic the shards rely on, and the argument checks the engine wrappers make before a pointer crosses the C ABI."""
import numpy as np
import pytest

from latent_diffusion_planning_amd.dist import shard_bounds
from latent_diffusion_planning_amd.engine import check_candidate_range
from tests import best_of_oracle as O


def test_density_costs_of_three_points_by_hand():
    """x = (0,0), (1,0), (0,2): d2 = 1, 4, 5; Var = 2/9 + 8/9, so m = 20/9 (= (2 * 10) / 9 ordered pairs) and 2 h2 = 10/9 at bandwidth 0.5."""
    x = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 2.0]])
    assert abs(O.mean_sq_distance(x) - 20.0 / 9.0) < 1e-15
    e = lambda d2: np.exp(-d2 * 0.9)                                   # noqa: E731
    want = -np.array([1 + e(1) + e(4), 1 + e(1) + e(5), 1 + e(4) + e(5)])
    np.testing.assert_allclose(O.density_costs(x, 0.5), want, rtol=1e-14)
    assert O.argmin(O.density_costs(x, 0.5)) == 0
    # twice the bandwidth = a quarter of the exponent
    np.testing.assert_allclose(O.density_costs(x, 1.0), -np.array([1 + e(.25) + e(1), 1 + e(.25) + e(1.25), 1 + e(1) + e(1.25)]), rtol=1e-14)


def test_argmin_ties_nan_and_all_nan():
    assert O.argmin([3.0, 1.0, 1.0, 2.0]) == 1                         # ties: the lowest index
    assert O.argmin([np.nan, 5.0, np.nan, 4.0]) == 3                   # a NaN compares as +inf
    assert O.argmin([np.nan, np.inf, 7.0]) == 2
    assert O.argmin([np.nan, np.nan, np.nan]) == 0                     # all NaN: candidate 0
    assert O.argmin([np.inf, np.nan]) == 0
    assert O.argmin([-np.inf, -np.inf]) == 0


def test_equal_candidates_cost_minus_n_without_a_division():
    x = np.tile(np.arange(6.0), (4, 1))
    assert O.mean_sq_distance(x) == 0
    with np.errstate(all="raise"):
        c = O.density_costs(x, 0.5)
    assert np.array_equal(c, np.full(4, -4.0)) and O.argmin(c) == 0
    assert np.array_equal(O.density_costs(np.ones((1, 9))), [-1.0])   # N = 1


def test_goal_costs_by_hand():
    x = np.arange(2 * 3 * 2, dtype=np.float64).reshape(2, 3, 2)        # rows (t) of candidate 0: (0,1) (2,3) (4,5); candidate 1: + 6
    assert np.array_equal(O.goal_costs(x, [4.0, 4.0]), [1.0, 36 + 49])
    assert np.array_equal(O.goal_costs(x, [4.0, 4.0], weight=[0.0, 2.0], t_goal=0), [2 * 9.0, 2 * 9.0])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_bandwidth_half_finds_the_majority_mode_and_one_finds_the_midpoint(seed):
    """Why the default is 0.5: 27 + 18 candidates in two modes and 5 half way between them, K = 200."""
    x, label = O.two_modes(200, seed)
    for bw, want in ((0.25, 0), (0.5, 0), (1.0, 2), (4.0, 2)):
        assert label[O.argmin(O.density_costs(x, bw))] == want, bw
    assert label[np.argmin(((x - x.mean(0)) ** 2).sum(-1))] == 2       # nearest-to-the-mean picks a plan that lies in neither mode


def test_candidate_major_rows():
    B, N = 3, 5
    r = np.arange(N * B)
    assert np.array_equal(r % B, np.tile(np.arange(B), N))             # row r is conditioned on observation r mod B
    assert all(O.row(c, b, B) == c * B + b and O.row(c, b, B) // B == c for c in range(N) for b in range(B))
    assert [O.row(0, b, B) for b in range(B)] == [0, 1, 2]             # N = 1: row b is sample()'s row b
    x = r.reshape(N * B, 1) * 1.0
    assert np.array_equal(O.of_observation(x, 1, B)[:, 0], [1, 4, 7, 10, 13])
    assert np.array_equal(x.reshape(N, B, 1).transpose(1, 0, 2)[1, :, 0], O.of_observation(x, 1, B)[:, 0])     # the (B, N, ...) view of the metrics


@pytest.mark.parametrize("n,world", [(37, 2), (8192, 8), (5, 8), (1, 1), (64, 3)])
def test_candidate_shards_are_contiguous_row_ranges_that_concatenate(n, world):
    B = 2
    rows = []
    for r in range(world):
        c0, c1 = shard_bounds(n, world, r)
        rows += list(range(c0 * B, c1 * B))                            # candidates [c0, c1) = rows [c0 B, c1 B)
    assert rows == list(range(n * B))
    assert shard_bounds(37, 2, 0) == (0, 19) and shard_bounds(37, 2, 1) == (19, 37)


def test_wrapper_argument_checks_name_the_argument():
    check_candidate_range(2, 5, 200)
    check_candidate_range(2, 5, 200, c0=3, n_loc=2, bandwidth=0.5)
    for kw, word in ((dict(B=0, N=5, K=8), "B"), (dict(B=1, N=0, K=8), "n_candidates"), (dict(B=1, N=5, K=0), "K"),
                     (dict(B=1, N=5, K=8, c0=3, n_loc=3), "c0"), (dict(B=1, N=5, K=8, c0=-1, n_loc=2), "c0"),
                     (dict(B=1, N=5, K=8, c0=0, n_loc=0), "n_loc"), (dict(B=1, N=5, K=8, bandwidth=0.0), "bandwidth"),
                     (dict(B=1, N=5, K=8, bandwidth=-1.0), "bandwidth"), (dict(B=1, N=5, K=8, bandwidth=float("nan")), "bandwidth"),
                     (dict(B=1, N=5, K=8, bandwidth=float("inf")), "bandwidth")):
        with pytest.raises(ValueError, match=word):
            check_candidate_range(**kw)


def test_the_library_refuses_bad_arguments_without_a_gpu():
    """The stand-alone calls check their arguments before any HIP call: LDP_EINVAL and a message naming the argument."""
    import ctypes as C
    import os

    from latent_diffusion_planning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libldp_hip.so not built")
    lib = _lib.load()
    p = C.c_void_p(256)                                                # never dereferenced: the checks come first
    for args, word in (((p, 1, 0, 8, 0, 1, C.c_float(0.5), p, None), b"N "), ((p, 1, 5, 8, 3, 3, C.c_float(0.5), p, None), b"c0 + n_loc"),
                       ((p, 1, 5, 0, 0, 5, C.c_float(0.5), p, None), b"K "), ((p, 1, 5, 8, 0, 5, C.c_float(0.0), p, None), b"bandwidth"),
                       ((p, 1, 5, 8, 0, 5, C.c_float(float("nan")), p, None), b"bandwidth"), ((p, 0, 5, 8, 0, 5, C.c_float(0.5), p, None), b"B ")):
        assert lib.ldp_plan_cost_density(*args) == -1 and word in lib.ldp_last_error(), (args, lib.ldp_last_error())
    assert lib.ldp_plan_select(p, p, 1, 0, 8, p, p, p, None) == -1 and b"N " in lib.ldp_last_error()
    assert lib.ldp_plan_cost_goal(p, 1, 2, 8, 25, 8, p, p, p, None) == -1 and b"t_goal" in lib.ldp_last_error()
    assert lib.ldp_plan_candidates(None, p, 1, 1, 1, 0, 1, None, None, 0, 0, 100, p, 1, None) == -1
