"""The reach2d task on the host: known answers of the NumPy restatement (tests/toyenv_oracle.py) the kernels are held to, the task's own
conditions under the Philox draws (the expert solves it, a straight line mostly does not, random actions never do) and
harness.run_device_eval on the NumPy environment with a scripted stand-in for the policy.  No GPU."""
import numpy as np
import pytest

from latent_diffusion_planning_amd import harness
from tests import toyenv_oracle as O

F32 = np.float32
N_TASK = 4096


def _state(px, py, gx=0.8, gy=0.0, side=1.0):
    return np.array([[px, py, gx, gy, side, 0, 0, 0]], F32)


# ---- the library's C ABI ---------------------------------------------------------------------------------------------------------------
def test_env_header_binding_and_library_list_the_same_symbols():
    """libldp_env.so is a library of its own: include/ldp_env.h, _envlib.SIGNATURES and its dynamic symbol table agree, and the agent's
    library exports none of it (tests/test_abi.py holds libldp_hip.so to include/ldp_hip.h)."""
    import os
    import subprocess
    from latent_diffusion_planning_amd import _envlib, _lib
    syms = _envlib.header_symbols()
    assert syms == sorted(_envlib.SIGNATURES) == ["ldp_env_last_error", "ldp_env_observe", "ldp_env_reset", "ldp_env_step"]
    assert not set(syms) & set(_lib.SIGNATURES)
    with open(os.path.join(os.path.dirname(_envlib.LIB_PATH), "csrc", "Makefile")) as f:
        assert "libldp_env.so" in f.read()
    if os.path.exists(_envlib.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", _envlib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert sorted(line.split()[-1] for line in out.splitlines() if line.strip()) == syms
        lib = _envlib.load()
        assert lib.ldp_env_reset(None, 4, 0, 0, None) == -1 and b"null state" in lib.ldp_env_last_error()      # refused before any HIP call
        with pytest.raises(_lib.LDPHipError, match="N must be"):
            _envlib.check(lib.ldp_env_step(1 << 20, 0, 1, None, 2, 1, 0.0, 0, 0, None, None, None, None, None))


def test_a_missing_env_library_fails_loudly(monkeypatch, tmp_path):
    from latent_diffusion_planning_amd import _envlib, _lib
    monkeypatch.setattr(_envlib, "_lib", None)
    monkeypatch.setattr(_envlib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.LDPHipUnavailable, match="no other implementation"):
        _envlib.load()


# ---- known answers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u, want", [(0.0, [0, -1, 0, 1]), (0.5, [0.5, -0.5, -1, -0.5]), (-0.5, [-0.5, -0.5, 1, -0.5]),
                                     (1.0, [1, 1, 1, 1]), (-1.0, [-1, 1, -1, 1])])
def test_chebyshev_known_values(u, want):
    assert O.chebyshev(F32(u)).tolist() == [float(v) for v in want]


def test_observation_layout():
    s = _state(-0.5, 0.5, gx=0.5, gy=-0.5)
    pos, goal, lat = O.observe(s)
    assert pos.tolist() == [[-0.5, 0.5]] and goal.tolist() == [[0.5, -0.5]]
    want = np.concatenate([O.chebyshev(F32(-0.5)), O.chebyshev(F32(0.5)), O.chebyshev(F32(0.5)), O.chebyshev(F32(-0.5))])
    assert lat.shape == (1, 16) and np.array_equal(lat[0], want)
    assert np.abs(lat).max() <= 1


def test_reset_follows_the_philox_words():
    from oracle import philox
    s = O.reset(5, seed=77, episode0=1000)
    w = philox.words(77, 1000, 0, O.STREAM_ENV, 5)
    assert np.array_equal(s[:, O.PY], F32(-0.5) + (w[:, 0] >> 8).astype(F32) * F32(2.0 ** -24))
    assert np.array_equal(s[:, O.SIDE], np.where(w[:, 2] & 1, 1, -1).astype(F32))
    assert np.all(s[:, O.PX] == F32(-0.8)) and np.all(s[:, O.GX] == F32(0.8)) and np.all(s[:, 5:] == 0)
    assert np.all((s[:, O.GY] >= -0.5) & (s[:, O.GY] < 0.5))
    assert np.array_equal(O.reset(8, 77, 997)[3:], s)                             # episode0 keys the episode, not the batch


def test_a_move_into_the_disc_is_refused_and_counted():
    s = _state(-0.32, 0.0)
    O.step(s, 2, actions=np.array([[[1.0, 0.0], [0.0, 1.0]]], F32))
    # the first move would end at x = -0.24, inside R = 0.3: p stays; the second (0, +0.08) is outside and is taken
    assert s[0, O.PX] == F32(-0.32) and s[0, O.PY] == O.fma32(O.DT, F32(1), F32(0)) and s[0, O.BLOCKED] == 1 and s[0, O.T] == 2


def test_the_disc_boundary_is_not_inside():
    """A point with qx^2 + qy^2 >= R^2 (here: exactly R on the axis, R^2 = rn(R * R) by definition) is free."""
    s = _state(0.3, 0.0)
    O.step(s, 1, actions=np.zeros((1, 1, 2), F32))
    assert s[0, O.BLOCKED] == (1 if O.fma32(F32(0.3), F32(0.3), F32(0)) < O.R2 else 0) == 0


def test_walls_clamp_the_position():
    s = _state(0.97, -0.97)
    O.step(s, 1, actions=np.array([[[1.0, -1.0]]], F32))
    assert s[0, O.PX] == 1 and s[0, O.PY] == -1 and s[0, O.BLOCKED] == 0


def test_nan_and_out_of_range_actions():
    a = np.array([[[np.nan, 3.0], [-3.0, np.nan], [np.inf, -np.inf]]], F32)
    s, ref = _state(-0.8, 0.6), _state(-0.8, 0.6)
    taken = O.step(s, 3, actions=a)[0]
    assert taken[0].tolist() == [[0, 1], [-1, 0], [1, -1]]
    O.step(ref, 3, actions=np.array([[[0, 1], [-1, 0], [1, -1]]], F32))
    assert np.array_equal(s, ref)


def test_only_two_components_are_read():
    a = np.zeros((1, 2, 7), F32)
    a[0, :, :2], a[0, :, 2:] = [[0.5, -0.25], [1, 1]], np.nan
    s, ref = _state(-0.8, 0.0), _state(-0.8, 0.0)
    taken = O.step(s, 2, actions=a)[0]
    O.step(ref, 2, actions=a[:, :, :2].copy())
    assert np.array_equal(s, ref) and taken.shape == (1, 2, 7) and np.all(taken[:, :, 2:] == 0)


def test_first_success_latches():
    s = _state(0.7, 0.0, gx=0.8, gy=0.0)
    a = np.array([[[1, 0], [1, 0], [1, 0], [-1, 0]]], F32)                          # 0.78 (inside TOL), 0.86, 0.94 (outside), 0.86
    O.step(s, 4, actions=a)
    assert s[0, O.FIRST] == 1 and s[0, O.T] == 4
    far = _state(-0.8, 0.0)
    O.step(far, 3, actions=np.zeros((1, 3, 2), F32))
    assert far[0, O.FIRST] == 0


def test_the_tolerance_includes_its_boundary():
    s = _state(0.5, 0.0, gx=0.5, gy=0.0)
    s[0, O.PY] = O.TOL                                                              # d = (0, TOL): dy^2 = rn(TOL * TOL) = TOL^2
    O.step(s, 1, actions=np.zeros((1, 1, 2), F32))
    assert s[0, O.FIRST] == 1


def test_expert_heads_for_its_side_then_for_the_goal():
    s = _state(-0.8, 0.0, gx=0.8, gy=0.25, side=-1.0)
    a = O.scripted_action(s, O.EXPERT, 0.0, 0)
    d = ((np.array([0, -0.65], F32) - np.array([-0.8, 0], F32)).astype(F32) * F32(12.5)).astype(F32)
    assert np.array_equal(a[0], (d / np.abs(d).max()).astype(F32)) and a[0, 0] == 1
    assert np.array_equal(O.scripted_action(s, O.STRAIGHT, 0.0, 0)[0], np.array([1, F32(0.25 * 12.5) / F32(1.6 * 12.5)], F32))
    s[0, O.PX] = F32(0.1)
    g = O.scripted_action(s, O.EXPERT, 0.0, 0)
    assert np.array_equal(g, O.scripted_action(s, O.STRAIGHT, 0.0, 0))


def test_policy_noise_is_keyed_by_episode_and_time():
    s = O.reset(6, 3, 40)
    a = O.scripted_action(s, O.EXPERT, 0.3, 3, 40)
    assert np.array_equal(O.scripted_action(s[2:], O.EXPERT, 0.3, 3, 42), a[2:])
    s[:, O.T] = 5
    assert not np.array_equal(O.scripted_action(s, O.EXPERT, 0.3, 3, 40), a)
    r = O.scripted_action(s, O.RANDOM, 0.0, 3, 40)
    assert np.all((r >= -1) & (r < 1))


# ---- the task's own conditions, under the Philox draws ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rollouts():
    return {(p, nz): O.rollout(N_TASK, O.POLICIES[p], nz, seed=11)[0] for p, nz in (("expert", 0.1), ("straight", 0.1), ("random", 0.0))}


def test_the_expert_solves_the_task(rollouts):
    s = rollouts["expert", 0.1]
    rate = float((s[:, O.FIRST] != 0).mean())
    print(f"expert: success {rate:.4f}, first success mean {s[s[:, O.FIRST] != 0, O.FIRST].mean():.2f} max {s[:, O.FIRST].max():.0f}")
    assert rate >= 0.99
    assert np.all(s[:, O.T] == O.H)


def test_a_straight_line_mostly_fails(rollouts):
    s = rollouts["straight", 0.1]
    rate, blocked = float((s[:, O.FIRST] != 0).mean()), float((s[:, O.BLOCKED] > 0).mean())
    print(f"straight: success {rate:.4f}, blocked at least once {blocked:.4f}")
    assert rate <= 0.30


def test_random_actions_never_succeed(rollouts):
    assert not np.any(rollouts["random", 0.0][:, O.FIRST] != 0)


def test_the_demonstrations_pass_on_both_sides():
    _, act, pos, goal, lat = O.rollout(512, O.EXPERT, 0.1, seed=11)
    s0 = O.reset(512, 11)
    y_mid = pos[np.arange(512), np.abs(pos[:, :, 0]).argmin(1), 1]               # the height at which each episode crosses x = 0
    up = y_mid > 0
    assert np.array_equal(up, s0[:, O.SIDE] > 0) and 0.35 < up.mean() < 0.65
    assert np.all(np.abs(y_mid) > O.R) and np.abs(lat).max() <= 1 and np.abs(act).max() <= 1


# ---- run_device_eval on the NumPy environment ------------------------------------------------------------------------------------------
class _FakePolicy:
    """The expert, computed from the observation batch alone, as a stand-in for an agent: records how it was called."""

    def __init__(self, ah, kind="expert"):
        self.ah, self.kind, self.calls, self.resets = ah, kind, [], 0

    def reset(self):
        self.resets += 1

    def act(self, batch, rng, cycle):
        self.calls.append((rng, cycle))
        pos, goal = batch["obs"]["pos"][:, 0], batch["obs"]["goal"][:, 0]
        assert batch["obs"]["latent_image"].shape == (pos.shape[0], 1, 16)
        if self.kind == "still":
            return np.zeros((pos.shape[0], self.ah, 2), F32), {}
        up = goal[:, 1] > 0                                                        # pass above when the goal is above
        tgt = np.where((pos[:, 0] < 0)[:, None], np.stack([np.zeros_like(up, F32), np.where(up, 0.65, -0.65)], -1), goal).astype(F32)
        d = (tgt - pos) * 12.5
        a = d / np.maximum(np.abs(d).max(-1, keepdims=True), 1)
        return np.repeat(a[:, None], self.ah, 1).astype(F32), {"plan": None}


def test_run_device_eval_counts_cycles_rngs_and_resets():
    env, pol = O.NumpyReach2DEnv(8), _FakePolicy(4)
    res = harness.run_device_eval(env, pol.act, 24, seed=5, eval_rng=7, on_reset=pol.reset, episode0=100)
    assert pol.resets == 3 and res["n_calls"] == 36 and res["cycles_per_episode"] == 12 and res["n_rollout"] == 24
    assert [c for _, c in pol.calls] == list(range(12)) * 3
    assert [r for r, _ in pol.calls] == [7 * 1000003 + n for n in range(1, 37)]
    assert env.episode0 == 116 and env.seed == 5 and np.all(env.state[:, O.T] == O.H)
    assert res["ms_per_call"] > 0


def test_run_device_eval_metric_arithmetic():
    N, ah = 16, 4
    env, pol = O.NumpyReach2DEnv(N), _FakePolicy(ah)
    res = harness.run_device_eval(env, pol.act, 2 * N, seed=9, eval_rng=1)
    # the same closed loop by hand
    first, blocked = [], []
    for r in range(2):
        s = O.reset(N, 9, r * N)
        ref = _FakePolicy(ah)
        for c in range(O.H // ah):
            pos, goal, lat = O.observe(s)
            a, _ = ref.act({"obs": {"pos": pos[:, None], "goal": goal[:, None], "latent_image": lat[:, None]}}, 0, c)
            O.step(s, ah, actions=a)
        first.append(s[:, O.FIRST]); blocked.append(s[:, O.BLOCKED])
    first, blocked = np.concatenate(first), np.concatenate(blocked)
    ok = first != 0
    assert 0 < ok.sum()
    assert res["success_rate"] == float(ok.mean()) and res["mean_first_success"] == float(first[ok].astype(np.int64).mean())
    assert res["blocked_share"] == float(blocked.sum() / (2 * N * O.H))


def test_run_device_eval_without_a_success_and_with_a_ragged_last_cycle():
    env, pol = O.NumpyReach2DEnv(4), _FakePolicy(5, "still")                       # 48 = 9 * 5 + 3: the tenth cycle executes three actions
    res = harness.run_device_eval(env, lambda b, rng, c: pol.act(b, rng, c)[0], 4, seed=1, eval_rng=0)
    assert res["cycles_per_episode"] == 10 and np.all(env.state[:, O.T] == O.H)
    assert res["success_rate"] == 0 and np.isnan(res["mean_first_success"]) and res["blocked_share"] == 0
    with pytest.raises(ValueError, match="multiple"):
        harness.run_device_eval(env, pol.act, 6, seed=1, eval_rng=0)
