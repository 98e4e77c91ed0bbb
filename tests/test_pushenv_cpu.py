"""The push2d task on the host: the library's C ABI, known answers of the NumPy restatement (tests/pushenv_oracle.py) the kernels are held
to, the task's own conditions under the Philox draws (the expert solves it on both goal sides, a straight run at the disc mostly does not,
random actions do not) and harness.run_device_eval on the NumPy environment with a scripted stand-in for the policy.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from latent_diffusion_planning_amd import harness
from tests import pushenv_oracle as O

F32 = np.float32
N_TASK = 4096


def _state(px, py, ox, oy, gx=0.6, gy=0.0, side=1.0):
    return np.array([[px, py, ox, oy, gx, gy, side, 0, 0, 0, 0, 0]], F32)


def _act(*rows):
    return np.array([list(rows)], F32)


# ---- the library's C ABI ---------------------------------------------------------------------------------------------------------------
SYMS = ["ldp_push_last_error", "ldp_push_observe", "ldp_push_reset", "ldp_push_step"]


def test_push_header_binding_and_library_list_the_same_symbols():
    """libldp_push.so is a library of its own: include/ldp_push.h, _pushlib.SIGNATURES and its dynamic symbol table agree."""
    from latent_diffusion_planning_amd import _pushlib
    assert _pushlib.header_symbols() == sorted(_pushlib.SIGNATURES) == SYMS
    with open(os.path.join(os.path.dirname(_pushlib.LIB_PATH), "csrc", "Makefile")) as f:
        assert "libldp_push.so" in f.read()
    assert os.path.exists(_pushlib.LIB_PATH), "build() makes libldp_push.so"
    out = subprocess.run(["nm", "-D", "--defined-only", _pushlib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(line.split()[-1] for line in out.splitlines() if line.strip()) == SYMS
    _pushlib.load()


def test_the_other_libraries_export_no_push_symbol():
    from latent_diffusion_planning_amd import _envlib, _lib, _pixlib
    for mod in (_lib, _envlib, _pixlib):
        assert not [s for s in mod.SIGNATURES if s.startswith("ldp_push")]
        assert not [s for s in mod.header_symbols() if s.startswith("ldp_push")]
        if os.path.exists(mod.LIB_PATH):
            out = subprocess.run(["nm", "-D", "--defined-only", mod.LIB_PATH], capture_output=True, text=True, check=True).stdout
            assert "ldp_push" not in out, mod.LIB_PATH


def test_the_constants_of_header_binding_and_restatement_agree():
    import re
    from latent_diffusion_planning_amd import _pushlib
    with open(_pushlib.HEADER_PATH) as f:
        defs = dict(re.findall(r"#define (LDP_P\w+) (\d+)u?\b", f.read()))
    assert int(defs["LDP_PUSH_STATE"]) == _pushlib.PUSH_STATE == O.STATE == 12
    assert int(defs["LDP_PUSH_LATENT"]) == _pushlib.PUSH_LATENT == O.LATENT == 16
    assert int(defs["LDP_PUSH_EPISODE_LEN"]) == _pushlib.PUSH_EPISODE_LEN == O.H == 48
    assert int(defs["LDP_PHILOX_STREAM_PUSH"]) == _pushlib.PHILOX_STREAM_PUSH == O.STREAM_PUSH == 14
    assert {k: int(defs["LDP_PUSH_POLICY_" + k.upper()]) for k in O.POLICIES} == O.POLICIES == _pushlib.PUSH_POLICIES
    assert int(defs["LDP_PUSH_POLICY_GIVEN"]) == O.GIVEN == 0


def test_a_missing_push_library_fails_loudly(monkeypatch, tmp_path):
    from latent_diffusion_planning_amd import _lib, _pushlib
    monkeypatch.setattr(_pushlib, "_lib", None)
    monkeypatch.setattr(_pushlib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.LDPHipUnavailable, match="no other implementation"):
        _pushlib.load()


def test_bad_arguments_are_refused_by_name_before_any_hip_call():
    """Every refusal below is decided on the host from the arguments alone: the pointers are never dereferenced and no device is needed."""
    import ctypes as C
    from latent_diffusion_planning_amd import _lib, _pushlib
    lib = _pushlib.load()
    p, a = 1 << 20, 1 << 21                                                        # aligned, never touched

    def step(state=p, N=4, n_sub=2, actions=a, A=2, policy=0, noise=0.0, episode0=0):
        return lib.ldp_push_step(state, N, n_sub, actions, A, policy, C.c_float(noise), 0, episode0, None, None, None, None, None)
    for call, word in ((lambda: step(state=None), "null state"), (lambda: step(state=p + 4), "16-byte aligned"), (lambda: step(N=0), "N must be"),
                       (lambda: step(N=-3), "N must be"), (lambda: step(n_sub=0), "n_sub"), (lambda: step(A=1), "A must be"),
                       (lambda: step(actions=None, policy=4), "policy"), (lambda: step(actions=None, policy=-1), "policy"),
                       (lambda: step(actions=None, policy=1, noise=float("nan")), "noise"),
                       (lambda: step(actions=None, policy=1, noise=float("inf")), "noise"), (lambda: step(episode0=-1), "episode0"),
                       (lambda: step(actions=None, policy=0), "actions"), (lambda: step(policy=1), "actions"),
                       (lambda: lib.ldp_push_reset(None, 4, 0, 0, None), "null state"), (lambda: lib.ldp_push_reset(p + 8, 4, 0, 0, None), "aligned"),
                       (lambda: lib.ldp_push_reset(p, 0, 0, 0, None), "N must be"), (lambda: lib.ldp_push_reset(p, 4, 0, -1, None), "episode0"),
                       (lambda: lib.ldp_push_observe(None, 4, a, None, None, None), "null state"),
                       (lambda: lib.ldp_push_observe(p, 0, a, None, None, None), "N must be"),
                       (lambda: lib.ldp_push_observe(p, 4, None, None, None, None), "output")):
        with pytest.raises(_lib.LDPHipError, match=word) as e:
            _pushlib.check(call())
        assert e.value.code == -1


# ---- known answers ---------------------------------------------------------------------------------------------------------------------
def test_a_head_on_push_puts_the_disc_at_contact_distance():
    s = _state(0.0, 0.0, 0.25, 0.0)
    O.step(s, 1, actions=_act([1.0, 0.0]))
    q = O.fma32(O.DT, F32(1), F32(0))
    assert s[0, O.PX] == q and s[0, O.PY] == 0 and s[0, O.OX] == F32(q + O.C) and s[0, O.OY] == 0
    assert s[0, O.PUSHED] == 1 and s[0, O.BLOCKED] == 0 and s[0, O.T] == 1


def test_an_oblique_push_moves_the_disc_along_the_contact_normal():
    s = _state(0.0, 0.0, 0.2, 0.1)
    O.step(s, 1, actions=_act([1.0, 0.0]))
    q = np.array([0.08, 0.0])
    d = np.array([F32(0.2), F32(0.1)], np.float64) - np.array([F32(0.08), 0.0])
    want = np.array([F32(0.08), 0.0], np.float64) + 0.2 * d / np.linalg.norm(d)
    got = s[0, [O.OX, O.OY]].astype(np.float64)
    assert np.abs(got - want).max() < 1e-6 and got[1] > 0.1 and s[0, O.PUSHED] == 1          # sideways as well as forward
    assert abs(np.linalg.norm(got - q) - 0.2) < 1e-6


def test_coinciding_centres_take_the_normal_1_0():
    s = _state(0.0, 0.0, O.fma32(F32(0.08), F32(1), F32(0)), 0.0)
    O.step(s, 1, actions=_act([1.0, 0.0]))
    assert s[0, O.OX] == F32(s[0, O.PX] + O.C) and s[0, O.OY] == 0 and s[0, O.PUSHED] == 1 and not np.isnan(s).any()


def test_a_push_past_the_limit_is_refused_and_counted():
    s = _state(0.6, 0.0, 0.84, 0.0)
    before = s.copy()
    O.step(s, 1, actions=_act([1.0, 0.0]))                                           # q = 0.68, the disc would go to 0.88 > LIM
    assert np.array_equal(s[0, :4], before[0, :4]) and s[0, O.BLOCKED] == 1 and s[0, O.PUSHED] == 0 and s[0, O.T] == 1
    s = _state(0.0, 0.6, 0.0, 0.84)
    O.step(s, 1, actions=_act([0.0, 1.0]))                                           # and in y
    assert s[0, O.PY] == F32(0.6) and s[0, O.OY] == F32(0.84) and s[0, O.BLOCKED] == 1
    s = _state(0.4, 0.0, 0.62, 0.0)
    O.step(s, 1, actions=_act([1.0, 0.0]))                                           # q = 0.48, the disc goes to 0.68 < LIM: taken
    assert s[0, O.BLOCKED] == 0 and s[0, O.PUSHED] == 1


def test_the_contact_boundary_is_not_contact():
    """d2 >= C2 = rn(C * C) by definition is free: the disc at exactly C from q does not move."""
    s = _state(0.0, 0.0, 0.2, 0.0)
    O.step(s, 1, actions=np.zeros((1, 1, 2), F32))
    assert s[0, O.PUSHED] == (1 if O.fma32(F32(0.2), F32(0.2), F32(0)) < O.C2 else 0) == 0 and s[0, O.OX] == F32(0.2)


def test_walls_clamp_the_point():
    s = _state(0.97, -0.97, 0.0, 0.0)
    O.step(s, 1, actions=_act([1.0, -1.0]))
    assert s[0, O.PX] == 1 and s[0, O.PY] == -1 and s[0, O.BLOCKED] == 0 and s[0, O.PUSHED] == 0


def test_nan_and_out_of_range_actions():
    a = np.array([[[np.nan, 3.0], [-3.0, np.nan], [np.inf, -np.inf]]], F32)
    s, ref = _state(-0.8, 0.6, 0.0, 0.0), _state(-0.8, 0.6, 0.0, 0.0)
    taken = O.step(s, 3, actions=a)[0]
    assert taken[0].tolist() == [[0, 1], [-1, 0], [1, -1]]
    O.step(ref, 3, actions=np.array([[[0, 1], [-1, 0], [1, -1]]], F32))
    assert np.array_equal(s, ref)


def test_only_two_components_are_read():
    a = np.zeros((1, 2, 7), F32)
    a[0, :, :2], a[0, :, 2:] = [[0.5, -0.25], [1, 1]], np.nan
    s, ref = _state(-0.8, 0.0, 0.0, 0.0), _state(-0.8, 0.0, 0.0, 0.0)
    taken = O.step(s, 2, actions=a)[0]
    O.step(ref, 2, actions=a[:, :, :2].copy())
    assert np.array_equal(s, ref) and taken.shape == (1, 2, 7) and np.all(taken[:, :, 2:] == 0)


def test_success_latches_and_says_where_the_disc_is():
    s = _state(0.1, 0.0, 0.35, 0.0, gx=0.6, gy=0.0)
    firsts = []
    for _ in range(6):                                                              # the disc goes 0.38, 0.46, 0.54 (inside TOL), ... 0.78 (outside)
        O.step(s, 1, actions=_act([1.0, 0.0]))
        firsts.append(int(s[0, O.FIRST]))
    assert firsts == [0, 0, 3, 3, 3, 3] and s[0, O.T] == 6
    assert abs(float(s[0, O.OX]) - 0.6) > 0.1                                       # it has left, the latch stays
    # the point at the goal is no success
    s = _state(0.6, 0.0, 0.0, 0.5, gx=0.6, gy=0.0)
    O.step(s, 3, actions=np.zeros((1, 3, 2), F32))
    assert s[0, O.FIRST] == 0


def test_the_tolerance_includes_its_boundary():
    s = _state(-0.8, 0.0, 0.5, O.TOL, gx=0.5, gy=0.0)                               # e = (0, TOL): ey^2 = rn(TOL * TOL) = TOL2
    O.step(s, 1, actions=np.zeros((1, 1, 2), F32))
    assert s[0, O.FIRST] == 1


def test_reset_follows_the_philox_words():
    from oracle import philox
    s = O.reset(64, seed=77, episode0=1000)
    w = philox.words(77, 1000, 0, O.STREAM_PUSH, 64)
    u = lambda k: (w[:, k] >> 8).astype(F32) * F32(2.0 ** -24)                       # noqa: E731
    assert np.array_equal(s[:, O.PY], F32(-0.5) + u(0)) and np.all(s[:, O.PX] == F32(-0.8))
    assert np.array_equal(s[:, O.OX], O.fma32(F32(0.6), u(1), F32(-0.3))) and np.array_equal(s[:, O.OY], O.fma32(F32(0.8), u(2), F32(-0.4)))
    assert np.array_equal(s[:, O.GX], np.where(w[:, 0] & 1, F32(-0.6), F32(0.6))) and np.array_equal(s[:, O.GY], F32(-0.5) + u(3))
    assert np.array_equal(s[:, O.SIDE], np.where(w[:, 1] & 1, 1, -1).astype(F32))
    assert np.all(s[:, O.T:] == 0)
    assert 0.2 < (s[:, O.GX] < 0).mean() < 0.8 and 0.2 < (s[:, O.SIDE] > 0).mean() < 0.8
    assert np.all(np.abs(s[:, O.OX]) <= 0.3) and np.all(np.abs(s[:, O.OY]) <= 0.4)
    assert np.array_equal(O.reset(67, 77, 997)[3:], s)                              # episode0 keys the episode, not the batch
    assert np.array_equal(O.reset(3, 77, np.array([1000, 1063, 1005], np.uint64)), s[[0, 63, 5]])


def test_observation_layout_and_range():
    s = _state(-0.5, 0.5, 0.25, -0.25, gx=-0.6, gy=0.125)
    pos, goal, lat = O.observe(s)
    assert pos.tolist() == [[-0.5, 0.5]] and goal.tolist() == [[F32(-0.6), 0.125]]
    x = np.array([-0.5, 0.5, 0.25, -0.25, F32(F32(F32(-0.6) - F32(0.25)) * F32(0.5)), F32(0.375 * 0.5), 0.375, -0.375], F32)
    assert lat.shape == (1, 16) and np.array_equal(lat[0, 0::2], x) and np.array_equal(lat[0, 1::2], O.fma32(x + x, x, F32(-1)))
    assert O.cheb2(F32(0.5)).tolist() == [0.5, -0.5] and O.cheb2(F32(1)).tolist() == [1, 1] and O.cheb2(F32(0)).tolist() == [0, -1]
    # the extremes the dynamics allow: the point in a corner, the disc at its limit
    s = _state(1.0, -1.0, -0.85, 0.85, gx=0.6, gy=-0.5)
    assert np.abs(O.observe(s)[2]).max() <= 1


def test_policy_noise_is_keyed_by_episode_and_time():
    s = O.reset(6, 3, 40)
    a = O.scripted_action(s, O.EXPERT, 0.3, 3, 40)
    assert np.array_equal(O.scripted_action(s[2:], O.EXPERT, 0.3, 3, 42), a[2:])
    s[:, O.T] = 5
    assert not np.array_equal(O.scripted_action(s, O.EXPERT, 0.3, 3, 40), a)
    r = O.scripted_action(s, O.RANDOM, 0.0, 3, 40)
    assert np.all((r >= -1) & (r < 1))


def test_the_expert_pushes_from_behind_and_goes_round_from_the_front():
    behind = _state(-0.3, 0.0, 0.0, 0.0, gx=0.6, gy=0.0)                             # on the far side of the disc from the goal: push
    assert np.array_equal(O.expert_target(behind)[0], np.array([F32(-0.1), 0], F32))
    front = _state(0.3, 0.0, 0.0, 0.0, gx=0.6, gy=0.0, side=-1.0)                    # between disc and goal, |lat| <= 0.05: `side` decides
    t = O.expert_target(front)[0]
    assert t[1] == O.fma32(F32(-0.39), F32(1), F32(0)) and t[0] == F32(0.3)          # nh = (0, 1), s = -1
    front[0, O.SIDE] = 1
    assert O.expert_target(front)[0, 1] == F32(0.39)
    assert np.array_equal(O.scripted_action(front, O.STRAIGHT, 0.0, 0)[0], np.array([-1, 0], F32))


# ---- the task's own conditions, under the Philox draws ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rollouts():
    return {p: O.rollout(N_TASK, O.POLICIES[p], 0.1, seed=11)[0] for p in ("expert", "straight", "random")}


def test_the_expert_solves_the_task_on_both_goal_sides(rollouts):
    s = rollouts["expert"]
    ok, left = s[:, O.FIRST] != 0, s[:, O.GX] < 0
    print(f"expert: success {ok.mean():.4f} (left {ok[left].mean():.4f} of {left.sum()}, right {ok[~left].mean():.4f}), first success mean "
          f"{s[ok, O.FIRST].mean():.2f} max {s[:, O.FIRST].max():.0f}, contact moves {s[:, O.PUSHED].mean():.2f}, refused {s[:, O.BLOCKED].sum():.0f}")
    assert ok.mean() >= 0.99 and ok[left].mean() >= 0.98 and ok[~left].mean() >= 0.98
    assert 0.4 < left.mean() < 0.6
    assert s[:, O.FIRST].max() <= 46
    assert np.all(s[:, O.T] == O.H)


def test_a_straight_run_at_the_disc_mostly_fails(rollouts):
    s = rollouts["straight"]
    rate = float((s[:, O.FIRST] != 0).mean())
    print(f"straight: success {rate:.4f}")
    assert rate <= 0.15


def test_random_actions_do_not_succeed(rollouts):
    rate = float((rollouts["random"][:, O.FIRST] != 0).mean())
    print(f"random: success {rate:.4f}")
    assert rate <= 0.01


def test_the_demonstrations_stay_in_range(rollouts):
    _, act, pos, goal, lat = O.rollout(256, O.EXPERT, 0.1, seed=11)
    assert np.abs(lat).max() <= 1 and np.abs(act).max() <= 1 and np.abs(pos).max() <= 1
    assert np.all(np.abs(rollouts["expert"][:, [O.OX, O.OY]]) <= O.LIM)


# ---- run_device_eval on the NumPy environment ------------------------------------------------------------------------------------------
class _FakePolicy:
    """The noiseless expert, computed from the observation batch alone (the disc is read out of the latent), as a stand-in for an agent."""

    def __init__(self, ah, kind="expert"):
        self.ah, self.kind, self.calls, self.resets = ah, kind, [], 0

    def reset(self):
        self.resets += 1

    def act(self, batch, rng, cycle):
        self.calls.append((rng, cycle))
        pos, goal, lat = batch["obs"]["pos"][:, 0], batch["obs"]["goal"][:, 0], batch["obs"]["latent_image"][:, 0]
        assert lat.shape == (pos.shape[0], 16)
        if self.kind == "still":
            return np.zeros((pos.shape[0], self.ah, 2), F32), {}
        s = np.zeros((pos.shape[0], O.STATE), F32)
        s[:, [O.PX, O.PY]], s[:, [O.OX, O.OY]], s[:, [O.GX, O.GY]], s[:, O.SIDE] = pos, lat[:, [4, 6]], goal, 1
        a = O.scripted_action(s, O.EXPERT, 0.0, 0)
        return np.repeat(a[:, None], self.ah, 1).astype(F32), {"plan": None}


def test_run_device_eval_counts_cycles_rngs_and_resets():
    env, pol = O.NumpyPush2DEnv(8), _FakePolicy(4)
    res = harness.run_device_eval(env, pol.act, 24, seed=5, eval_rng=7, on_reset=pol.reset, episode0=100)
    assert pol.resets == 3 and res["n_calls"] == 36 and res["cycles_per_episode"] == 12 and res["n_rollout"] == 24
    assert [c for _, c in pol.calls] == list(range(12)) * 3
    assert [r for r, _ in pol.calls] == [7 * 1000003 + n for n in range(1, 37)]
    assert env.episode0 == 116 and env.seed == 5 and np.all(env.state[:, O.T] == O.H)


def test_run_device_eval_metric_arithmetic():
    N, ah = 16, 2
    env, pol = O.NumpyPush2DEnv(N), _FakePolicy(ah)
    res = harness.run_device_eval(env, pol.act, 2 * N, seed=9, eval_rng=1)
    first, blocked = [], []
    for r in range(2):                                                              # the same closed loop by hand
        s = O.reset(N, 9, r * N)
        ref = _FakePolicy(ah)
        for c in range(O.H // ah):
            pos, goal, lat = O.observe(s)
            a, _ = ref.act({"obs": {"pos": pos[:, None], "goal": goal[:, None], "latent_image": lat[:, None]}}, 0, c)
            O.step(s, ah, actions=a)
        first.append(s[:, O.FIRST]); blocked.append(s[:, O.BLOCKED])
    first, blocked = np.concatenate(first), np.concatenate(blocked)
    ok = first != 0
    assert ok.sum() > N                                                             # a closed-loop expert holding each action for two steps still pushes
    assert res["success_rate"] == float(ok.mean()) and res["mean_first_success"] == float(first[ok].astype(np.int64).mean())
    assert res["blocked_share"] == float(blocked.sum() / (2 * N * O.H))
    assert np.array_equal(env.pushed(), env.state[:, O.PUSHED].astype(np.int32)) and env.pushed().sum() > 0


def test_run_device_eval_without_a_success_and_with_a_ragged_last_cycle():
    env, pol = O.NumpyPush2DEnv(4), _FakePolicy(5, "still")                        # 48 = 9 * 5 + 3: the tenth cycle executes three actions
    res = harness.run_device_eval(env, lambda b, rng, c: pol.act(b, rng, c)[0], 4, seed=1, eval_rng=0)
    assert res["cycles_per_episode"] == 10 and np.all(env.state[:, O.T] == O.H)
    assert res["success_rate"] == 0 and np.isnan(res["mean_first_success"]) and res["blocked_share"] == 0
