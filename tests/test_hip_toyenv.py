"""The device-resident reach task (csrc/env.hip, toyenv.py, harness.run_device_eval) on the GPU: the kernels against the NumPy restatement
of tests/toyenv_oracle.py bit for bit, whole expert rollouts and the demonstrations recorded from them, the closed loop with a
random-weight agent against a hand-written observe -> sample -> step loop, and a short training run on drawn demonstrations."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import toyenv_oracle as O
from tests.util import idm_params, planner_params, rng

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = 0x1234_5678_9ABC_DEF1
NS = (1, 3, 257)                                       # 257 crosses a work-group


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same(got, want, what=""):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.argwhere(g != w)
    assert not len(bad), f"{what}: {len(bad)} words differ, first at {bad[0].tolist()}"


def _env(N, A=2):
    from latent_diffusion_planning_amd.toyenv import Reach2DEnv
    return Reach2DEnv(N, action_dim=A)


def _hard_states(N, seed, episode0=0):
    """Reset states with every third environment moved next to the disc and every third one into a corner, so that given actions run
    into the disc and into the walls."""
    s = O.reset(N, seed, episode0)
    spots = np.array([[-0.33, 0.02], [0.96, -0.97], [0.02, 0.31], [-0.97, 0.96]], F32)
    for i in range(N):
        if i % 3:
            s[i, :2] = spots[(i + i // 3) % 4]
    return s


def _given(N, n_sub, A, seed):
    g = rng(seed)
    a = g.uniform(-1.5, 1.5, (N, n_sub, A)).astype(F32)
    pick = g.integers(0, 8, (N, n_sub, A))
    a[pick == 0], a[pick == 1], a[pick == 2] = 3.0, -3.0, np.nan
    a[0, 0, :2] = [np.nan, 3.0]
    return a


# ---- kernels against the restatement, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
def test_reset_and_observe(N):
    env = _env(N)
    env.reset(SEED, 5)
    ref = O.reset(N, SEED, 5)
    same(env.state, ref, "state")
    ob = env.observe()["obs"]
    pos, goal, lat = O.observe(ref)
    assert set(ob) == {"pos", "goal", "latent_image"} and ob["latent_image"].shape == (N, 1, 16)
    same(ob["pos"], pos[:, None], "pos"); same(ob["goal"], goal[:, None], "goal"); same(ob["latent_image"], lat[:, None], "latent")


@pytest.mark.parametrize("A", [2, 7])
@pytest.mark.parametrize("n_sub", [1, 4])
@pytest.mark.parametrize("N", NS)
def test_given_actions(N, n_sub, A):
    env = _env(N, A)
    ref = _hard_states(N, SEED)
    env.state.copy_(torch.from_numpy(ref))
    a = _given(N, n_sub, A, 10 * N + n_sub)
    rec = env.step(torch.from_numpy(a).cuda(), record=True)
    taken, pos, goal, lat = O.step(ref, n_sub, actions=a)
    same(env.state, ref, "state")
    same(rec["actions"], taken, "actions"); same(rec["pos"], pos, "pos"); same(rec["goal"], goal, "goal"); same(rec["latent_image"], lat, "latent")
    # the same step without the recording leaves the same state
    env2 = _env(N, A)
    env2.state.copy_(torch.from_numpy(_hard_states(N, SEED)))
    assert env2.step(torch.from_numpy(a).cuda()) is None
    same(env2.state, ref, "state (no record)")


def test_given_actions_hit_the_disc_and_the_walls():
    """What the hard states are for: at N = 257 the given actions are refused by the disc and clamped by the walls (checked on the
    restatement, which test_given_actions holds the kernel to)."""
    ref = _hard_states(257, SEED)
    O.step(ref, 4, actions=_given(257, 4, 2, 2574))
    assert (ref[:, O.BLOCKED] > 0).sum() > 10 and (np.abs(ref[:, :2]) == 1).any(axis=1).sum() > 10


@pytest.mark.parametrize("policy", ["expert", "straight", "random"])
@pytest.mark.parametrize("n_sub", [1, 4])
def test_scripted_policies(policy, n_sub):
    for N in NS:
        for A in (2, 7):
            env = _env(N, A)
            env.reset(SEED, 9)
            ref = O.reset(N, SEED, 9)
            for call in range(2):                                           # the second call starts at t = n_sub: its draws are those of step 1 + t
                rec = env.step_scripted(policy, 0.3, n_sub=n_sub, record=True)
                taken, pos, goal, lat = O.step(ref, n_sub, policy=O.POLICIES[policy], noise=0.3, seed=SEED, episode0=9, A=A)
                same(env.state, ref, f"state N={N} A={A} call={call}")
                same(rec["actions"], taken, "actions"); same(rec["pos"], pos, "pos"); same(rec["latent_image"], lat, "latent")
                same(rec["goal"], goal, "goal")


def test_policy_seed_is_its_own_argument():
    env, ref = _env(3), O.reset(3, 1, 0)
    env.reset(1, 0)
    env.step_scripted("expert", 0.3, seed=99, n_sub=4)
    O.step(ref, 4, policy=O.EXPERT, noise=0.3, seed=99, episode0=0)
    same(env.state, ref)


def test_an_episode_does_not_depend_on_the_split():
    whole, a, b = _env(257), _env(100), _env(157)
    a_np = _given(257, 4, 2, 77)
    dev = torch.from_numpy(a_np).cuda()
    outs = []
    for env, e0, sl in ((whole, 0, slice(0, 257)), (a, 0, slice(0, 100)), (b, 100, slice(100, 257))):
        env.reset(SEED, e0)
        r1 = env.step_scripted("expert", 0.3, n_sub=4, record=True)
        env.step(dev[sl].contiguous())
        r2 = env.step_scripted("random", n_sub=4, record=True)
        outs.append((env.state, r1["actions"], r1["latent_image"], r2["actions"], env.observe()["obs"]["latent_image"]))
    for k in range(5):
        same(torch.cat([outs[1][k], outs[2][k]]), outs[0][k], f"output {k}")


def test_refusals_name_the_argument():
    from latent_diffusion_planning_amd import _envlib as _lib
    from latent_diffusion_planning_amd.toyenv import Reach2DEnv
    lib = _lib.load()
    st = torch.zeros((4, 8), device="cuda")
    act = torch.zeros((4, 2, 2), device="cuda")
    p, a = st.data_ptr(), act.data_ptr()

    def step(N=4, n_sub=2, actions=a, A=2, policy=0, noise=0.0):
        return lib.ldp_env_step(p, N, n_sub, actions, A, policy, C.c_float(noise), 0, 0, None, None, None, None, None)
    for call, word in ((lambda: step(N=0), "N must be"), (lambda: step(n_sub=0), "n_sub"), (lambda: step(A=1), "A must be"),
                       (lambda: step(actions=None, policy=4), "policy"), (lambda: step(actions=None, policy=-1), "policy"),
                       (lambda: step(actions=None, policy=1, noise=float("nan")), "noise"),
                       (lambda: step(actions=None, policy=1, noise=float("inf")), "noise"),
                       (lambda: step(actions=None, policy=0), "actions"), (lambda: step(policy=1), "actions"),
                       (lambda: lib.ldp_env_reset(p, 0, 0, 0, None), "N must be"), (lambda: lib.ldp_env_reset(None, 4, 0, 0, None), "state"),
                       (lambda: lib.ldp_env_observe(p, 4, None, None, None, None), "output")):
        with pytest.raises(_lib.LDPHipError, match=word) as e:
            _lib.check(call())
        assert e.value.code == -1
    assert step() == 0
    with pytest.raises(ValueError, match="action_dim"):
        Reach2DEnv(4, action_dim=1)
    with pytest.raises(ValueError, match="shape"):
        Reach2DEnv(4).step(torch.zeros((3, 2, 2), device="cuda"))
    with pytest.raises(ValueError, match="policy"):
        Reach2DEnv(4).step_scripted("best")


# ---- whole expert rollouts and the demonstrations recorded from them -------------------------------------------------------------------
@pytest.fixture(scope="module")
def expert_ref():
    return O.rollout(257, O.EXPERT, 0.1, seed=SEED, episode0=2000)


def test_expert_rollout_first_success_equals_the_restatement(expert_ref):
    env = _env(257)
    env.reset(SEED, 2000)
    for _ in range(O.H // 4):
        env.step_scripted("expert", 0.1, n_sub=4)
    s = expert_ref[0]
    same(env.state, s, "state")
    assert np.array_equal(env.first_success().cpu().numpy(), s[:, O.FIRST].astype(np.int32)) and env.first_success().dtype == torch.int32
    assert np.array_equal(env.success().cpu().numpy(), s[:, O.FIRST] != 0) and bool(env.success().all())
    assert np.array_equal(env.blocked().cpu().numpy(), s[:, O.BLOCKED].astype(np.int32))


def test_recorded_demonstrations_equal_the_restatement(expert_ref):
    from latent_diffusion_planning_amd.toyenv import collect_demos
    _, act, pos, goal, lat = expert_ref
    ds = collect_demos(257, SEED, 0.1, episode0=2000)
    T = O.H
    assert ds.total_n_sequences == 257 * T and ds.n_demos == 257 and (ds.frame_stack, ds.seq_length) == (1, 9)
    for k, want in (("actions", act), ("pos", pos), ("goal", goal), ("latent_image", lat)):
        same(ds.tables[k], want.reshape(257 * T, -1), k)
    b = ds.bounds.cpu().numpy()
    assert np.array_equal(b[:, 0], np.repeat(np.arange(257) * T, T)) and np.array_equal(b[:, 1], b[:, 0] + T)


def test_drawn_batch_has_the_agents_shapes():
    from latent_diffusion_planning_amd.toyenv import collect_demos, reach2d_config
    cfg = reach2d_config(action_dim=7)
    ds = collect_demos(16, 3, 0.1, action_dim=7)
    batch = next(ds.batches(33, seed=1))
    kw = cfg["agent_kwargs"]
    W = kw["obs_horizon"] + kw["pred_horizon"]
    assert list(batch["obs"]) == ["pos", "goal", "latent_image"] == kw["lowdim_obs"] + kw["rgb_obs"]
    assert batch["actions"].shape == (33, kw["pred_horizon"] + 1, cfg["shape_meta"]["ac_dim"]) and bool((batch["actions"][..., 2:] == 0).all())
    for k in batch["obs"]:
        assert batch["obs"][k].shape == (33, W, cfg["shape_meta"]["all_shapes"][k][0]) and batch["obs"][k].is_cuda
        assert set(cfg["obs_normalization"]["obs"][k]) == {"min", "max"}
    # an episode's last windows repeat its last row (the weld clamps at the episode's end)
    last = ds.sample(1, 0, 0, indices=[O.H - 1])
    assert bool((last["obs"]["pos"][0] == last["obs"]["pos"][0, 0]).all())


# ---- the closed loop with a random-weight agent ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def agent():
    from latent_diffusion_planning_amd.agent import LDPAgent
    from latent_diffusion_planning_amd.toyenv import reach2d_config
    cfg = reach2d_config()
    ag = LDPAgent.create(0, None, cfg["shape_meta"], **cfg["agent_kwargs"])
    pp, ip = planner_params(D=20), idm_params(D=20, A=2)
    ag = ag.replace(planner_state=ag.planner_state.replace(params=pp, ema_params=pp), idm_state=ag.idm_state.replace(params=ip, ema_params=ip))
    yield ag
    ag._engine.close()


N_LOOP, RNG = 3, 21


def _hand_loop(env, call, episodes=(0,), on_reset=None):
    """observe -> call(batch, rng) -> step, written out: -> the states at the end of every round."""
    n, states = 0, []
    for e0 in episodes:
        env.reset(SEED, e0)
        if on_reset:
            on_reset()
        for c in range(O.H // 4):
            n += 1
            action = call(env.observe(), RNG * 1000003 + n)[0]
            assert action.shape == (N_LOOP, 4, 2)
            env.step(action.tensor)
        states.append(env.state.clone())
    return states


def _metrics(states):
    s = torch.cat(states).cpu().numpy()
    ok = s[:, O.FIRST] != 0
    return dict(success_rate=float(ok.mean()), mean_first_success=float(s[ok, O.FIRST].astype(np.int64).mean()) if ok.any() else float("nan"),
                blocked_share=float(s[:, O.BLOCKED].sum() / (len(s) * O.H)))


def _agree(res, want):
    for k, v in want.items():
        assert res[k] == v or (np.isnan(v) and np.isnan(res[k])), (k, res[k], v)


def test_run_device_eval_equals_the_hand_loop_and_repeats(agent):
    from latent_diffusion_planning_amd import harness
    sample = lambda batch, rng, cycle=None: agent.sample(batch, rng, sampler="ddim", n_steps=10)      # noqa: E731
    env = _env(N_LOOP)
    want = _hand_loop(env, sample, episodes=(0, N_LOOP))
    assert not np.array_equal(want[1][:, :2].cpu().numpy(), O.reset(N_LOOP, SEED, N_LOOP)[:, :2])                 # the policy moved the points
    runs = []
    for _ in range(2):
        res = harness.run_device_eval(env, sample, 2 * N_LOOP, SEED, RNG)
        runs.append((env.state.clone(), res))
    same(runs[0][0], want[1], "state after the last round")
    same(runs[1][0], want[1], "state after the last round, repeated")
    _agree(runs[0][1], _metrics(want)); _agree(runs[1][1], _metrics(want))
    assert runs[0][1]["n_calls"] == 24 and runs[0][1]["cycles_per_episode"] == 12 and runs[0][1]["ms_per_call"] > 0


def test_run_device_eval_with_a_replanner_equals_the_hand_loop(agent):
    from latent_diffusion_planning_amd import harness
    slots = list(range(N_LOOP))
    env = _env(N_LOOP)
    rp = agent.replanner(N_LOOP, warm_steps=2, sampler="ddim", n_steps=10)
    want = _hand_loop(env, lambda b, r: rp.act(b, r, slots), episodes=(0, N_LOOP), on_reset=rp.reset)
    assert rp.calls == dict(warm=22, cold=2)
    rp2 = agent.replanner(N_LOOP, warm_steps=2, sampler="ddim", n_steps=10)
    res = harness.run_device_eval(env, lambda b, r, c: rp2.act(b, r, slots), 2 * N_LOOP, SEED, RNG, on_reset=rp2.reset)
    assert rp2.calls == dict(warm=22, cold=2)
    same(env.state, want[1], "state after the last round")
    _agree(res, _metrics(want))
    # and a warm-started loop is not the cold one
    cold = _hand_loop(_env(N_LOOP), lambda b, r: agent.sample(b, r, sampler="ddim", n_steps=10), episodes=(0, N_LOOP))
    assert not np.array_equal(bits(cold[1]), bits(want[1]))


# ---- training on drawn demonstrations -------------------------------------------------------------------------------------------------
def test_fit_on_drawn_demonstrations(agent):
    from latent_diffusion_planning_amd import harness
    from latent_diffusion_planning_amd.toyenv import collect_demos
    ds = collect_demos(64, 5, 0.1)
    keys = ["planner/" + k for k in list(agent.planner_state.params)[:3]] + ["idm/" + k for k in list(agent.idm_state.params)[:3]]
    tree = lambda ag: {**{"planner/" + k: v for k, v in ag.planner_state.params.items()}, **{"idm/" + k: v for k, v in ag.idm_state.params.items()}}  # noqa: E731
    before = {k: np.array(tree(agent)[k]) for k in keys}
    logged = []
    fitted, m = harness.fit(agent, ds.batches(32, seed=2), 50, 4, log_every=10, on_log=lambda s, d: logged.append((s, d)))
    assert [s for s, _ in logged] == [10, 20, 30, 40, 50]
    for _, d in logged:
        assert np.isfinite(d["loss"]) and np.isfinite(d["plan_loss"]) and np.isfinite(d["idm_loss"]), d
    after = tree(fitted)
    for k in keys:
        a = np.array(after[k])
        assert np.isfinite(a).all() and not np.array_equal(a, before[k]), k
    # the trained agent still acts in the loop
    env = _env(N_LOOP)
    res = harness.run_device_eval(env, lambda b, r, c: fitted.sample(b, r, sampler="ddim", n_steps=10), N_LOOP, SEED, RNG)
    assert 0 <= res["success_rate"] <= 1 and bool(torch.isfinite(env.state).all())
