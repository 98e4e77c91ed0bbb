"""The device-resident pushing task (csrc/push.hip, pushenv.py, harness.run_device_eval) on the GPU: the kernels against the NumPy
restatement of tests/pushenv_oracle.py bit for bit -- reset, observation, given actions, every scripted policy, hand-built contact cases,
the strided loop at the first N at which a thread takes a second environment --, whole expert rollouts and the demonstrations recorded
from them, the closed loop with a random-weight agent against a hand-written observe -> sample -> step loop, a short training run, and the
action-free property of the planner's side of update_mixed."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import pushenv_oracle as O
from tests.util import idm_params, planner_params, rng

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = 0x1234_5678_9ABC_DEF1
NS = (1, 3, 257)                                       # a lone thread, a partial wave, one thread past a work-group
MARK = 12345.5


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same(got, want, what=""):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.argwhere(g != w)
    assert not len(bad), f"{what}: {len(bad)} words differ, first at {bad[0].tolist()}"


def _env(N, A=2):
    from latent_diffusion_planning_amd.pushenv import Push2DEnv
    return Push2DEnv(N, action_dim=A)


def _hard_states(N, seed, episode0=0):
    """Reset states with three in four environments moved: the point just short of contact with the disc, the disc next to its limit with
    the point behind it, the point in a corner -- so that given actions push, are refused and are clamped."""
    s = O.reset(N, seed, episode0)
    for i in range(N):
        k = i % 4
        if k == 1:
            s[i, O.PX], s[i, O.PY] = s[i, O.OX] - F32(0.21), s[i, O.OY] + F32(0.02)
        elif k == 2:
            s[i, O.OX], s[i, O.OY] = F32(0.82), F32(-0.3)
            s[i, O.PX], s[i, O.PY] = F32(0.60), F32(-0.28)
        elif k == 3:
            s[i, O.PX], s[i, O.PY] = F32(0.96), F32(-0.97)
    return s


def _given(N, n_sub, A, seed):
    g = rng(seed)
    a = g.uniform(-1.5, 1.5, (N, n_sub, A)).astype(F32)
    pick = g.integers(0, 8, (N, n_sub, A))
    a[pick == 0], a[pick == 1], a[pick == 2] = 3.0, -3.0, np.nan
    a[0, 0, :2] = [np.nan, 3.0]
    a[1::4, :, 0], a[2::4, :, 0] = 1.0, 1.0                                       # into the disc / into the limit
    return a


# ---- kernels against the restatement, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
def test_reset_and_observe(N):
    env = _env(N)
    env.reset(SEED, 5)
    ref = O.reset(N, SEED, 5)
    assert env.state.shape == (N, 12)
    same(env.state, ref, "state")
    ob = env.observe()["obs"]
    pos, goal, lat = O.observe(ref)
    assert set(ob) == {"pos", "goal", "latent_image"} and ob["latent_image"].shape == (N, 1, 16)
    same(ob["pos"], pos[:, None], "pos"); same(ob["goal"], goal[:, None], "goal"); same(ob["latent_image"], lat[:, None], "latent")


@pytest.mark.parametrize("A", [2, 7])
@pytest.mark.parametrize("n_sub", [1, 4, 48])
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
    assert A == 2 or bool((rec["actions"][..., 2:] == 0).all())
    # the same step without the recording leaves the same state
    env2 = _env(N, A)
    env2.state.copy_(torch.from_numpy(_hard_states(N, SEED)))
    assert env2.step(torch.from_numpy(a).cuda()) is None
    same(env2.state, ref, "state (no record)")


def test_given_actions_push_are_refused_and_are_clamped():
    """What the hard states are for: at N = 257 the given actions move the disc, are refused at its limit and are clamped by the walls
    (checked on the restatement, which test_given_actions holds the kernel to)."""
    ref = _hard_states(257, SEED)
    O.step(ref, 4, actions=_given(257, 4, 2, 2574))
    assert (ref[:, O.PUSHED] > 0).sum() > 30 and (ref[:, O.BLOCKED] > 0).sum() > 30 and (np.abs(ref[:, :2]) == 1).any(axis=1).sum() > 10


@pytest.mark.parametrize("policy", ["expert", "straight", "random"])
@pytest.mark.parametrize("n_sub", [1, 4, 48])
def test_scripted_policies(policy, n_sub):
    for N in NS:
        for A in (2, 7):
            env = _env(N, A)
            env.reset(SEED, 9)
            ref = O.reset(N, SEED, 9)
            for call in range(1 if n_sub == 48 else 2):                     # the second call starts at t = n_sub: its draws are those of step 1 + t
                rec = env.step_scripted(policy, 0.3, n_sub=n_sub, record=True)
                taken, pos, goal, lat = O.step(ref, n_sub, policy=O.POLICIES[policy], noise=0.3, seed=SEED, episode0=9, A=A)
                same(env.state, ref, f"state N={N} A={A} call={call}")
                same(rec["actions"], taken, "actions"); same(rec["pos"], pos, "pos"); same(rec["latent_image"], lat, "latent")
                same(rec["goal"], goal, "goal")
                assert A == 2 or bool((rec["actions"][..., 2:] == 0).all())


def test_hand_built_contact_cases():
    """The known answers of tests/test_pushenv_cpu.py through the kernel: head-on, oblique, coinciding centres, refused in x and in y, the
    contact boundary, the walls, NaN, the success latch."""
    q1 = O.fma32(F32(0.08), F32(1), F32(0))
    rows = [(0.0, 0.0, 0.25, 0.0), (0.0, 0.0, 0.2, 0.1), (0.0, 0.0, q1, 0.0), (0.6, 0.0, 0.84, 0.0), (0.0, 0.6, 0.0, 0.84), (-0.08, 0.0, 0.2, 0.0),
            (0.97, -0.97, 0.0, 0.0), (-0.8, 0.6, 0.0, 0.0), (0.1, 0.0, 0.35, 0.0)]
    s = np.zeros((len(rows), 12), F32)
    s[:, :4], s[:, O.GX], s[:, O.SIDE] = np.array(rows, F32), F32(0.6), 1
    a = np.zeros((len(rows), 6, 2), F32)
    a[:, :, 0] = 1
    a[4], a[6, :, 1], a[7, 0] = [0, 1], -1, [np.nan, np.nan]
    env = _env(len(rows))
    env.state.copy_(torch.from_numpy(s))
    one = s.copy()
    env.step(torch.from_numpy(a[:, :1].copy()).cuda())
    O.step(one, 1, actions=a[:, :1])
    same(env.state, one, "after one step")
    got = env.state.cpu().numpy()
    assert got[0, O.OX] == F32(q1 + O.C) and got[0, O.OY] == 0 and got[0, O.PUSHED] == 1                 # head-on: exactly q + (C, 0)
    assert got[1, O.OY] > F32(0.1) and got[1, O.PUSHED] == 1                                             # oblique: sideways too
    assert got[2, O.OX] == F32(q1 + O.C) and got[2, O.OY] == 0 and not np.isnan(got).any()               # dist == 0: the normal (1, 0)
    assert np.array_equal(got[3:5, :4], s[3:5, :4]) and np.all(got[3:5, O.BLOCKED] == 1) and np.all(got[3:5, O.PUSHED] == 0)
    assert got[6, O.PX] == 1 and got[6, O.PY] == -1 and np.array_equal(got[7, :2], s[7, :2])             # walls; NaN reads as 0
    env.step(torch.from_numpy(a[:, 1:].copy()).cuda())
    O.step(one, 5, actions=a[:, 1:])
    same(env.state, one, "after six steps")
    assert env.first_success().cpu().numpy()[8] == 3 and abs(float(env.state[8, O.OX]) - 0.6) > 0.1      # latched, and the disc has left
    assert env.pushed().dtype == torch.int32 and np.array_equal(env.pushed().cpu().numpy(), one[:, O.PUSHED].astype(np.int32))


def test_the_stride_loop():
    """N = 2048 * 256 + 3: the smallest N at which a thread takes a second environment (rows 524 288 .. 524 290 are the second ones of
    threads 0 .. 2).  One reset and one expert step of two sub-steps; the restatement computes the compared rows alone through episode0."""
    N, e0 = 2048 * 256 + 3, 7
    rows = np.unique(np.concatenate([[0, 255, 256, 524287, 524288, 524290], rng(5).integers(0, N, 64)]))
    env = _env(N)
    env.reset(SEED, e0)
    idx = torch.from_numpy(rows).cuda()
    ref = O.reset(len(rows), SEED, (rows + e0).astype(np.uint64))
    same(env.state[idx], ref, "reset")
    rec = env.step_scripted("expert", 0.3, n_sub=2, record=True)
    taken, pos, goal, lat = O.step(ref, 2, policy=O.EXPERT, noise=0.3, seed=SEED, episode0=(rows + e0).astype(np.uint64))
    same(env.state[idx], ref, "state")
    same(rec["actions"][idx], taken, "actions"); same(rec["pos"][idx], pos, "pos"); same(rec["goal"][idx], goal, "goal")
    same(rec["latent_image"][idx], lat, "latent")
    assert bool((env.state[:, O.T] == 2).all())                                        # every environment was stepped, once


def test_policy_seed_is_its_own_argument():
    env, ref = _env(3), O.reset(3, 1, 0)
    env.reset(1, 0)
    env.step_scripted("expert", 0.3, seed=99, n_sub=4)
    O.step(ref, 4, policy=O.EXPERT, noise=0.3, seed=99, episode0=0)
    same(env.state, ref)


def test_an_episode_does_not_depend_on_the_split():
    """Neither on how N is split over calls (episode0), nor on how the sub-steps are split over launches."""
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
    one, many = _env(257), _env(257)
    one.reset(SEED, 3); many.reset(SEED, 3)
    r = one.step_scripted("expert", 0.1, n_sub=48, record=True)
    parts = [many.step_scripted("expert", 0.1, n_sub=n, record=True) for n in (1, 4, 7, 36)]
    same(many.state, one.state, "state")
    for k in r:
        same(torch.cat([p[k] for p in parts], dim=1), r[k], k)


def test_outputs_stay_inside_their_buffers():
    """Every output of a recording step and of observe, pre-filled with a marker, with a guard region behind it: every word inside is
    written, no word of the guard is."""
    from latent_diffusion_planning_amd import _pushlib as _lib
    N, n_sub, A, G = 259, 3, 7, 64
    lib = _lib.load()
    env = _env(N, A)
    env.reset(SEED, 0)
    st = torch.full((N * 12 + G,), MARK, device="cuda")
    _lib.check(lib.ldp_push_reset(st.data_ptr(), N, C.c_uint64(SEED), 0, None))
    same(st[:N * 12].reshape(N, 12), env.state, "state"); assert bool((st[N * 12:] == MARK).all())
    widths = dict(actions=A, pos=2, goal=2, latent=16)
    for frames, call in ((1, "observe"), (n_sub, "step")):
        buf = {k: torch.full((N * frames * w + G,), MARK, device="cuda") for k, w in widths.items()}
        if call == "observe":
            _lib.check(lib.ldp_push_observe(st.data_ptr(), N, buf["pos"].data_ptr(), buf["goal"].data_ptr(), buf["latent"].data_ptr(), None))
        else:
            _lib.check(lib.ldp_push_step(st.data_ptr(), N, n_sub, None, A, 1, C.c_float(0.1), C.c_uint64(SEED), 0, buf["actions"].data_ptr(),
                                         buf["pos"].data_ptr(), buf["goal"].data_ptr(), buf["latent"].data_ptr(), None))
        for k, w in widths.items():
            body, guard = buf[k][:N * frames * w], buf[k][N * frames * w:]
            assert bool((guard == MARK).all()), (call, k)
            assert (call == "observe" and k == "actions") or bool((body != MARK).all()), (call, k)
    assert bool((st[N * 12:] == MARK).all())
    ref = O.reset(N, SEED, 0)
    taken, pos, goal, lat = O.step(ref, n_sub, policy=O.EXPERT, noise=0.1, seed=SEED, A=A)
    same(st[:N * 12].reshape(N, 12), ref, "state after the step")
    same(buf["actions"][:N * n_sub * A].reshape(N, n_sub, A), taken, "actions"); same(buf["latent"][:N * n_sub * 16].reshape(N, n_sub, 16), lat, "latent")


def test_refusals_name_the_argument():
    from latent_diffusion_planning_amd import _pushlib as _lib
    from latent_diffusion_planning_amd.pushenv import Push2DEnv
    lib = _lib.load()
    st = torch.zeros((4, 12), device="cuda")
    act = torch.zeros((4, 2, 2), device="cuda")
    p, a = st.data_ptr(), act.data_ptr()

    def step(N=4, n_sub=2, actions=a, A=2, policy=0, noise=0.0):
        return lib.ldp_push_step(p, N, n_sub, actions, A, policy, C.c_float(noise), 0, 0, None, None, None, None, None)
    for call, word in ((lambda: step(N=0), "N must be"), (lambda: step(n_sub=0), "n_sub"), (lambda: step(A=1), "A must be"),
                       (lambda: step(actions=None, policy=4), "policy"), (lambda: step(actions=None, policy=1, noise=float("nan")), "noise"),
                       (lambda: step(actions=None, policy=0), "actions"), (lambda: step(policy=1), "actions"),
                       (lambda: lib.ldp_push_reset(p + 4, 4, 0, 0, None), "aligned"),
                       (lambda: lib.ldp_push_observe(p, 4, None, None, None, None), "output")):
        with pytest.raises(_lib.LDPHipError, match=word) as e:
            _lib.check(call())
        assert e.value.code == -1
    assert step() == 0
    with pytest.raises(ValueError, match="action_dim"):
        Push2DEnv(4, action_dim=1)
    with pytest.raises(ValueError, match="shape"):
        Push2DEnv(4).step(torch.zeros((3, 2, 2), device="cuda"))
    with pytest.raises(ValueError, match="policy"):
        Push2DEnv(4).step_scripted("best")


# ---- whole expert rollouts and the demonstrations recorded from them -------------------------------------------------------------------
@pytest.fixture(scope="module")
def expert_ref():
    return O.rollout(64, O.EXPERT, 0.1, seed=SEED, episode0=2000)


def test_expert_rollout_equals_the_restatement(expert_ref):
    env = _env(64)
    env.reset(SEED, 2000)
    for _ in range(O.H // 4):
        env.step_scripted("expert", 0.1, n_sub=4)
    s = expert_ref[0]
    same(env.state, s, "state")
    assert np.array_equal(env.first_success().cpu().numpy(), s[:, O.FIRST].astype(np.int32)) and env.first_success().dtype == torch.int32
    assert np.array_equal(env.success().cpu().numpy(), s[:, O.FIRST] != 0) and bool(env.success().all())
    assert np.array_equal(env.blocked().cpu().numpy(), s[:, O.BLOCKED].astype(np.int32))
    assert np.array_equal(env.pushed().cpu().numpy(), s[:, O.PUSHED].astype(np.int32)) and int(env.pushed().min()) > 0
    assert np.array_equal(env.goal_side().cpu().numpy(), s[:, O.GX] < 0)


@pytest.mark.parametrize("policy", ["expert", "random"])
def test_recorded_demonstrations_equal_the_restatement(expert_ref, policy):
    from latent_diffusion_planning_amd.pushenv import collect_push_demos, without_actions
    _, act, pos, goal, lat = expert_ref if policy == "expert" else O.rollout(64, O.RANDOM, 0.1, seed=SEED, episode0=2000)
    ds = collect_push_demos(64, SEED, 0.1, episode0=2000, policy=policy)
    T = O.H
    assert ds.total_n_sequences == 64 * T and ds.n_demos == 64 and (ds.frame_stack, ds.seq_length) == (1, 9)
    assert ds.env_meta["env_name"] == "push2d" and ds.env_meta["policy"] == policy
    for k, want in (("actions", act), ("pos", pos), ("goal", goal), ("latent_image", lat)):
        same(ds.tables[k], want.reshape(64 * T, -1), k)
    b = ds.bounds.cpu().numpy()
    assert np.array_equal(b[:, 0], np.repeat(np.arange(64) * T, T)) and np.array_equal(b[:, 1], b[:, 0] + T)
    free = without_actions(ds)
    assert bool((free.tables["actions"] == 0).all()) and free.tables["pos"] is ds.tables["pos"] and bool((ds.tables["actions"] != 0).any())


def test_drawn_batch_has_the_agents_shapes():
    from latent_diffusion_planning_amd.pushenv import collect_push_demos, push2d_config
    from latent_diffusion_planning_amd.toyenv import reach2d_config
    cfg = push2d_config(action_dim=7)
    ref = reach2d_config(action_dim=7)
    assert cfg["agent_kwargs"]["data_name"] == "push2d" and cfg["shape_meta"] == ref["shape_meta"]
    assert {k: v for k, v in cfg["agent_kwargs"].items() if k != "data_name"} == {k: v for k, v in ref["agent_kwargs"].items() if k != "data_name"}
    ds = collect_push_demos(16, 3, 0.1, action_dim=7)
    batch = next(ds.batches(33, seed=1))
    kw = cfg["agent_kwargs"]
    W = kw["obs_horizon"] + kw["pred_horizon"]
    assert list(batch["obs"]) == ["pos", "goal", "latent_image"] == kw["lowdim_obs"] + kw["rgb_obs"]
    assert batch["actions"].shape == (33, kw["pred_horizon"] + 1, cfg["shape_meta"]["ac_dim"]) and bool((batch["actions"][..., 2:] == 0).all())
    for k in batch["obs"]:
        assert batch["obs"][k].shape == (33, W, cfg["shape_meta"]["all_shapes"][k][0]) and batch["obs"][k].is_cuda
    assert sum(cfg["shape_meta"]["all_shapes"][k][0] for k in batch["obs"]) == 20                     # obs_dim stays 20


# ---- the closed loop with a random-weight agent ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def agent():
    from latent_diffusion_planning_amd.agent import LDPAgent
    from latent_diffusion_planning_amd.pushenv import push2d_config
    cfg = push2d_config()
    ag = LDPAgent.create(0, None, cfg["shape_meta"], **cfg["agent_kwargs"])
    pp, ip = planner_params(D=20), idm_params(D=20, A=2)
    ag = ag.replace(planner_state=ag.planner_state.replace(params=pp, ema_params=pp), idm_state=ag.idm_state.replace(params=ip, ema_params=ip))
    yield ag
    ag._engine.close()


N_LOOP, RNG = 3, 21


def _hand_loop(env, call, episodes=(0,)):
    """observe -> call(batch, rng) -> step, written out: -> the states at the end of every round."""
    n, states = 0, []
    for e0 in episodes:
        env.reset(SEED, e0)
        for c in range(O.H // 4):
            n += 1
            action = call(env.observe(), RNG * 1000003 + n)[0]
            assert action.shape == (N_LOOP, 4, 2)
            env.step(action.tensor)
        states.append(env.state.clone())
    return states


def test_run_device_eval_equals_the_hand_loop_and_repeats(agent):
    from latent_diffusion_planning_amd import harness
    sample = lambda batch, rng, cycle=None: agent.sample(batch, rng, sampler="ddim", n_steps=10)      # noqa: E731
    env = _env(N_LOOP)
    want = _hand_loop(env, sample, episodes=(0, N_LOOP))
    assert not np.array_equal(want[1][:, :2].cpu().numpy(), O.reset(N_LOOP, SEED, N_LOOP)[:, :2])                 # the policy moved the points
    s = torch.cat(want).cpu().numpy()
    ok = s[:, O.FIRST] != 0
    metrics = dict(success_rate=float(ok.mean()), mean_first_success=float(s[ok, O.FIRST].astype(np.int64).mean()) if ok.any() else float("nan"),
                   blocked_share=float(s[:, O.BLOCKED].sum() / (len(s) * O.H)))
    for _ in range(2):
        res = harness.run_device_eval(env, sample, 2 * N_LOOP, SEED, RNG)
        same(env.state, want[1], "state after the last round")
        for k, v in metrics.items():
            assert res[k] == v or (np.isnan(v) and np.isnan(res[k])), (k, res[k], v)
        assert res["n_calls"] == 24 and res["cycles_per_episode"] == 12 and res["ms_per_call"] > 0


# ---- training on drawn demonstrations -------------------------------------------------------------------------------------------------
def test_ten_fit_steps_give_finite_losses(agent):
    from latent_diffusion_planning_amd import harness
    from latent_diffusion_planning_amd.pushenv import collect_push_demos
    ds = collect_push_demos(64, 5, 0.1)
    logged = []
    fitted, m = harness.fit(agent, ds.batches(32, seed=2), 10, 4, log_every=5, on_log=lambda s, d: logged.append((s, d)))
    assert [s for s, _ in logged] == [5, 10] and fitted.planner_state.step == 10
    for _, d in logged:
        assert np.isfinite(d["loss"]) and np.isfinite(d["plan_loss"]) and np.isfinite(d["idm_loss"]), d
    k = next(iter(agent.planner_state.params))
    assert not np.array_equal(np.array(fitted.planner_state.params[k]), np.array(agent.planner_state.params[k]))


def test_the_planners_side_of_update_mixed_reads_no_actions(agent):
    """Two update_mixed steps, twice: the planner's batch is drawn from the expert's demonstrations with their real `actions` table, then
    from the same demonstrations with an all-zero one (pushenv.without_actions).  Same IDM batch, same seeds, explicit noise: the planner's
    and the IDM's parameters must come out bit-equal, i.e. the planner learns from action-free data."""
    from latent_diffusion_planning_amd.pushenv import collect_push_demos, without_actions
    B, T, D, A, n_idm = 16, 8, 20, 2, 100
    real = collect_push_demos(32, 5, 0.1)
    free = without_actions(real)
    labelled = collect_push_demos(4, 6, 0.1, episode0=5000)
    out = []
    for ds in (real, free):
        ag = agent
        for step in range(2):
            batch, mb = ds.sample(B, 11, step), labelled.sample(B, 12, step)
            assert bool((batch["actions"] == 0).all()) == (ds is free)
            nz = np.random.Generator(np.random.PCG64(100 + step))
            noise = dict(t_plan=nz.integers(0, 100, B), noise_plan=nz.standard_normal((B, T, D)).astype(F32),
                         t_idm=nz.integers(0, n_idm, B * T), noise_idm=nz.standard_normal((B * T, A)).astype(F32))
            ag, m = ag.update_mixed(batch, mb, 40 + step, step, noise=noise)
        assert np.isfinite(float(m["plan_loss"])) and np.isfinite(float(m["idm_loss"]))
        out.append((dict(ag.planner_state.params), dict(ag.idm_state.params)))
    for which in (0, 1):
        assert list(out[0][which]) == list(out[1][which])
        for k in out[0][which]:
            same(np.array(out[0][which][k]), np.array(out[1][which][k]), f"{('planner', 'idm')[which]}/{k}")
    k = next(iter(out[0][0]))
    assert not np.array_equal(np.array(out[0][0][k]), np.array(agent.planner_state.params[k]))           # and the steps did train
