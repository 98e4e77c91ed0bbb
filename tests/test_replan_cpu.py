"""Warm-started replanning without a GPU: the float64 restatement of tests/replan_oracle.py against oracle.np64, the host
logic of Replanner / LDPAgent.sample_warm on a recording stub engine (in the style of tests/train_stub.py), and the harness option."""
import numpy as np
import pytest
import torch

from latent_diffusion_planning_amd import weights as W
from latent_diffusion_planning_amd.agent import LDPAgent, ParamState
from latent_diffusion_planning_amd._lib import LDPHipFault
from latent_diffusion_planning_amd.harness import run_aloha_eval, run_eval
from latent_diffusion_planning_amd.replan import Replanner, check_warm_steps, group_rows
from oracle import np64
from tests import cfgs, replan_oracle as RO
from tests.fake_env import make_aloha_env, make_env
from tests.train_stub import TrainStub
from tests.util import planner_params, rng

DATA = cfgs.RM_LIFT
D, A, T, AH = 25, 7, 8, 4


# ---- 1. the oracle restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler,n_train,n,m", [("ddim", 100, 4, 2), ("ddpm", 6, 6, 4)])
def test_ranges_compose_to_the_whole_loop_exactly(sampler, n_train, n, m):
    """planner_range(0, m) then planner_range(m, n) is np64.planner_sample, bit for bit.  DDPM visits every training timestep, so its
    case runs on a 6-step schedule (np64's own n_train argument): the whole loop stays affordable for the float64 U-Net, and the noise
    rows, the timesteps and the noise-free last step are np64.planner_sample's own."""
    pp = np64.to64(planner_params(D=D))
    g = rng(900 + n)
    cond, x0 = g.uniform(-1, 1, (1, D)), g.standard_normal((1, T, D))
    nz = g.standard_normal((n, 1, T, D)) if sampler == "ddpm" else None
    kw = dict(step_noise=nz, n_train=n_train, n_steps=n, sampler=sampler)
    whole = np64.planner_sample(pp, cond, x0, **kw)
    mid = RO.planner_range(pp, cond, x0, 0, m, **kw)
    assert not np.array_equal(mid, x0) and not np.array_equal(mid, whole)
    assert np.array_equal(RO.planner_range(pp, cond, mid, m, n, **kw), whole)
    assert np.array_equal(RO.planner_range(pp, cond, x0, 0, 0, **kw), x0)                    # an empty range is the identity
    stride = n_train // n
    assert [RO.step_timestep(i, n_train, n, sampler) for i in (0, n - 1)] == [(n - 1) * stride, 0]


@pytest.mark.parametrize("shift", [0, AH, T - 1, T + 3])
def test_shift_holds_the_edge(shift):
    x = rng(3).standard_normal((2, T, D))
    xs = RO.shift_hold(x, shift)
    for j in range(T):
        assert np.array_equal(xs[:, j], x[:, min(j + shift, T - 1)])
    # warm_init is FlaxDDPMScheduler.add_noise of the shifted plan at one timestep for every row
    eps = rng(4).standard_normal((2, T, D))
    a, s = RO.warm_coefs(40)
    got = RO.warm_init(x, shift, 40, eps)
    assert np.array_equal(got, np64.ddpm_add_noise(xs, eps, np.array([40, 40])))
    assert np.abs(got - (a * xs + s * eps)).max() <= 4 * np.finfo(np.float64).eps * np.abs(got).max()
    assert abs(a * a + s * s - 1.0) < 1e-15


# ---- 2. Replanner on a stub engine -----------------------------------------------------------------------------------------------------
class ReplanStub(TrainStub):
    """Records the two sampling calls.  Row b of a result carries the first embedding value of its observation (who), the global row it was
    drawn as (row_offset + b) and whether it was warm, so the test can see which call produced which returned row."""
    image_size = 64

    def _result(self, obs_emb, row_offset, warm):
        B = obs_emb.shape[0]
        who = obs_emb[:, 0, 0].reshape(B, 1, 1)
        row = (row_offset + torch.arange(B, dtype=torch.float32)).reshape(B, 1, 1)
        x = who + torch.zeros(B, T, D)
        x[:, :, 1], x[:, :, 2] = row[:, :, 0], float(warm)
        return x, x[:, :AH + 1].clone(), x[:, :AH, :A].clone()

    refuse_next_cold = False                                 # the next agent_sample raises LDP_EFAULT once (an earlier, unread fault)

    def agent_sample(self, obs_emb, obs_horizon, *, seed=0, row_offset=0, sampler="ddpm", planner_steps=None, idm_steps=None, **kw):
        self.calls.append(("agent_sample", obs_emb.shape[0], row_offset, seed, sampler, planner_steps, idm_steps))
        if self.refuse_next_cold:
            self.refuse_next_cold = False
            raise LDPHipFault(-6, "results since the last poll are invalid")
        self.call_seq += 1
        return self._result(obs_emb, row_offset, False)

    def agent_resample(self, obs_emb, obs_horizon, x_store, step_begin, *, slot=None, shift=None, seed=0, row_offset=0, sampler="ddim",
                       planner_steps=None, idm_steps=None, **kw):
        idx = torch.arange(obs_emb.shape[0]) if slot is None else torch.as_tensor(slot)
        prev = x_store[idx].clone()
        self.calls.append(("agent_resample", obs_emb.shape[0], row_offset, seed, sampler, planner_steps, idm_steps, step_begin,
                           None if slot is None else [int(v) for v in slot], shift, prev))
        self.call_seq += 1
        x, plan, act = self._result(obs_emb, row_offset, True)
        x_store[idx] = x
        return x, plan, act


@pytest.fixture
def agent(monkeypatch):
    monkeypatch.setattr(W, "check_params", lambda tree, shapes: None)          # the stub's trees hold one leaf
    cfg = dict(lowdim_obs=DATA["lowdim_obs"], rgb_obs=DATA["rgb_obs"], obs_horizon=1, pred_horizon=T, action_horizon=AH, obs_dim=D,
               action_dim=A, vae_feature_dim=16, planner_n_diffusion_steps=100, idm_n_diffusion_steps=100, name="ldp_agent")
    st = lambda: ParamState({"w": np.zeros(1, np.float32)})                    # noqa: E731
    return LDPAgent(st(), st(), None, DATA["obs_normalization"], True, True, 1, 1, cfg, ReplanStub(), W.PlannerSpec(D, D), W.IDMSpec(D, A),
                    W.VAESpec(), torch.device("cpu"))


def _who(ag, batch):
    return ag.get_obs_cond(ag._postprocess(batch)["obs"])[:, 0, 0].numpy()


def test_replanner_groups_warm_rows_first_and_restores_the_order(agent):
    eng = agent._engine
    rp = agent.replanner(6, warm_steps=2, sampler="ddim", n_steps=10)
    assert isinstance(rp, Replanner) and (rp.step_begin, rp.shift, rp.n_steps, rp.idm_steps) == (8, AH, 10, 10) and rp.valid == [False] * 6
    assert group_rows([True, False, True, False], [1, 2, 0, 3]) == ([1, 2, 0, 3], 2)
    assert group_rows([False, True, False, True], [1, 2, 0, 3]) == ([0, 3, 1, 2], 2)
    assert group_rows([False] * 4, [3, 1]) == ([0, 1], 0) and group_rows([True] * 4, [3, 1]) == ([0, 1], 2)

    # call 1: slots 4 and 2, both cold -> one agent_sample over both rows, row_offset 0
    b1 = cfgs.synth_latent_batch(DATA, 2, 1, 1)
    a1, m1 = rp.act(b1, 7, [4, 2])
    (c1,) = [c for c in eng.calls if c[0].startswith("agent_")]
    assert c1 == ("agent_sample", 2, 0, 7, "ddim", 10, 10)
    assert rp.valid == [False, False, True, False, True, False] and rp.calls == dict(warm=0, cold=1)
    x1 = np.array(m1["x"])
    assert np.array_equal(x1[:, 0, 0], _who(agent, b1)) and x1[:, 0, 1].tolist() == [0.0, 1.0] and x1[:, 0, 2].tolist() == [0.0, 0.0]
    assert np.array_equal(rp.table[4].numpy(), x1[0]) and np.array_equal(rp.table[2].numpy(), x1[1])      # cold rows store their x
    assert set(m1) == {"plan", "x", "plan_viz"} and a1.shape == (2, AH, A) and m1["plan"].shape == (2, AH + 1, D)

    # call 2: rows (slot 0: cold, slot 2: warm, slot 5: cold, slot 4: warm) -> warm rows [1, 3] first, then cold rows [0, 2]
    del eng.calls[:]
    b2 = cfgs.synth_latent_batch(DATA, 4, 1, 2)
    who = _who(agent, b2)
    a2, m2 = rp.act(b2, 9, [0, 2, 5, 4])
    warm, cold = [c for c in eng.calls if c[0].startswith("agent_")]
    assert warm[:9] == ("agent_resample", 2, 0, 9, "ddim", 10, 10, 8, [2, 4]) and warm[9] == AH
    assert np.array_equal(warm[10].numpy(), x1[[1, 0]])                      # each warm row read ITS slot's previous state
    assert cold == ("agent_sample", 2, 2, 9, "ddim", 10, 10)                 # row_offset = first position of the cold group
    x2 = np.array(m2["x"])
    assert np.array_equal(x2[:, 0, 0], who)                                  # results are back in the caller's row order
    assert x2[:, 0, 2].tolist() == [0.0, 1.0, 0.0, 1.0]                      # cold, warm, cold, warm
    assert x2[:, 0, 1].tolist() == [2.0, 0.0, 3.0, 1.0]                      # reordered positions: warm rows 0, 1; cold rows 2, 3
    assert np.array_equal(np.array(a2), x2[:, :AH, :A]) and np.array_equal(np.array(m2["plan"]), x2[:, :AH + 1])
    for row, slot in enumerate([0, 2, 5, 4]):
        assert np.array_equal(rp.table[slot].numpy(), x2[row])
    assert rp.valid == [True, False, True, False, True, True] and rp.calls == dict(warm=1, cold=2)

    # reset: slot 2 is cold again, slot 4 stays warm -> stable order [row of slot 4], then [row of slot 2]
    rp.reset([2])
    assert rp.valid[2] is False and rp.valid[4] is True
    del eng.calls[:]
    _, m3 = rp.act(cfgs.synth_latent_batch(DATA, 2, 1, 3), 1, [2, 4])
    kinds = [(c[0], c[1], c[2]) for c in eng.calls if c[0].startswith("agent_")]
    assert kinds == [("agent_resample", 1, 0), ("agent_sample", 1, 1)]
    assert np.array(m3["x"])[:, 0, 2].tolist() == [0.0, 1.0]
    rp.reset()
    assert rp.valid == [False] * 6


class _NoStream:
    def synchronize(self):
        pass


def test_replanner_retries_and_recomputes_cold(agent, monkeypatch):
    """What a fault does to a call whose warm rows have already overwritten their slots: the in-call retry and the deferred recompute both
    run every row cold, and a deferred recompute leaves alone the slots a later act() has written since."""
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: _NoStream())      # (the fault protocol waits for the stream)
    eng = agent._engine
    rp = agent.replanner(4, warm_steps=2, sampler="ddim", n_steps=10)
    rp.act(cfgs.synth_latent_batch(DATA, 2, 1, 1), 1, [0, 1])
    # slot 0 warm, slot 2 cold; the cold engine call is refused once -> the retry is ONE cold call over both rows, in the caller's order
    del eng.calls[:]
    eng.refuse_next_cold = True
    _, m = rp.act(cfgs.synth_latent_batch(DATA, 2, 1, 2), 2, [0, 2])
    kinds = [(c[0], c[1], c[2]) for c in eng.calls if c[0].startswith("agent_")]
    assert kinds == [("agent_resample", 1, 0), ("agent_sample", 1, 1), ("agent_sample", 2, 0)]
    x = np.array(m["x"])
    assert x[:, 0, 2].tolist() == [0.0, 0.0] and x[:, 0, 1].tolist() == [0.0, 1.0]
    assert np.array_equal(rp.table[0].numpy(), x[0]) and np.array_equal(rp.table[2].numpy(), x[1]) and rp.gen == [2, 1, 1, 0]
    # a fault found when call A's results are first read, after call B advanced slot 1: A recomputes cold and stores slot 3 only
    _, ma = rp.act(cfgs.synth_latent_batch(DATA, 2, 1, 3), 3, [1, 3])
    _, mb = rp.act(cfgs.synth_latent_batch(DATA, 1, 1, 4), 4, [1])
    slot1 = rp.table[1].clone()
    del eng.calls[:]
    eng.fault_upto, eng.last_fault_kinds = ma["x"]._record.seqs[0], 0
    xa = np.array(ma["x"])
    assert [(c[0], c[1], c[2]) for c in eng.calls if c[0].startswith("agent_")] == [("agent_sample", 2, 0)]
    assert xa[:, 0, 2].tolist() == [0.0, 0.0]                                  # both rows cold now (row 0 was warm in the faulted call)
    assert torch.equal(rp.table[1], slot1) and np.array_equal(rp.table[3].numpy(), xa[1])


def test_replanner_validates_slots_and_warm_steps(agent):
    rp = agent.replanner(3, warm_steps=10, n_steps=10)
    assert rp.step_begin == 0
    b = cfgs.synth_latent_batch(DATA, 2, 1, 1)
    with pytest.raises(ValueError, match="distinct"):
        rp.act(b, 0, [1, 1])
    with pytest.raises(ValueError, match="0..2"):
        rp.act(b, 0, [0, 3])
    with pytest.raises(ValueError, match="0..2"):
        rp.reset([-1])
    with pytest.raises(ValueError, match="2 rows but 1 slots"):
        rp.act(b, 0, [0])
    assert rp.valid == [False] * 3 and not [c for c in agent._engine.calls if c[0] == "agent_resample"]
    for k in (0, 11, -1):
        with pytest.raises(ValueError, match="warm_steps"):
            agent.replanner(3, warm_steps=k, n_steps=10)
        with pytest.raises(ValueError, match="warm_steps"):
            check_warm_steps(k, 10)
        with pytest.raises(ValueError, match="warm_steps"):
            agent.sample_warm(b, 0, torch.zeros(2, T, D), k, n_steps=10)
    assert check_warm_steps(1, 10) == 9 and check_warm_steps(10, 10) == 0
    with pytest.raises(ValueError, match="n_slots"):
        agent.replanner(0, warm_steps=1)
    with pytest.raises(ValueError, match="go together"):
        agent.sample_warm(b, 0, None, 3)


def test_sample_warm_passes_a_copy_of_prev_and_returns_x(agent):
    eng = agent._engine
    b = cfgs.synth_latent_batch(DATA, 2, 1, 5)
    prev = torch.full((2, T, D), 5.0)
    action, m = agent.sample_warm(b, 3, prev, 4, n_steps=10, row_offset=6)
    (c,) = [c for c in eng.calls if c[0].startswith("agent_")]
    assert c[:10] == ("agent_resample", 2, 6, 3, "ddim", 10, 10, 6, None, AH) and torch.equal(c[10], prev)
    assert torch.equal(prev, torch.full((2, T, D), 5.0))                      # the in-place write-back went to a copy
    assert set(m) == {"plan", "x", "plan_viz"} and np.array(m["x"]).shape == (2, T, D) and action.shape == (2, AH, A)
    # the cold call that also returns x: the existing path
    del eng.calls[:]
    _, m0 = agent.sample_warm(b, 3, None, None, n_steps=10)
    assert [c[0] for c in eng.calls if c[0].startswith("agent_")] == ["agent_sample"] and "x" in m0
    # a DeviceArray prev (the metrics['x'] of the previous call) is accepted as it is
    _, m1 = agent.sample_warm(b, 4, m0["x"], 2, n_steps=10)
    assert np.array(m1["x"])[:, 0, 2].tolist() == [1.0, 1.0]


def test_other_agents_name_ldp_agent():
    from latent_diffusion_planning_amd.dp_agent import DPAgent
    from latent_diffusion_planning_amd.dp_vae_agent import DPVAEAgent
    from latent_diffusion_planning_amd.hier_agent import LDPHierAgent
    for cls in (LDPHierAgent, DPVAEAgent, DPAgent):
        for name in ("sample_warm", "replanner"):
            with pytest.raises(NotImplementedError, match="LDPAgent"):
                getattr(cls, name)(object())
    with pytest.raises(NotImplementedError, match="LDPAgent"):
        LDPAgent.sample_best_of(type("P", (), dict(use_planner=True, use_idm=True))(), {}, 0, 4, prev=np.zeros(1), warm_steps=1)


# ---- 3. the harness option ---------------------------------------------------------------------------------------------------------------
def test_run_aloha_eval_resets_its_slot_once_per_episode():
    class Rp:
        def __init__(self):
            self.resets, self.acts, self.valid = [], [], False

        def reset(self, slots):
            self.resets.append(list(slots))
            self.valid = False

        def act(self, batch, rng, slots, decode=False):
            self.acts.append((list(slots), self.valid, decode))
            self.valid = True
            return np.full((1, 4, 14), 0.5, np.float32), {}

    class Pol:
        config = {"name": "dp_agent"}
        made = []

        def replanner(self, n_slots, **kw):
            self.made.append((n_slots, kw))
            self.rp = Rp()
            return self.rp

        def sample(self, batch, rng):
            raise AssertionError("with replan= every call goes through the replanner")
        sample_viz = sample

    env_params = dict(obs_horizon=1, lowdim_obs=["qpos"], rgb_obs=["latent_wrist64_image"], rgb_viz=None,
                      env_kwargs=dict(task_name="sim_transfer_cube", horizon=12))
    pol = Pol()
    logs, videos = run_aloha_eval(env_params, pol, n_rollout=3, seed=5, eval_rng=2, env_factory=make_aloha_env,
                                  replan=dict(warm_steps=2, sampler="ddim", n_steps=10))
    rp = pol.rp
    assert pol.made == [(1, dict(warm_steps=2, sampler="ddim", n_steps=10))]
    assert rp.resets == [[0]] * 3                                              # once per episode
    assert logs["policy_calls"] == len(rp.acts) and all(s == [0] and d is False for s, _, d in rp.acts)
    assert [v for _, v, _ in rp.acts].count(False) == 3                        # the first call of every episode is cold, the rest warm
    assert len(rp.acts) > 3 and rp.acts[0][1] is False and rp.acts[1][1] is True


class _EvalRp:
    def __init__(self, n_slots):
        self.resets, self.acts, self.valid = [], [], [False] * n_slots

    def reset(self, slots):
        self.resets.append(list(slots))
        for s in slots:
            self.valid[s] = False

    def act(self, batch, rng, slots, decode=False):
        x = next(iter(batch["obs"].values()))
        assert x.shape[0] == len(slots)
        self.acts.append((list(slots), [self.valid[s] for s in slots], decode))
        for s in slots:
            self.valid[s] = True
        return np.full((len(slots), 4, 7), 0.5, np.float32), {}


class _EvalPol:
    config = {"name": "dp_agent", "action_horizon": 4}

    def __init__(self):
        self.made = []

    def replanner(self, n_slots, **kw):
        self.made.append((n_slots, kw))
        self.rp = _EvalRp(n_slots)
        return self.rp

    def sample(self, batch, rng):
        raise AssertionError("with replan= every call goes through the replanner")
    sample_viz = sample


def test_run_eval_keeps_one_slot_per_worker_and_resets_it_on_the_sentinel():
    env = dict(obs_horizon=2, rgb_viz=None, env_kwargs=dict(lowdim_obs=["robot0_eef_pos"], rgb_obs=["latent_agentview_image"], horizon=24))
    pol = _EvalPol()
    logs, videos = run_eval(env, pol, n_rollout=6, n_proc=3, seed=10, eval_rng=1, env_factory=make_env, keep_latent_keys=True,
                            replan=dict(warm_steps=2, sampler="ddim", n_steps=10))
    rp = pol.rp
    assert pol.made == [(3, dict(warm_steps=2, sampler="ddim", n_steps=10))] and logs["success"] == 1.0 and len(videos) == 6
    assert logs["policy_calls"] == len(rp.acts) and all(d is False for _, _, d in rp.acts)
    assert all(set(s) <= {0, 1, 2} and len(set(s)) == len(s) for s, _, _ in rp.acts)      # the slot of a row is its worker's id
    # a worker ends each of its two episodes with the reset sentinel.  The one between its episodes sits in its queue in front of the next
    # episode's first observation, so it is always seen; the one behind its LAST episode may still be unread when the worker's results
    # arrive and its queues are dropped (nothing follows it): one or two resets per worker, one slot each
    per = [sum(r == [w] for r in rp.resets) for w in range(3)]
    assert all(len(r) == 1 for r in rp.resets) and sum(per) == len(rp.resets) and all(p in (1, 2) for p in per)
    cold = sum(v.count(False) for _, v, _ in rp.acts)
    assert cold == 6 and sum(len(v) for _, v, _ in rp.acts) > 6               # the first call of each of the 6 episodes is cold, the rest warm
