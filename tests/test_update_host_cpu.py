"""The host side of the training steps without a GPU: `update` / `update_mixed` / `_update_step` of LDPAgent, LDPHierAgent and DPVAEAgent
and the weight hand-off between a state and an engine slot, on the recording stub engine (tests/train_stub.py).  What is pinned here is the
call sequence, the host draws, the shard arithmetic and the metric assembly; the numbers of a step are pinned by the GPU goldens."""
import numpy as np
import pytest
import torch

from latent_diffusion_planning_amd import agent as agent_mod, dp_vae_agent as dp_mod, weights as W
from latent_diffusion_planning_amd.agent import LDPAgent, ParamState
from latent_diffusion_planning_amd.dp_vae_agent import DPState, DPVAEAgent
from latent_diffusion_planning_amd.hier_agent import LDPHierAgent
from latent_diffusion_planning_amd.vae_model import StableVAEModel
from tests import cfgs
from tests.train_stub import TrainStub

DATA = cfgs.RM_LIFT
B, OH, FUTURE, D, A = 3, 1, 4, 25, 7          # three samples, one observed frame, four future frames
H = OH + FUTURE
N_PLAN, N_IDM = 100, 50                        # diffusion steps of the two networks
SEED = 11
OBS_KEYS = DATA["lowdim_obs"] + DATA["rgb_obs"]


def sched_p(count):
    return 1e-4 + 1e-6 * count


def sched_i(count):
    return 3e-4 + 1e-6 * count


@pytest.fixture(autouse=True)
def tiny_trees(monkeypatch):
    monkeypatch.setattr(W, "check_params", lambda tree, shapes: None)          # the stub's trees hold one leaf


@pytest.fixture
def philox(monkeypatch):
    """agent._philox_normal, recorded: (seed, elem0, step, stream, n) per call."""
    seen = []

    def fake(seed, elem0, step, stream_id, n, device):
        seen.append((seed, elem0, step, stream_id, n))
        return torch.full((n,), float(stream_id))
    monkeypatch.setattr(agent_mod, "_philox_normal", fake)
    monkeypatch.setattr(dp_mod, "_philox_normal", fake)                       # (imported there by name)
    return seen


def _config(**kw):
    cfg = dict(lowdim_obs=DATA["lowdim_obs"], rgb_obs=DATA["rgb_obs"], obs_horizon=OH, pred_horizon=8, action_horizon=4, obs_dim=D,
               action_dim=A, vae_feature_dim=16, planner_n_diffusion_steps=N_PLAN, idm_n_diffusion_steps=N_IDM, update_planner_every=1,
               update_idm_every=1, update_idm_after=-1, update_planner_until=-1, update_planner_after=-1)
    cfg.update(kw)
    return cfg


def _state():
    return ParamState({"w": np.zeros(1, np.float32)})


def _ldp(alpha_planner=1, alpha_idm=1, **cfg):
    return LDPAgent(_state(), _state(), None, DATA["obs_normalization"], True, True, alpha_planner, alpha_idm, _config(**cfg), TrainStub(),
                    W.PlannerSpec(D, D * OH), W.IDMSpec(D, A), W.VAESpec(), torch.device("cpu"), lr_schedules={"planner": sched_p, "idm": sched_i})


def _hier():
    ag = LDPHierAgent(_state(), _state(), None, DATA["obs_normalization"], True, True, 1, 1, _config(idm_horizon=2), TrainStub(grad_norm=3.0),
                      W.PlannerSpec(D, D * OH), None, W.VAESpec(), torch.device("cpu"), lr_schedules={"planner": sched_p, "idm": sched_i})
    ag._idm_engine, ag._idm_unet_spec = TrainStub(grad_norm=4.0), W.PlannerSpec(A, 2 * D, down_dims=(256, 512))
    return ag


def _batch(seed, n=B):
    return cfgs.synth_latent_batch(DATA, n, H, seed, with_actions=True)


def _emb(ag, batch):
    """(observation embedding, normalised actions) as the step sees them."""
    nb = ag._postprocess(batch)
    return LDPAgent.get_obs_cond(ag, nb["obs"]).contiguous(), nb["actions"]


def _draws(seed, *sizes_and_highs):
    g = np.random.Generator(np.random.PCG64(seed & (2**63 - 1)))
    return [g.integers(0, high, size=size) for size, high in sizes_and_highs]


LDP_KEYS = (["planner_lr", "planner_step", "idm_lr", "idm_step", "plan_loss", "idm_loss", "loss", "g_norm", "emb_min", "emb_max", "emb_mean",
             "emb_std", "action_min", "action_max"] + [f"{k}_{s}" for k in OBS_KEYS for s in ("min", "max")])


# ---- 1. LDPAgent.update: two steps ---------------------------------------------------------------------------------------------------------
def test_ldp_update_call_sequence_draws_and_metrics(philox):
    ag0 = _ldp(alpha_planner=2, alpha_idm=0.5)
    eng = ag0._engine
    batch = _batch(1)
    ag1, m = ag0.update(batch, SEED, 0)
    stats = ["stats"] * (2 + len(OBS_KEYS))
    assert eng.kinds() == ["load", "load"] + stats + ["idm_grad", "planner_grad", "apply", "apply", "grad_norm"]
    assert [c[1] for c in eng.of("load")] == ["planner", "idm"] and [c[1] for c in eng.of("apply")] == ["planner", "idm"]
    assert eng.of("grad_norm") == [("grad_norm", ["planner", "idm"])]
    # host draws: one PCG64(seed) generator, the planner's B timesteps first, then the IDM's B x transitions
    t_plan, t_idm = _draws(SEED, (B, N_PLAN), (B * FUTURE, N_IDM))
    (_, x0, eps_p, tp, cond, w_p), = eng.of("planner_grad")
    (_, s, a, eps_i, ti, w_i), = eng.of("idm_grad")
    np.testing.assert_array_equal(tp, t_plan)
    np.testing.assert_array_equal(ti, t_idm)
    emb, act = _emb(ag0, batch)
    assert torch.equal(x0, emb[:, OH:]) and torch.equal(cond, emb[:, :OH].reshape(B, -1))
    assert torch.equal(s, torch.cat([emb[:, OH - 1:-1], emb[:, OH:]], dim=-1).reshape(-1, 2 * D)) and torch.equal(a, act[:, :-1].reshape(-1, A))
    assert [torch.equal(c[1], want) for c, want in zip(eng.of("stats"), [emb, act])] == [True, True]
    assert (w_p, w_i) == (2.0, 0.5)                                            # alpha * B / n, n = B
    # the noise: Philox stream 7 for the planner and 8 for the IDM, from element 0, enqueued IDM first
    assert philox == [(SEED, 0, 0, 8, a.numel()), (SEED, 0, 0, 7, x0.numel())]
    assert tuple(eps_p.shape) == tuple(x0.shape) and tuple(eps_i.shape) == tuple(a.shape)
    # Adam takes each network's own schedule; both reported rates come from the last-built one (the IDM's), at the old step
    assert [c[2] for c in eng.of("apply")] == [float(np.float32(sched_p(0))), float(np.float32(sched_i(0)))]
    assert m["planner_lr"] == np.float32(sched_i(0)) and m["idm_lr"] == np.float32(sched_i(0)) and isinstance(m["planner_lr"], np.float32)
    assert list(m) == LDP_KEYS and (m["planner_step"], m["idm_step"]) == (0, 0)
    assert float(m["plan_loss"]) == 0.25 and float(m["idm_loss"]) == 0.5 and float(m["loss"]) == 0.75 and float(m["g_norm"]) == 3.0
    assert float(m["emb_min"]) == float(emb.min()) and float(m["action_max"]) == float(act.max())
    assert (ag1.planner_state.step, ag1.idm_state.step) == (1, 1) and (ag0.planner_state.step, ag0.idm_state.step) == (0, 0)

    # the second step trains on what the first left in the arenas
    del eng.calls[:]
    ag2, m2 = ag1.update(_batch(2), SEED + 1, 1)
    assert eng.kinds() == stats + ["idm_grad", "planner_grad", "apply", "apply", "grad_norm"]
    assert [c[2] for c in eng.of("apply")] == [float(np.float32(sched_p(1))), float(np.float32(sched_i(1)))]
    assert m2["planner_lr"] == np.float32(sched_i(1)) and (m2["planner_step"], m2["idm_step"]) == (1, 1)
    np.testing.assert_array_equal(eng.of("planner_grad")[0][3], _draws(SEED + 1, (B, N_PLAN))[0])
    for st in (ag1.planner_state, ag1.idm_state):
        with pytest.raises(RuntimeError, match="superseded"):
            st.params
        with pytest.raises(RuntimeError, match="superseded"):
            st.opt_state
    assert float(ag2.planner_state.params["Dense_0/bias"][0]) == eng.TRAIN_PARAMS
    assert float(ag2.idm_state.opt_state["nu"]["MLPResNet_0/Dense_1/bias"][0]) == eng.TRAIN_NU and ag2.idm_state.opt_state["count"] == 2


def test_ldp_update_slices_explicit_noise_only_when_it_is_global(philox):
    ag = _ldp()
    emb, act = _emb(ag, _batch(1))
    noise = dict(t_plan=np.arange(B), noise_plan=np.ones((B, FUTURE, D), np.float32), t_idm=np.arange(B * FUTURE) % N_IDM,
                 noise_idm=np.full((B * FUTURE, A), 2.0, np.float32))
    ag.update(_batch(1), SEED, 0, noise=noise)
    (_, _, eps_p, tp, _, _), = ag._engine.of("planner_grad")
    (_, _, _, eps_i, ti, _), = ag._engine.of("idm_grad")
    np.testing.assert_array_equal(tp, noise["t_plan"])
    np.testing.assert_array_equal(ti, noise["t_idm"])
    assert torch.equal(eps_p, torch.ones(B, FUTURE, D)) and torch.equal(eps_i, torch.full((B * FUTURE, A), 2.0))


# ---- 2. update_mixed and the gates ------------------------------------------------------------------------------------------------------------
def test_update_mixed_feeds_the_idm_from_the_mixed_batch(philox):
    ag = _ldp()
    eng = ag._engine
    batch, mixed = _batch(1), _batch(2, n=B + 1)
    ag.update_mixed(batch, mixed, SEED, 0)
    emb, act = _emb(ag, batch)
    emb_m, act_m = _emb(ag, mixed)
    (_, x0, _, tp, cond, _), = eng.of("planner_grad")
    (_, s, a, _, ti, _), = eng.of("idm_grad")
    assert torch.equal(x0, emb[:, OH:]) and torch.equal(cond, emb[:, :OH].reshape(B, -1))
    assert torch.equal(s, torch.cat([emb_m[:, OH - 1:-1], emb_m[:, OH:]], dim=-1).reshape(-1, 2 * D))
    assert torch.equal(a, act_m[:, :-1].reshape(-1, A))
    t_plan, t_idm = _draws(SEED, (B, N_PLAN), ((B + 1) * FUTURE, N_IDM))
    np.testing.assert_array_equal(tp, t_plan)
    np.testing.assert_array_equal(ti, t_idm)
    st = eng.of("stats")
    assert torch.equal(st[0][1], emb) and torch.equal(st[1][1], act) and len(st) == 2 + len(OBS_KEYS)


def test_a_gated_off_planner_reports_zeros_and_keeps_its_state(philox):
    ag = _ldp(update_planner_every=2)
    eng = ag._engine
    before = ag.planner_state
    ag2, m = ag.update(_batch(1), SEED, 1)
    assert ag2.planner_state is before and ag2.idm_state is not ag.idm_state and ag2.idm_state.step == 1
    assert "planner_grad" not in eng.kinds() and [c[1] for c in eng.of("load") + eng.of("apply")] == ["idm", "idm"]
    assert eng.of("grad_norm") == [("grad_norm", ["idm"])]
    assert list(m)[:5] == ["planner_lr", "planner_step", "noise_diff", "idm_lr", "idm_step"]
    assert (m["planner_lr"], m["planner_step"], m["noise_diff"]) == (0, 0, 0) and float(m["plan_loss"]) == 0.0
    # a gated-off network draws nothing: the IDM's timesteps are the generator's FIRST draw
    np.testing.assert_array_equal(eng.of("idm_grad")[0][4], _draws(SEED, (B * FUTURE, N_IDM))[0])
    assert philox == [(SEED, 0, 0, 8, B * FUTURE * A)]
    # ... and the IDM gated off (update_idm_after), the planner trained
    ag3 = _ldp(update_idm_after=5)
    before = ag3.idm_state
    ag4, m = ag3.update(_batch(1), SEED, 0)
    assert ag4.idm_state is before and (m["idm_lr"], m["idm_step"]) == (0, 0) and "noise_diff" not in m
    assert "idm_grad" not in ag3._engine.kinds() and ag3._engine.of("grad_norm") == [("grad_norm", ["planner"])]


def test_side_streams_wait_for_the_main_stream_and_the_main_stream_for_them(philox, monkeypatch):
    """The choreography with side streams, on named stand-ins: the statistics go to `stats` and the IDM's tape to `idm`, each behind what
    the main stream holds so far; the planner's tape stays on the main stream, which waits for both before the optimiser."""
    import contextlib
    ag = _ldp()
    eng = ag._engine

    class Stream:
        def __init__(self, name):
            self.name = name

        def wait_stream(self, other):
            eng.calls.append(("wait", self.name, other.name))
    main, side = Stream("main"), {"idm": Stream("idm"), "stats": Stream("stats")}

    @contextlib.contextmanager
    def on_stream(stream):
        eng.calls.append(("enter", stream.name))
        yield
        eng.calls.append(("exit", stream.name))
    eng.aux_streams = lambda: side
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: main)
    monkeypatch.setattr(torch.cuda, "stream", on_stream)
    ag.update(_batch(1), SEED, 0)
    flow = [c[:3] if c[0] == "wait" else c[:2] if c[0] in ("enter", "exit") else c[0] for c in eng.calls if c[0] != "stats"]
    assert flow == ["load", "load", ("wait", "stats", "main"), ("enter", "stats"), ("exit", "stats"), ("wait", "idm", "main"), ("enter", "idm"),
                    "idm_grad", ("exit", "idm"), "planner_grad", ("wait", "main", "idm"), ("wait", "main", "stats"), "apply", "apply", "grad_norm"]
    kinds = eng.kinds()
    assert kinds.index("enter") < kinds.index("stats") and len(kinds) - 1 - kinds[::-1].index("stats") < kinds.index("exit")
    # one network alone trains on the main stream; the statistics keep their stream
    del eng.calls[:]
    ag.replace(config=dict(ag.config, update_planner_every=2)).update(_batch(1), SEED, 1)
    assert ("enter", "idm") not in eng.calls and ("enter", "stats") in eng.calls and ("wait", "main", "stats") in eng.calls
    # train_streams off: no stream is touched
    del eng.calls[:]
    eng.get_option = lambda name: 0
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: pytest.fail("the step looked up a CUDA stream"))
    ag.update(_batch(1), SEED, 0)
    assert not [c for c in eng.calls if c[0] in ("wait", "enter", "exit")]


# ---- 3. a shard of a global batch -----------------------------------------------------------------------------------------------------------
@pytest.fixture
def one_rank_group(tmp_path, monkeypatch):
    """A one-process gloo group (its all-reduces are identities); every all-reduce is recorded."""
    import torch.distributed as dist
    dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    seen, real = [], dist.all_reduce

    def recorded(tensor, *a, **k):
        seen.append(tensor)
        return real(tensor, *a, **k)
    monkeypatch.setattr(dist, "all_reduce", recorded)
    yield seen
    dist.destroy_process_group()


def test_a_shard_takes_its_rows_of_the_global_draws_and_weights_by_its_share(philox, one_rank_group):
    lo, n = 2, 8
    ag = _ldp()
    eng = ag._engine
    g = np.random.Generator(np.random.PCG64(5))
    noise = dict(noise_plan=g.standard_normal((n, FUTURE, D)).astype(np.float32))       # explicit for the planner, Philox for the IDM
    ag.replace()._update_step(_batch(1), None, SEED, True, True, noise, shard={"rows": (lo, n), "mixed_rows": (0, n), "group": None})
    t_plan, t_idm = _draws(SEED, (n, N_PLAN), (n * FUTURE, N_IDM))
    (_, x0, eps_p, tp, _, w_p), = eng.of("planner_grad")
    (_, _, a, _, ti, w_i), = eng.of("idm_grad")
    np.testing.assert_array_equal(tp, t_plan[lo:lo + B])
    np.testing.assert_array_equal(ti, t_idm[lo * FUTURE:(lo + B) * FUTURE])
    assert torch.equal(eps_p, torch.as_tensor(noise["noise_plan"][lo:lo + B]))
    assert philox == [(SEED, lo * FUTURE * A, 0, 8, a.numel())]                          # elem0 = lo x elements per sample
    assert w_p == w_i == float(np.float32(B) / np.float32(n))
    # one all-reduce per trained gradient arena and one for the two loss scalars, all before the first apply
    kinds = eng.kinds()
    assert eng.of("arena") == [("arena", "planner", eng.TRAIN_GRADS), ("arena", "idm", eng.TRAIN_GRADS)]
    assert max(i for i, k in enumerate(kinds) if k == "arena") < kinds.index("apply") and kinds.index("planner_grad") < kinds.index("arena")
    assert len(one_rank_group) == 3 and one_rank_group[0] is eng.arenas[("planner", eng.TRAIN_GRADS)]
    assert one_rank_group[1] is eng.arenas[("idm", eng.TRAIN_GRADS)] and tuple(one_rank_group[2].shape) == (2,)


# ---- 4. LDPHierAgent: two handles, both training their planner slot -----------------------------------------------------------------------------
def test_hier_update_trains_two_handles(philox):
    ag0 = _hier()
    eng, ieng = ag0._engine, ag0._idm_engine
    batch = _batch(1)
    ag1, m = ag0.update(batch, SEED, 0)
    assert eng.kinds() == ["load"] + ["stats"] * (2 + len(OBS_KEYS)) + ["planner_grad", "apply", "grad_norm"]
    assert ieng.kinds() == ["load", "planner_grad", "apply", "grad_norm"]                # each handle: apply before grad_norm
    for e in (eng, ieng):
        assert [c[1] for c in e.of("load") + e.of("apply")] == ["planner", "planner"] and e.of("grad_norm") == [("grad_norm", ["planner"])]
    emb, act = _emb(ag0, batch)
    ih, K = 2, FUTURE // 2
    (_, x0, _, tp, cond, w_p), = eng.of("planner_grad")
    (_, a, eps_i, ti, s, w_i), = ieng.of("planner_grad")                                  # train_planner_grad(a, eps, t, s, alpha)
    assert torch.equal(x0, emb[:, OH::ih]) and tuple(x0.shape) == (B, K, D) and torch.equal(cond, emb[:, :OH].reshape(B, -1))
    assert torch.equal(s, torch.cat([emb[:, OH - 1:-1:ih], emb[:, OH - 1 + ih::ih]], dim=-1).reshape(-1, 2 * D)) and tuple(s.shape) == (B * K, 2 * D)
    assert torch.equal(a, act[:, OH - 1:-1].reshape(B * K, ih, A)) and tuple(eps_i.shape) == (B * K, ih, A)
    t_plan, t_idm = _draws(SEED, (B, N_PLAN), (B * K, N_IDM))
    np.testing.assert_array_equal(tp, t_plan)
    np.testing.assert_array_equal(ti, t_idm)
    assert philox == [(SEED, 0, 0, 8, a.numel()), (SEED, 0, 0, 7, x0.numel())] and (w_p, w_i) == (1.0, 1.0)
    assert eng.of("apply")[0][2] == float(np.float32(sched_p(0))) and ieng.of("apply")[0][2] == float(np.float32(sched_i(0)))
    assert list(m) == LDP_KEYS and m["planner_lr"] == np.float32(sched_i(0)) and float(m["g_norm"]) == 5.0      # sqrt(3^2 + 4^2)
    assert float(m["loss"]) == 2 * TrainStub.PLAN_LOSS                                    # both losses come from train_planner_grad
    ag2, _ = ag1.update(batch, SEED, 1)
    assert "load" not in eng.kinds()[1:] + ieng.kinds()[1:]
    with pytest.raises(RuntimeError, match="superseded"):
        ag1.idm_state.params
    assert ieng.of("read") == [] and float(ag2.idm_state.params["Dense_0/bias"][0]) == ieng.TRAIN_PARAMS and len(ieng.of("read")) == 1


# ---- 5. DPVAEAgent.update ---------------------------------------------------------------------------------------------------------------------
def _dp(use_ema=False):
    cfg = dict(n_diffusion_steps=N_PLAN, lowdim_obs=DATA["lowdim_obs"], rgb_obs=DATA["rgb_obs"], obs_horizon=2, name="dp", action_dim=A,
               pred_horizon=8, action_horizon=4, random_shift=0, use_ema=use_ema, vae_feature_dim=16, obs_dim=D, planner_ema_decay=0.75)
    return DPVAEAgent(DPState({"w": np.zeros(1, np.float32)}, None, ema_is_params=True), None, DATA["obs_normalization"], cfg, TrainStub(),
                      W.PlannerSpec(A, 2 * D), W.VAESpec(), torch.device("cpu"), lr_schedule=sched_p)


def test_dp_vae_update_trains_with_the_ema(philox):
    ag0 = _dp()
    eng = ag0._engine
    batch = cfgs.synth_latent_batch(DATA, B, 8, 3, with_actions=True)
    ag1, m = ag0.update(batch, SEED, 0)
    assert eng.kinds() == ["load", "ema"] + ["stats"] * (2 + len(OBS_KEYS)) + ["planner_grad", "apply"]
    assert eng.of("ema") == [("ema", "planner", 0.75)] and eng.train_ema_token["planner"] == ag1.planner_state.ema_version
    assert eng.train_token["planner"] == ag1.planner_state.version
    (_, x0, eps, t, cond, w), = eng.of("planner_grad")
    np.testing.assert_array_equal(t, _draws(SEED, (B, N_PLAN))[0])
    assert tuple(x0.shape) == (B, 8, A) and tuple(cond.shape) == (B, 2 * D) and w == 1.0 and philox == [(SEED, 0, 0, 7, B * 8 * A)]
    assert list(m) == (["loss", "obs_min", "obs_max", "obs_mean", "obs_std", "action_min", "action_max"]
                       + [f"{k}_{s}" for k in OBS_KEYS for s in ("min", "max", "mean", "std")] + ["planner_lr", "planner_step"])
    assert m["planner_lr"] == np.float32(sched_p(0)) and m["planner_step"] == 0 and float(m["loss"]) == TrainStub.PLAN_LOSS
    ag2, _ = ag1.update(batch, SEED, 1)
    assert eng.kinds().count("load") == 1 and eng.kinds().count("ema") == 1 and ag2.planner_state.step == 2
    assert float(ag2.planner_state.ema_params["Dense_0/bias"][0]) == eng.TRAIN_EMA        # read from the EMA arena
    assert float(ag2.planner_state.params["Dense_0/bias"][0]) == eng.TRAIN_PARAMS
    with pytest.raises(RuntimeError, match="superseded"):
        ag1.planner_state.params
    with pytest.raises(RuntimeError, match="superseded"):
        ag1.planner_state.ema_params
    # a distinct EMA tree is written over the arena's copy of the parameters
    other = ag0.replace(planner_state=ag0.planner_state.replace(ema_params={"w": np.ones(1, np.float32)}))
    del eng.calls[:]
    other.update(batch, SEED, 0)
    assert eng.kinds()[:2] == ["load", "write"] and eng.of("write") == [("write", "planner", eng.TRAIN_EMA)]


# ---- 6. the sampling-side hand-off -------------------------------------------------------------------------------------------------------------
def test_sampling_slots_are_filled_from_the_cheapest_source(philox):
    ag = _ldp().replace(vae_params={"v": np.zeros(1, np.float32)})
    eng = ag._engine
    ag._sync_weights(need_vae=True)                                            # foreign states: one upload of all three trees
    (_, trees, versions), = eng.calls
    assert sorted(trees) == ["idm", "planner", "vae"] and trees["planner"] is ag.planner_state.params
    assert versions == {"planner": ag.planner_state.version, "idm": ag.idm_state.version, "vae": ag._vae_version}
    ag._sync_weights(need_vae=True)                                            # the engine holds the tokens: no call
    assert len(eng.calls) == 1
    ag1, _ = ag.update(_batch(1), SEED, 0)
    del eng.calls[:]
    ag1._sync_weights()                                                        # trained states: published from the arenas
    assert eng.calls == [("publish", ["planner"], {"planner": ag1.planner_state.version}), ("publish", ["idm"], {"idm": ag1.idm_state.version})]
    ag1._sync_weights()
    assert len(eng.calls) == 2
    with pytest.raises(ValueError, match="VAE weights"):
        _ldp()._sync_weights(need_vae=True)


def test_hier_sampling_slots_use_both_handles(philox):
    ag = _hier()
    ag._sync_weights()
    assert [sorted(e.calls[0][1]) for e in (ag._engine, ag._idm_engine)] == [["planner"], ["planner"]]
    assert ag._idm_engine.loaded["planner"] == ag.idm_state.version
    ag1, _ = ag.update(_batch(1), SEED, 0)
    ag1._sync_weights()
    assert ag1._engine.calls[-1] == ("publish", ["planner"], {"planner": ag1.planner_state.version})
    assert ag1._idm_engine.calls[-1] == ("publish", ["planner"], {"planner": ag1.idm_state.version})


def test_a_trained_ema_is_published_from_its_arena(philox):
    batch = cfgs.synth_latent_batch(DATA, B, 8, 3, with_actions=True)
    for use_ema in (False, True):
        ag, _ = _dp(use_ema=use_ema).update(batch, SEED, 0)
        eng, st = ag._engine, ag.planner_state
        del eng.calls[:]
        ag._sync_weights()
        ag._sync_weights()
        assert eng.calls == [("publish_ema", ["planner"], {"planner": st.ema_version}) if use_ema else ("publish", ["planner"], {"planner": st.version})]
    fresh = _dp(use_ema=True)                                                  # never trained: the EMA (= the parameters) is uploaded
    fresh._sync_weights()
    (_, trees, versions), = fresh._engine.calls
    assert trees["planner"] is fresh.planner_state.params and versions == {"planner": fresh.planner_state.ema_version}
    # StableVAEModel: the same three-way choice on the "vae" slot, counted in `uploads`
    cfg = dict(rgb_obs=["agentview_image"], name="stable_vae_model", use_kl=True, beta=1e-5, n_downsample=6, data_name="rm_lift")
    m = StableVAEModel(DPState({"w": np.zeros(1, np.float32)}, None, ema_is_params=True), {"obs": {"agentview_image": dict(min=0.0, max=255.0)}},
                       cfg, TrainStub(), W.VAESpec(), 64, "cpu", lr_schedule=sched_p, ema_decay=0.99)
    m1, _ = m.update({"obs": {"agentview_image": np.zeros((2, 1, 64, 64, 3), np.float32)}}, 0, 0)
    del m._engine.calls[:]
    m1._sync_weights(use_ema=True)
    m1._sync_weights(use_ema=True)
    m1._sync_weights(use_ema=False)
    assert m._engine.kinds() == ["publish_ema", "publish"] and m1.uploads == 2
