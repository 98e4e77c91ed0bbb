"""Composed planning without a GPU: the step sizes and constraint levels on a timestep table, the float64 restatement of
tests/compose_oracle.py against the solver's and the guide's oracles, the host logic of LDPAgent.plan / Controller.act on a recording stub
engine, and the agreement of header, binding and export map on the three new symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from latent_diffusion_planning_amd import _lib, constrain as CN, guide as GD, schedule, weights as W
from latent_diffusion_planning_amd.agent import LDPAgent, ParamState
from latent_diffusion_planning_amd.replan import Controller, Replanner, group_rows
from tests import cfgs, compose_oracle as XO, guide_oracle as GO, solver_oracle as SO
from tests.test_replan_cpu import ReplanStub
from tests.util import rng

DATA = cfgs.RM_LIFT
D, A, T, AH = 25, 7, 8, 4
CFG = dict(pred_horizon=T, obs_dim=D, action_horizon=AH, vae_feature_dim=16, rgb_obs=["latent_agentview_image"], planner_n_diffusion_steps=100)
NEW = ("ldp_plan_compose_step", "ldp_plan_sample_composed", "ldp_agent_sample_composed")


# ---- 1. step sizes and constraint levels on a timestep table --------------------------------------------------------------------------
@pytest.mark.parametrize("sched", ["sigma2", "constant", "table"])
def test_step_sizes_on_agrees_with_step_sizes_on_the_uniform_grid(sched):
    g = rng(1)
    n = 10
    table = np.linspace(0.3, 0.05, n)
    gd = GD.build_guide(CFG, 2, goal=g.uniform(-1, 1, (2, D)), smooth=0.1, scale=0.2, schedule=table if sched == "table" else sched)
    ts = schedule.step_timesteps(100, n, schedule.SAMPLER_DDIM)
    on = gd.step_sizes_on(ts)
    assert on.dtype == np.float32 and np.array_equal(on, gd.step_sizes(n, "ddim"))
    if sched == "sigma2":
        acp = schedule.make_schedule(100).alphas_cumprod.astype(np.float64)
        log = schedule.solver_timesteps(100, n, "logsnr")
        assert np.array_equal(gd.step_sizes_on(log), (0.2 * (1.0 - acp[log])).astype(np.float32))
        assert not np.array_equal(gd.step_sizes_on(log), on)
        with pytest.raises(NotImplementedError, match="dpmpp"):
            gd.step_sizes(n, "dpmpp")                                          # (the uniform-grid method keeps refusing)
    with pytest.raises(ValueError, match="timesteps"):
        gd.step_sizes_on([100, 50, 0])


def test_step_sizes_on_refuses_a_step_beyond_the_descent_bound():
    gd = GD.build_guide(CFG, 1, goal=np.zeros((1, D), np.float32), smooth=0.25, scale=1.0, schedule="sigma2")      # L = 2
    assert gd.lipschitz == 2.0
    with pytest.raises(ValueError, match="> 1"):
        gd.step_sizes_on([90, 50, 0])                                          # 1 - abar_90 is close to 1: rho L close to 2
    ok = gd.step_sizes_on([10, 5, 0])
    assert float(ok.max()) * gd.lipschitz <= 1.0


def test_table_level_coefs():
    for n in (10, 20):
        ts = schedule.step_timesteps(100, n, schedule.SAMPLER_DDIM)
        got = CN.table_level_coefs(100, ts)
        assert got.dtype == np.float32 and got.shape == (n + 1, 2) and np.array_equal(got, CN.level_coefs(100, n))
        assert got[n].tolist() == [1.0, 0.0]
    log = schedule.solver_timesteps(100, 10, "logsnr")
    got = CN.table_level_coefs(100, log)
    acp = schedule.make_schedule(100).alphas_cumprod
    for j, t in enumerate(log):
        a = float(np.float32(acp[t]))
        assert got[j].tolist() == [float(np.float32(np.sqrt(a))), float(np.float32(np.sqrt(1.0 - a)))]
        assert XO.level_coefs(j, "dpmpp", 100, 10, log) == (np.sqrt(a), np.sqrt(1.0 - a))
    assert got[10].tolist() == [1.0, 0.0] and XO.level_coefs(10, "dpmpp", 100, 10, log) == (1.0, 0.0)
    with pytest.raises(ValueError, match="timesteps"):
        CN.table_level_coefs(100, [100, 0])


# ---- 2. the float64 oracle ---------------------------------------------------------------------------------------------------------------
def _eps_fn(x, t):
    return 0.6 * np.tanh(x) + 0.002 * t


def _guide(g, B, anchor=True):
    return GO.make(B, T, D, target=g.uniform(-1, 1, (B, T, D)), wg=g.uniform(0, 2, (B, T, D)) * (g.uniform(size=(B, T, D)) < 0.5),
                   anchor=g.uniform(-1, 1, (B, D)) if anchor else None, lam=g.uniform(0, 0.5, D), beta=g.uniform(0, 3, D),
                   lo=-0.6 * g.uniform(0.5, 1, D), hi=0.6 * g.uniform(0.5, 1, D))


def test_oracle_without_parts_is_the_solver_oracle():
    g = rng(2)
    ts = schedule.solver_timesteps(100, 10, "logsnr")
    x = g.standard_normal((2, T, D))
    for begin, end in ((0, 10), (3, 10), (0, 4)):
        got = XO.composed_loop(_eps_fn, x, begin, end, sampler="dpmpp", n_steps=10, ts=ts)
        assert np.array_equal(got, SO.solve(_eps_fn, x, ts, begin, end))
    # the rows the kernel holds (quotients) and the rows of the float64 loops (exp(-h)) are the same numbers to float64 round-off
    for i in range(10):
        q, e = XO.step_row("dpmpp", i, 100, 10, ts), XO.step_row("dpmpp", i, 100, 10, ts, quotient=False)
        assert all(abs(q[k] - e[k]) <= 1e-12 for k in XO.KEYS)


def test_oracle_with_a_guide_under_ddim_is_the_guide_oracle():
    g = rng(3)
    G = _guide(g, 2)
    rho = np.linspace(1.0, 0.2, 10) / GO.lipschitz(G)
    x = g.standard_normal((2, T, D))
    ref = x
    for i in range(10):
        k = GO.step_coefs(i, 100, 10, "ddim")
        eps = _eps_fn(ref, int(k[0]))
        one, yg = XO.compose_step(ref, eps, XO.step_row("ddim", i, 100, 10), G, rho[i])
        ref = GO.guided_step(ref, eps, G, rho[i], k)
        assert np.array_equal(one, ref) and np.abs(yg).max() <= 1.0
    assert np.array_equal(XO.composed_loop(_eps_fn, x, 0, 10, sampler="ddim", n_steps=10, G=G, rho=rho), ref)
    # DDPM with sigma > 0 reads the step noise
    z = g.standard_normal((2, T, D))
    k = GO.step_coefs(3, 100, 100, "ddpm")
    eps = _eps_fn(x, 96)
    assert k[6] > 0 and np.array_equal(XO.compose_step(x, eps, XO.step_row("ddpm", 3, 100, 100), G, 0.1, z)[0], GO.guided_step(x, eps, G, 0.1, k, z))


def test_oracle_constraint_is_a_select_after_the_update_and_spares_the_history():
    g = rng(4)
    G = _guide(g, 2)
    ts = schedule.solver_timesteps(100, 10, "logsnr")
    x, eps, h = g.standard_normal((2, T, D)), g.standard_normal((2, T, D)), g.uniform(-1, 1, (2, T, D))
    target = g.uniform(-1, 1, (2, T, D))
    target[0, 0, 0] = np.nan                                                   # under a zero mask: never reaches the state
    mask = np.zeros((2, T, D), bool)
    mask[:, 3] = True
    z = g.standard_normal((2, T, D))
    k = XO.step_row("dpmpp", 4, 100, 10, ts)
    free, yg = XO.compose_step(x, eps, k, G, 0.05, h_prev=h, second=True, solver=True)
    for mode, level in (("clamp", 5), ("repaint", 5), ("repaint", 10)):
        c = XO.constraint(target, mask, mode, level, "dpmpp", 100, 10, ts, z)
        got, yg2 = XO.compose_step(x, eps, k, G, 0.05, h_prev=h, second=True, cons=c, solver=True)
        assert np.array_equal(got[~mask], free[~mask]) and np.array_equal(yg2, yg) and np.isfinite(got).all()
        a, s = XO.level_coefs(level, "dpmpp", 100, 10, ts)
        want = target if mode == "clamp" or level == 10 else a * target + s * z
        assert np.array_equal(got[mask], want[mask])
    # the float32 emulation is within the bound of the float64 step it restates
    k32 = XO.step_row("dpmpp", 4, 100, 10, ts, cast32=True)
    G32 = G
    c = XO.constraint(np.nan_to_num(target).astype(np.float32), mask, "repaint", 5, "dpmpp", 100, 10, ts, z.astype(np.float32), cast32=True)
    args = (x.astype(np.float32), eps.astype(np.float32), k32, G32, float(np.float32(0.05)))
    kw = dict(h_prev=h.astype(np.float32), second=True, cons=c, solver=True)
    emu, emu_y = XO.emulate_step(*args, **kw)
    ref, ref_y = XO.compose_step(*args, **kw)
    bx, by = XO.step_bound(*args, **kw)
    assert (np.abs(emu - ref) <= bx).all() and (np.abs(emu_y - ref_y) <= by).all() and (np.abs(emu - ref) > 0).any()


# ---- 3. LDPAgent.plan and Controller.act on a stub engine ---------------------------------------------------------------------------------
class ComposeStub(ReplanStub):
    """ReplanStub plus the composed call: records what reached it."""
    solver_tables = {}

    def set_solver_timesteps(self, ts):
        self.solver_tables = dict(self.solver_tables)
        self.solver_tables[len(ts)] = np.asarray(ts, np.int64)

    def plan_guide_cost(self, x, guide, n_per=1):
        self.calls.append(("plan_guide_cost", x.shape[0]))
        return torch.zeros(x.shape[0])

    def mean_sq_diff(self, a, b):
        return ((a - b) ** 2).mean().reshape(1)

    def agent_sample_composed(self, obs_emb, obs_horizon, *, guide=None, rho=None, target=None, mask=None, mode="repaint", x_store=None,
                              slot=None, shift=None, step_begin=0, seed=0, row_offset=0, sampler="ddim", planner_steps=None, idm_steps=None,
                              **kw):
        B = obs_emb.shape[0]
        self.calls.append(("agent_sample_composed", B, row_offset, seed, sampler, planner_steps, idm_steps, step_begin,
                           None if slot is None else [int(v) for v in slot], shift,
                           dict(guide=guide, rho=rho, target=target, mask=mask, mode=mode, x_store=None if x_store is None else x_store.clone(),
                                who=obs_emb[:, 0, 0].clone(), kw=kw)))
        self.call_seq += 1
        x, plan, act = self._result(obs_emb, row_offset, x_store is not None)
        if x_store is not None:
            idx = torch.arange(B) if slot is None else torch.as_tensor(slot)
            x_store[idx] = x
        return x, plan, act


@pytest.fixture
def agent(monkeypatch):
    monkeypatch.setattr(W, "check_params", lambda tree, shapes: None)          # the stub's trees hold one leaf
    cfg = dict(lowdim_obs=DATA["lowdim_obs"], rgb_obs=DATA["rgb_obs"], obs_horizon=1, pred_horizon=T, action_horizon=AH, obs_dim=D,
               action_dim=A, vae_feature_dim=16, planner_n_diffusion_steps=100, idm_n_diffusion_steps=100, name="ldp_agent")
    st = lambda: ParamState({"w": np.zeros(1, np.float32)})                    # noqa: E731
    return LDPAgent(st(), st(), None, DATA["obs_normalization"], True, True, 1, 1, cfg, ComposeStub(), W.PlannerSpec(D, D), W.IDMSpec(D, A),
                    W.VAESpec(), torch.device("cpu"))


def _composed(eng):
    return [c for c in eng.calls if c[0].startswith("agent_")]


def test_plan_routes_every_part_to_one_engine_call(agent):
    eng = agent._engine
    B = 2
    b = cfgs.synth_latent_batch(DATA, B, 1, 5)
    goal = rng(6).uniform(-1, 1, (B, D)).astype(np.float32)
    gd = agent.build_guide(B, smooth=0.1, anchor=True, scale=0.5, schedule="sigma2")
    prev = torch.full((B, T, D), 5.0)
    action, m = agent.plan(b, 3, guide=gd, goal=goal, t_goal=[1, 3], goal_dims="latent", mode="clamp", prev=prev, warm_steps=4,
                           sampler="dpmpp", n_steps=10, row_offset=6)
    (c,) = _composed(eng)
    assert c[:10] == ("agent_sample_composed", B, 6, 3, "dpmpp", 10, 10, 6, None, AH)
    p = c[10]
    ts = eng.solver_tables.get(10, schedule.solver_timesteps(100, 10, "logsnr"))
    assert np.array_equal(p["rho"], gd.step_sizes_on(ts)) and p["mode"] == "clamp"
    assert torch.equal(p["x_store"], prev) and torch.equal(prev, torch.full((B, T, D), 5.0))      # the write-back went to a copy
    mk = np.asarray(p["mask"])
    want = np.zeros((B, T, D), np.uint8)
    want[:, [1, 3], :16] = 1
    assert np.array_equal(mk, want) and np.array_equal(np.asarray(p["target"])[:, 1, :16], goal[:, :16])
    assert p["guide"] is not gd and tuple(p["guide"].anchor.shape) == (B, D) and torch.equal(p["guide"].anchor[:, 0], p["who"])
    assert gd.anchor is True                                                   # (the caller's guide is not modified)
    assert sorted(m) == ["guide_cost", "plan", "plan_viz", "x"] and action.shape == (B, AH, A) and np.array(m["x"]).shape == (B, T, D)
    # no parts at all: still one composed call, cold; a training batch reports plan_mse
    del eng.calls[:]
    _, m0 = agent.plan(cfgs.synth_latent_batch(DATA, B, T + 1, 5), 3, n_steps=10)
    (c,) = _composed(eng)
    assert c[:10] == ("agent_sample_composed", B, 0, 3, "ddim", 10, 10, 0, None, None)
    assert all(c[10][k] is None for k in ("guide", "rho", "target", "mask", "x_store")) and sorted(m0) == ["plan", "plan_mse", "plan_viz", "x"]
    # explicit timesteps are registered with the engine and give the guide its step sizes
    del eng.calls[:]
    mine = [90, 60, 30, 10, 0]
    agent.plan(b, 3, guide=agent.build_guide(B, smooth=0.1, scale=0.5), sampler="dpmpp", n_steps=5, timesteps=mine)
    (c,) = _composed(eng)
    acp = schedule.make_schedule(100).alphas_cumprod.astype(np.float64)
    assert eng.solver_tables[5].tolist() == mine and np.array_equal(c[10]["rho"], (0.5 * (1.0 - acp[mine])).astype(np.float32))


def test_plan_refuses_before_anything_reaches_the_engine(agent):
    eng = agent._engine
    B = 2
    b = cfgs.synth_latent_batch(DATA, B, 1, 5)
    prev = torch.zeros(B, T, D)
    gd = agent.build_guide(B, smooth=0.25, goal=np.zeros((B, D), np.float32), scale=1.0)      # L = 2, scale 1: beyond the bound at high noise
    cases = [
        (dict(mode="blend"), ValueError, "mode"),
        (dict(guide=object()), ValueError, "guide.Guide"),
        (dict(prev=prev), ValueError, "go together"),
        (dict(warm_steps=3), ValueError, "go together"),
        (dict(prev=prev, warm_steps=0, n_steps=10), ValueError, "warm_steps"),
        (dict(prev=prev, warm_steps=11, n_steps=10), ValueError, "warm_steps"),
        (dict(prev=prev, warm_steps=2, n_steps=10, shift=-1), ValueError, "shift"),
        (dict(shift=2), ValueError, "shift"),
        (dict(prev=prev, warm_steps=2, n_steps=10, noise=dict(x_init=prev)), ValueError, "x_init"),
        (dict(target=prev), ValueError, "target and mask"),
        (dict(t_goal=2), ValueError, "goal"),
        (dict(guide=gd, n_steps=10), ValueError, "> 1"),
        (dict(guide=gd, sampler="dpmpp", n_steps=10), ValueError, "> 1"),
        (dict(timesteps="logsnr"), ValueError, "dpmpp"),
        (dict(sampler="dpmpp", n_steps=7), ValueError, "idm_steps"),
        (dict(sampler="dpmpp", n_steps=10, timesteps=[5, 0]), ValueError, "timesteps"),
    ]
    for kw, exc, word in cases:
        with pytest.raises(exc, match=word):
            agent.plan(b, 0, **kw)
    assert not _composed(eng) and not [c for c in eng.calls if c[0] == "plan_guide_cost"]
    # found once the batch is embedded, still before the engine's sampling call
    for kw, word in ((dict(guide=agent.build_guide(3, smooth=0.1)), "B = 3"), (dict(goal=np.zeros((3, D), np.float32)), "goal"),
                     (dict(goal=np.zeros((B, D), np.float32), t_goal=T), "t_goal"),
                     (dict(prev=torch.zeros(3, T, D), warm_steps=2, n_steps=10), "prev")):
        with pytest.raises(ValueError, match=word):
            agent.plan(b, 0, **kw)
    assert not _composed(eng)
    half = type("P", (), dict(use_planner=True, use_idm=False))()
    with pytest.raises(NotImplementedError, match="planner and the IDM"):
        LDPAgent.plan(half, b, 0)
    with pytest.raises(NotImplementedError, match="planner and the IDM"):
        LDPAgent.controller(half, 2, 1)


def test_controller_groups_like_replanner_and_hands_each_group_its_rows(agent):
    eng = agent._engine
    ct = agent.controller(6, warm_steps=2, sampler="dpmpp", n_steps=10)
    assert isinstance(ct, Controller) and isinstance(ct, Replanner) and (ct.step_begin, ct.shift, ct.n_steps, ct.idm_steps) == (8, AH, 10, 10)
    g = rng(8)
    b1 = cfgs.synth_latent_batch(DATA, 2, 1, 1)
    _, m1 = ct.act(b1, 7, [4, 2])                                              # no parts: both rows cold, one call
    (c,) = _composed(eng)
    assert c[:10] == ("agent_sample_composed", 2, 0, 7, "dpmpp", 10, 10, 0, None, None) and ct.calls == dict(warm=0, cold=1)
    x1 = np.array(m1["x"])
    assert np.array_equal(ct.table[4].numpy(), x1[0]) and np.array_equal(ct.table[2].numpy(), x1[1])

    # rows (slot 0: cold, slot 2: warm, slot 5: cold, slot 4: warm) with a guide and a goal for each row
    del eng.calls[:]
    slots = [0, 2, 5, 4]
    order, n_warm = group_rows(ct.valid, slots)
    assert (order, n_warm) == ([1, 3, 0, 2], 2)
    B = 4
    goal = g.uniform(-1, 1, (B, D)).astype(np.float32)
    tgt = g.uniform(-1, 1, (B, T, D)).astype(np.float32)
    gd = agent.build_guide(B, target=tgt, weight=1.0, smooth=0.1, anchor=g.uniform(-1, 1, (B, D)).astype(np.float32), scale=0.1)
    b2 = cfgs.synth_latent_batch(DATA, B, 1, 2)
    who = agent.get_obs_cond(agent._postprocess(b2)["obs"])[:, 0, 0].numpy()
    _, m2 = ct.act(b2, 9, slots, guide=gd, goal=goal, mode="clamp")
    warm, cold = _composed(eng)
    assert warm[:10] == ("agent_sample_composed", 2, 0, 9, "dpmpp", 10, 10, 8, [2, 4], AH)
    assert cold[:10] == ("agent_sample_composed", 2, 2, 9, "dpmpp", 10, 10, 0, None, None)
    ts = eng.solver_tables.get(10, schedule.solver_timesteps(100, 10, "logsnr"))
    for call, rows in ((warm, [1, 3]), (cold, [0, 2])):
        p = call[10]
        assert np.array_equal(p["who"].numpy(), who[rows]) and p["mode"] == "clamp"
        assert np.array_equal(np.asarray(p["guide"].target), tgt[rows]) and np.array_equal(np.asarray(p["guide"].anchor), np.asarray(gd.anchor)[rows])
        assert p["guide"].B == 2 and np.array_equal(p["rho"], gd.step_sizes_on(ts))
        assert np.array_equal(np.asarray(p["target"])[:, AH - 1], goal[rows]) and np.asarray(p["mask"])[:, AH - 1].all()
        assert np.asarray(p["mask"]).sum() == 2 * D
    assert np.array_equal(warm[10]["x_store"][[2, 4]].numpy(), x1[[1, 0]])    # each warm row read ITS slot's previous state
    x2 = np.array(m2["x"])
    assert np.array_equal(x2[:, 0, 0], who) and x2[:, 0, 2].tolist() == [0.0, 1.0, 0.0, 1.0] and x2[:, 0, 1].tolist() == [2.0, 0.0, 3.0, 1.0]
    for row, slot in enumerate(slots):
        assert np.array_equal(ct.table[slot].numpy(), x2[row])
    assert ct.calls == dict(warm=1, cold=2)
    # a slot reset in between: slot 2 cold again
    ct.reset([2])
    del eng.calls[:]
    ct.act(cfgs.synth_latent_batch(DATA, 2, 1, 3), 1, [2, 4])
    assert [(c[1], c[2], c[7], c[8]) for c in _composed(eng)] == [(1, 0, 8, [4]), (1, 1, 0, None)]
    # refusals: nothing reaches the engine
    del eng.calls[:]
    b = cfgs.synth_latent_batch(DATA, 2, 1, 4)
    for kw, exc, word in ((dict(mode="blend"), ValueError, "mode"), (dict(guide=object()), ValueError, "guide.Guide"),
                          (dict(guide=gd), ValueError, "B = 4"), (dict(weight=1.0), TypeError, "weight"),
                          (dict(target=tgt[:2]), ValueError, "target and mask"), (dict(t_goal=1), ValueError, "goal"),
                          (dict(guide=agent.build_guide(2, smooth=0.25, goal=goal[:2], scale=1.0)), ValueError, "> 1")):
        with pytest.raises(exc, match=word):
            ct.act(b, 0, [0, 1], **kw)
    with pytest.raises(ValueError, match="distinct"):
        ct.act(b, 0, [1, 1], guide=gd)
    assert not _composed(eng)
    # the plain Replanner still makes the calls it always made
    rp = agent.replanner(2, warm_steps=2, n_steps=10)
    rp.act(b, 0, [0, 1])
    rp.act(b, 0, [0, 1])
    assert [c[0] for c in _composed(eng)] == ["agent_sample", "agent_resample"]


def test_other_agents_name_ldp_agent():
    from latent_diffusion_planning_amd.dp_agent import DPAgent
    from latent_diffusion_planning_amd.dp_vae_agent import DPVAEAgent
    from latent_diffusion_planning_amd.hier_agent import LDPHierAgent
    for cls in (LDPHierAgent, DPVAEAgent, DPAgent):
        for name in ("plan", "controller"):
            with pytest.raises(NotImplementedError, match="LDPAgent"):
                getattr(cls, name)(object())


# ---- 4. header, binding and export map -----------------------------------------------------------------------------------------------------
def test_the_three_symbols_agree_in_header_binding_and_export_map():
    syms = _lib.header_symbols()
    assert len(syms) == 80 and sorted(_lib.SIGNATURES) == syms
    with open(_lib.HEADER_PATH) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in NEW:
        assert name in syms
        m = re.search(r"LDP_API\s+int\s+" + name + r"\s*\((.*?)\)\s*;", txt, flags=re.S)
        assert m, name
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(m.group(1).split(",")), name
        assert "const ldp_plan_compose* parts" in m.group(1)
    # the struct: the same fields in the same order as the header's
    body = re.search(r"typedef struct ldp_plan_compose \{(.*?)\} ldp_plan_compose;", txt, flags=re.S).group(1)
    names = re.findall(r"[\*\s,]([a-z_0-9]+)\s*(?=[;,])", body)
    assert names == [f[0] for f in _lib.LdpPlanCompose._fields_]
    with open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "exports.map")) as f:
        assert "global: ldp_*;" in f.read()                                    # every ldp_ entry point is exported by pattern
    with open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "Makefile")) as f:
        assert "compose.hip" in f.read()
