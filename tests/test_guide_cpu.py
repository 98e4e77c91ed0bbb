"""Guided planning without a GPU: the float64 oracle's own properties (tests/guide_oracle.py: the gradient against
central differences, the descent bound, the exact fma of the float32 emulation), guide.build_guide, the refusals, the host logic of
LDPAgent.sample_guided on a recording stub engine, and the ABI listing."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from latent_diffusion_planning_amd import _lib, guide as GD, schedule, weights as W
from latent_diffusion_planning_amd.agent import LDPAgent, ParamState
from oracle import np64
from tests import cfgs, guide_oracle as GO, replan_oracle as RO
from tests.train_stub import TrainStub
from tests.util import planner_params, rng

DATA = cfgs.RM_LIFT
T, D, A, AH, LAT = 8, 25, 7, 4, 16
CFG = dict(pred_horizon=T, obs_dim=D, action_horizon=AH, vae_feature_dim=LAT, rgb_obs=["agentview_image"], planner_n_diffusion_steps=100)


def _random_guide(g, B, T=T, D=D, anchor=True, box=0.6):
    """Weights of every kind switched on, and a box narrower than [-1, 1] so that the hinge is active on some entries."""
    return GO.make(B, T, D, target=g.uniform(-1, 1, (B, T, D)), wg=g.uniform(0, 2, (B, T, D)) * (g.uniform(size=(B, T, D)) < 0.5),
                   anchor=g.uniform(-1, 1, (B, D)) if anchor else None, lam=g.uniform(0, 0.5, D), beta=g.uniform(0, 3, D),
                   lo=-box * g.uniform(0.5, 1, D), hi=box * g.uniform(0.5, 1, D))


# ---- the float64 oracle ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("anchor", [False, True], ids=["free", "anchor"])
def test_gradient_matches_central_differences(anchor):
    """g against (J(y + h e) - J(y - h e)) / 2h at h = 1e-6, every element.  J is piecewise quadratic: the difference quotient is exact up
    to round-off away from the hinge's kinks, and within h of one it is off by at most beta h / 2."""
    g = rng(11)
    B, Ts, Ds = 2, 4, 6
    G = _random_guide(g, B, Ts, Ds, anchor)
    y = g.uniform(-1, 1, (B, Ts, Ds))
    got, h, worst = GO.grad(y, G), 1e-6, 0.0
    for idx in np.ndindex(B, Ts, Ds):
        e = np.zeros_like(y)
        e[idx] = h
        fd = (GO.cost(y + e, G)[idx[0]] - GO.cost(y - e, G)[idx[0]]) / (2 * h)
        worst = max(worst, abs(fd - got[idx]))
    print(f"max |g - central difference| = {worst:.2e}")
    assert worst < 1e-8
    assert np.abs(got).max() > 0.1                                             # (not a comparison of zeros)


def test_descent_at_the_largest_allowed_step():
    """J(clip(y - g / L)) <= J(y) for every sample: L = max wg + 4 max lam + max beta bounds the Lipschitz constant of g, and the box
    [-1, 1]^n is convex, so a projected gradient step of 1 / L cannot increase J."""
    g = rng(12)
    n = 0
    for trial in range(60):
        B = 50
        G = _random_guide(g, B, anchor=trial % 2 == 0, box=g.uniform(0.2, 1.2))
        y = np.clip(g.standard_normal((B, T, D)) * g.uniform(0.3, 2.0), -1, 1)
        L = GO.lipschitz(G)
        before, after = GO.cost(y, G), GO.cost(GO.project(y, G, 1.0 / L), G)
        assert (after <= before * (1 + 1e-12)).all(), float((after - before).max())
        assert (after < before).any()
        n += B
    assert n == 3000


def test_fma32_is_exact():
    g = rng(13)
    a, b = g.standard_normal(4000).astype(np.float32), g.standard_normal(4000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + g.uniform(-1, 1, 4000) * 2.0 ** g.integers(-30, 0, 4000))).astype(np.float32)
    got = GO.fma32(a, b, c)                                                    # (c close to -a b: cancellation, where double rounding bites)
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        near = np.float32(float(exact))                                        # within one float32 of the answer: pick among its neighbours
        cands = [near, np.nextafter(near, np.float32(np.inf)), np.nextafter(near, np.float32(-np.inf))]
        want = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))      # nearest, ties to even
        assert got[i] == want, (i, a[i], b[i], c[i])


def test_emulation_agrees_with_float64_within_the_bound():
    """The float32 emulation is held to the same bound as the kernel: a bound the emulation broke would be a wrong bound."""
    g = rng(14)
    B = 5
    G = _random_guide(g, B)
    x, eps = (g.standard_normal((B, T, D)) * 1.5).astype(np.float32), g.standard_normal((B, T, D)).astype(np.float32)
    z = g.standard_normal((B, T, D)).astype(np.float32)
    rho = np.float32(1.0 / GO.lipschitz(G))
    for sampler, n, i in (("ddim", 10, 0), ("ddim", 10, 9), ("ddpm", 100, 3), ("ddpm", 100, 99)):
        k = GO.step_coefs(i, 100, n, sampler, cast32=True)
        emu = GO.emulate_step(x, eps, G, rho, k, z)
        ref, bound = GO.guided_step(x, eps, G, float(rho), k, z), GO.step_bound(x, eps, G, float(rho), k, z)
        ratio = float((np.abs(emu - ref) / bound).max())
        print(f"{sampler}-{n} step {i}: max |emulation - float64| / bound = {ratio:.3f}")
        assert ratio <= 1.0


def test_oracle_zero_guide_is_the_free_loop_and_ranges_compose():
    g = rng(15)
    P = np64.to64(planner_params(D=D))
    B, n = 1, 4
    cond, x0 = g.uniform(-1, 1, (B, D)), g.standard_normal((B, T, D))
    G = _random_guide(g, B)
    kw = dict(n_train=100, n_steps=n, sampler="ddim")
    free = RO.planner_range(P, cond, x0, 0, n, **kw)
    zero = GO.planner_range_guided(P, cond, x0, 0, n, G, np.zeros(n), **kw)
    assert np.abs(zero - free).max() < 1e-12
    rho = np.full(n, 1.0 / GO.lipschitz(G))
    whole = GO.planner_range_guided(P, cond, x0, 0, n, G, rho, **kw)
    head = GO.planner_range_guided(P, cond, x0, 0, 2, G, rho, **kw)
    assert np.array_equal(GO.planner_range_guided(P, cond, head, 2, n, G, rho, **kw), whole)
    assert np.abs(whole - free).max() > 1e-2                                   # the guide steers
    # an all-zero weight set is no guide whatever the step size
    none = GO.make(B, T, D)
    assert np.abs(GO.planner_range_guided(P, cond, x0, 0, n, none, np.ones(n), **kw) - free).max() < 1e-12


# ---- build_guide ------------------------------------------------------------------------------------------------------------------------------
def test_build_guide_broadcasts():
    B = 3
    g = rng(21)
    target = g.uniform(-1, 1, (B, T, D)).astype(np.float32)
    for w, want in ((0.5, np.full((B, T, D), 0.5)), (np.arange(D) / D, np.broadcast_to(np.arange(D) / D, (B, T, D))),
                    (g.uniform(0, 1, (T, D)), None), (g.uniform(0, 1, (B, T, D)), None)):
        gd = GD.build_guide(CFG, B, target=target, weight=w, scale=0.0)
        want = np.broadcast_to(np.asarray(w), (B, T, D)) if want is None else want
        assert gd.weight.dtype == np.float32 and np.array_equal(gd.weight, want.astype(np.float32)) and np.array_equal(gd.target, target)
    gd = GD.build_guide(CFG, B, smooth=0.25, bound_weight=np.arange(D), lo=-0.5, hi=np.linspace(0.1, 1, D), anchor=True)
    assert all(getattr(gd, k).shape == (D,) and getattr(gd, k).dtype == np.float32 for k in ("lam", "beta", "lo", "hi"))
    assert np.all(gd.lam == 0.25) and np.array_equal(gd.beta, np.arange(D, dtype=np.float32)) and np.all(gd.lo == -0.5)
    assert gd.anchor is True and not gd.weight.any() and gd.lipschitz == 4 * 0.25 + (D - 1)
    # the goal form: build_constraint's columns and steps, a weight in place of the mask
    goal = g.uniform(-1, 1, (B, D)).astype(np.float32)
    gd = GD.build_guide(CFG, B, goal=goal, t_goal=[1, 7], goal_dims="lowdim", goal_weight=2.0)
    want_w = np.zeros((B, T, D), np.float32)
    want_w[:, [1, 7], LAT:] = 2.0
    assert np.array_equal(gd.weight, want_w) and np.array_equal(gd.target[:, 7, LAT:], goal[:, LAT:]) and not gd.target[:, 7, :LAT].any()
    gd = GD.build_guide(CFG, B, goal=goal)                                     # default: every column at action_horizon - 1, weight 1
    assert np.array_equal(gd.weight[:, AH - 1], np.ones((B, D), np.float32)) and gd.weight.sum() == B * D
    # both forms: the goal's entries win
    gd = GD.build_guide(CFG, B, target=target, weight=0.5, goal=goal, t_goal=2, goal_weight=np.full(D, 1.5))
    assert np.array_equal(gd.target[:, 2], goal) and np.all(gd.weight[:, 2] == 1.5) and np.array_equal(gd.target[:, 3], target[:, 3])
    # torch in, torch out
    gd = GD.build_guide(CFG, B, goal=torch.as_tensor(goal))
    assert torch.is_tensor(gd.target) and torch.is_tensor(gd.weight) and gd.lipschitz == 1.0
    # the empty guide
    gd = GD.build_guide(CFG, B)
    assert gd.lipschitz == 0.0 and not gd.step_sizes(10).any()


def test_step_size_schedules_against_their_formulas():
    B = 2
    gd = GD.build_guide(CFG, B, goal=np.zeros((B, D), np.float32), goal_weight=2.0, smooth=0.25, bound_weight=1.0, scale=0.125, schedule="sigma2")
    assert gd.lipschitz == 2.0 + 1.0 + 1.0
    acp = np64.ddpm_tables(100)[2].astype(np.float64)
    for sampler, n in (("ddim", 10), ("ddim", 50), ("ddpm", 100)):
        ts = np.array([RO.step_timestep(i, 100, n, sampler) for i in range(n)])
        rho = gd.step_sizes(n, sampler)
        assert rho.dtype == np.float32 and np.array_equal(rho, (0.125 * (1.0 - acp[ts])).astype(np.float32))
        assert np.all(np.diff(rho) < 0) and rho[0] < 0.125                     # guidance fades with the noise
    gd.schedule = "constant"
    assert np.array_equal(gd.step_sizes(10), np.full(10, 0.125, np.float32))
    gd.schedule, gd.scale = np.linspace(0.25, 0, 10), None
    assert np.array_equal(gd.step_sizes(10), np.linspace(0.25, 0, 10).astype(np.float32))
    # the default scale is the largest float32 step the bound allows
    for L in (1.9, 3.0, 7.3):
        gd = GD.build_guide(CFG, B, goal=np.zeros((B, D), np.float32), goal_weight=L, schedule="constant")
        rho = gd.step_sizes(5)
        assert float(rho[0]) * gd.lipschitz <= 1.0 < float(np.nextafter(rho[0], np.float32(1))) * gd.lipschitz * (1 + 1e-6)


@pytest.mark.parametrize("kw,word", [
    (dict(target=np.zeros((3, T, D), np.float32)), "weight"),
    (dict(weight=1.0), "target"),
    (dict(target=np.zeros((3, T, D + 1), np.float32), weight=1.0), "target"),
    (dict(target=np.zeros((2, T, D), np.float32), weight=1.0), "target"),
    (dict(target=np.zeros((3, T, D), np.float32), weight=np.ones((T,))), "weight"),
    (dict(target=np.zeros((3, T, D), np.float32), weight=-0.1), "weight"),
    (dict(target=np.zeros((3, T, D), np.float32), weight=np.nan), "weight"),
    (dict(goal=np.zeros((3, D + 1), np.float32)), "goal"),
    (dict(goal=np.zeros((3, D), np.float32), t_goal=T), "t_goal"),
    (dict(goal=np.zeros((3, D), np.float32), goal_dims="pose"), "goal_dims"),
    (dict(goal=np.zeros((3, D), np.float32), goal_weight=-1.0), "goal_weight"),
    (dict(goal=np.zeros((3, D), np.float32), goal_weight=np.ones(D + 1)), "goal_weight"),
    (dict(t_goal=3), "goal"),
    (dict(goal_weight=1.0), "goal"),
    (dict(smooth=-0.5), "smooth"),
    (dict(smooth=np.ones(D - 1)), "smooth"),
    (dict(bound_weight=-1e-3), "bound_weight"),
    (dict(anchor=np.zeros((3, D + 1), np.float32)), "anchor"),
    (dict(lo=0.5, hi=0.25), "lo"),
    (dict(lo=np.linspace(-1, 1, D), hi=0.0), r"lo\[13\]"),
    (dict(hi=np.inf), "hi"),
    (dict(scale=-1.0), "scale"),
    (dict(schedule="linear"), "schedule"),
    (dict(smooth=0.5, scale=0.6, schedule="constant"), r"0\.6.*2.*> 1"),       # rho L = 0.6 * 2 > 1: both numbers are named
    (dict(smooth=0.5, schedule=[0.1, 0.6, 0.1]), "> 1"),
    (dict(schedule=[0.1, -0.1]), "step sizes"),
])
def test_build_guide_refusals_name_the_argument(kw, word):
    with pytest.raises(ValueError, match=word):
        GD.build_guide(CFG, 3, **kw)
    with pytest.raises(ValueError, match="B must"):
        GD.build_guide(CFG, 0)


def test_step_sizes_refuse_a_wrong_length_and_a_step_beyond_the_bound():
    gd = GD.build_guide(CFG, 2, smooth=0.5, schedule=np.full(10, 0.5))
    with pytest.raises(ValueError, match="10 step sizes.*n_steps = 5"):
        gd.step_sizes(5)
    gd = GD.build_guide(CFG, 2, smooth=0.5, scale=0.75, schedule="sigma2")     # L = 2: fine while 1 - abar_t0 <= 2 / 3
    assert gd.step_sizes(2)[0] * 2 <= 1.0                                      # DDIM-2 starts at t = 50
    with pytest.raises(ValueError, match="> 1"):
        gd.step_sizes(10)                                                      # DDIM-10 starts at t = 90: 0.75 * 0.98 * 2 > 1
    with pytest.raises(NotImplementedError, match="dpmpp"):
        gd.step_sizes(10, "dpmpp")
    with pytest.raises(ValueError, match="engine"):
        gd(np.zeros((2, 1, T, D), np.float32))


# ---- the agent on a stub engine ---------------------------------------------------------------------------------------------------------------
class GuideStub(TrainStub):
    """Records the guided calls: x[b] carries the observation's first embedding value, the global row and the first step size."""
    image_size = 64

    def agent_sample_guided(self, obs_emb, obs_horizon, guide, rho, *, seed=0, row_offset=0, sampler="ddim", planner_steps=None,
                            idm_steps=None, **kw):
        self.calls.append(("agent_sample_guided", obs_emb.shape[0], row_offset, seed, sampler, planner_steps, idm_steps, guide,
                           np.array(rho), sorted(k for k, v in kw.items() if v is not None)))
        self.call_seq += 1
        B = obs_emb.shape[0]
        x = obs_emb[:, 0, 0].reshape(B, 1, 1) + torch.zeros(B, T, D)
        x[:, :, 1] = (row_offset + torch.arange(B, dtype=torch.float32)).reshape(B, 1)
        x[:, :, 2] = float(rho[0])
        return x, x[:, :AH + 1].clone(), x[:, :AH, :A].clone()

    def plan_guide_cost(self, x, guide, n_per=1):
        self.calls.append(("plan_guide_cost", x.shape[0], n_per, guide))
        return x.reshape(x.shape[0], -1)[:, 1] + 100.0

    def mean_sq_diff(self, a, b):
        return ((a - b) ** 2).mean()


@pytest.fixture
def agent(monkeypatch):
    monkeypatch.setattr(W, "check_params", lambda tree, shapes: None)          # the stub's trees hold one leaf
    cfg = dict(lowdim_obs=DATA["lowdim_obs"], rgb_obs=DATA["rgb_obs"], obs_horizon=1, pred_horizon=T, action_horizon=AH, obs_dim=D,
               action_dim=A, vae_feature_dim=16, planner_n_diffusion_steps=100, idm_n_diffusion_steps=100, name="ldp_agent")
    st = lambda: ParamState({"w": np.zeros(1, np.float32)})                    # noqa: E731
    return LDPAgent(st(), st(), None, DATA["obs_normalization"], True, True, 1, 1, cfg, GuideStub(), W.PlannerSpec(D, D), W.IDMSpec(D, A),
                    W.VAESpec(), torch.device("cpu"))


def test_sample_guided_on_the_stub_engine(agent):
    eng = agent._engine
    b = cfgs.synth_latent_batch(DATA, 2, 1, 5)
    emb = agent.get_obs_cond(agent._postprocess(b)["obs"])
    goal = torch.full((2, D), 0.25)
    action, m = agent.sample_guided(b, 3, goal=goal, smooth=0.25, anchor=True, scale=0.1, schedule="constant", n_steps=10, row_offset=6)
    call, cost = [c for c in eng.calls if c[0] in ("agent_sample_guided", "plan_guide_cost")]
    assert call[:7] == ("agent_sample_guided", 2, 6, 3, "ddim", 10, 10) and call[9] == ["action_bounds", "action_mode"]
    gd = call[7]
    assert isinstance(gd, GD.Guide) and gd.engine is eng and np.all(gd.lam == 0.25) and torch.equal(gd.target[:, AH - 1], goal)
    assert torch.equal(gd.anchor, emb[:, 0])                                   # anchor=True: the batch's own last observation embedding
    assert np.array_equal(call[8], np.full(10, 0.1, np.float32))
    assert cost[:3] == ("plan_guide_cost", 2, 1) and cost[3] is gd
    assert set(m) == {"plan", "x", "guide_cost", "plan_viz"}
    x = np.array(m["x"])
    assert x.shape == (2, T, D) and x[:, 0, 1].tolist() == [6.0, 7.0] and np.array_equal(np.array(m["guide_cost"]), x[:, 0, 1] + 100.0)
    assert action.shape == (2, AH, A) and m["plan"].shape == (2, AH + 1, D)
    # a prebuilt guide: its own step sizes for this call's step count; anchor=True resolved on a copy
    del eng.calls[:]
    mine = agent.build_guide(2, goal=goal, anchor=True, scale=0.5, schedule="sigma2")
    agent.sample_guided(b, 3, guide=mine, sampler="ddpm")
    call = [c for c in eng.calls if c[0] == "agent_sample_guided"][0]
    assert call[4:7] == ("ddpm", None, None) and np.array_equal(call[8], mine.step_sizes(100, "ddpm")) and len(call[8]) == 100
    assert mine.anchor is True and call[7] is not mine and torch.equal(call[7].anchor, emb[:, 0]) and call[7].target is mine.target
    # a training batch also reports plan_mse; explicit noise passes through
    del eng.calls[:]
    _, m = agent.sample_guided(cfgs.synth_latent_batch(DATA, 2, T + 1, 5), 3, smooth=0.1, n_steps=10, noise=dict(x_init=torch.zeros(2, T, D)))
    assert set(m) == {"plan", "x", "guide_cost", "plan_viz", "plan_mse"}
    assert [c for c in eng.calls if c[0] == "agent_sample_guided"][0][9] == ["action_bounds", "action_mode", "x_init"]


def test_sample_guided_refusals(agent):
    b = cfgs.synth_latent_batch(DATA, 2, 1, 5)
    eng = agent._engine
    with pytest.raises(NotImplementedError, match="dpmpp"):
        agent.sample_guided(b, 0, smooth=0.1, sampler="dpmpp", n_steps=10)
    mine = agent.build_guide(2, smooth=0.25)
    with pytest.raises(ValueError, match="smooth"):
        agent.sample_guided(b, 0, guide=mine, smooth=0.1)
    with pytest.raises(ValueError, match="Guide"):
        agent.sample_guided(b, 0, guide=dict(lam=1))
    with pytest.raises(ValueError, match="> 1"):
        agent.sample_guided(b, 0, guide=agent.build_guide(2, smooth=0.25, scale=1.5), n_steps=10)
    with pytest.raises(ValueError, match="B = 3"):
        agent.sample_guided(b, 0, guide=agent.build_guide(3, smooth=0.25), n_steps=10)
    with pytest.raises(ValueError, match="> 1"):
        agent.sample_guided(b, 0, smooth=0.25, scale=1.5, n_steps=10)
    with pytest.raises(ValueError, match="lo"):
        agent.sample_guided(b, 0, lo=0.5, hi=0.0, n_steps=10)
    assert not [c for c in eng.calls if c[0] == "agent_sample_guided"]         # nothing reached the engine
    half = LDPAgent.sample_guided
    with pytest.raises(NotImplementedError, match="planner and the IDM"):
        half(type("P", (), dict(use_planner=True, use_idm=False))(), b, 0)


def test_other_agents_name_ldp_agent():
    from latent_diffusion_planning_amd.dp_agent import DPAgent
    from latent_diffusion_planning_amd.dp_train_agent import DPTrainAgent
    from latent_diffusion_planning_amd.dp_vae_agent import DPVAEAgent
    from latent_diffusion_planning_amd.hier_agent import LDPHierAgent
    for cls in (LDPHierAgent, DPVAEAgent, DPAgent, DPTrainAgent):
        for name in ("sample_guided", "build_guide"):
            with pytest.raises(NotImplementedError, match="LDPAgent"):
                getattr(cls, name)(object())


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_guided_entry_points():
    syms = _lib.header_symbols()
    for name in ("ldp_plan_guide_step", "ldp_plan_guide_cost", "ldp_plan_sample_guided", "ldp_agent_sample_guided"):
        assert name in syms and name in _lib.SIGNATURES
    assert GD.SCHEDULES == ("sigma2", "constant")
    assert schedule.COEF_STRIDE == 8 and len(GO.step_coefs(0, 100, 10, "ddim")) == 7
    # the oracle's coefficient rows are schedule.step_coefficients' (the rows the engine's make_step_coefs mirrors)
    for sampler, sid, n in (("ddim", schedule.SAMPLER_DDIM, 10), ("ddpm", schedule.SAMPLER_DDPM, 100)):
        tab = schedule.step_coefficients(schedule.make_schedule(100), n, sid)
        for i in (0, n // 2, n - 1):
            assert np.array_equal(np.array(GO.step_coefs(i, 100, n, sampler, cast32=True), np.float32), tab[i, :7])
