"""Guided planning on the GPU (csrc/guide.hip, the guided loop of csrc/engine.hip, LDPAgent.sample_guided) -- DESIGN.md 4.19.
Kernel shapes: D = 25 (rm_lift / rm_square: D % 4 != 0, the group 24..27 straddles D) at T = 8 and T = 16 (a 16 x 7 group sample: one
pass of the 256 threads) and D = 30 (aloha); cfgs.py has no D % 4 == 0 configuration, so D = 28 stands in for the all-vector
instantiation, and D = 70 at T = 16 (288 channel groups per sample: more than the 256 threads, the kernel's loop).  B = 1 / 3 / 17: one work-group, a few, more samples than one 16-row bucket.  The loops run rm_lift (T = 8, D = 25 padded
to 32): DDIM-10 on the 100-step schedule, DDPM on a 12-step schedule (every training timestep, as DDPM must)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from latent_diffusion_planning_amd import guide as GD
from latent_diffusion_planning_amd._lib import LDPHipError
from latent_diffusion_planning_amd.engine import HipEngine, philox_normal
from oracle import np64
from tests import cfgs, guide_oracle as GO, replan_oracle as RO
from tests.util import assert_close, idm_params, make_agent, planner_params, rng

pytestmark = pytest.mark.gpu

D, A, T, AH, DP, LAT = 25, 7, 8, 4, 32, 16
N = 10                                                                         # DDIM-10
N12 = 12                                                                       # the DDPM engine's training steps
B_SPLIT = 1040
CFG = dict(pred_horizon=T, obs_dim=D, action_horizon=AH, vae_feature_dim=LAT, rgb_obs=["latent_agentview_image"], planner_n_diffusion_steps=100)


@pytest.fixture(scope="module")
def eng():
    e = HipEngine(obs_dim=D, action_dim=A, global_cond_dim=D, pred_horizon=T, action_horizon=AH)
    e.load_params(planner=planner_params(D=D), idm=idm_params(D=D, A=A))
    yield e
    e.check_fault()
    e.close()


@pytest.fixture(scope="module")
def eng12():
    e = HipEngine(obs_dim=D, action_dim=A, global_cond_dim=D, pred_horizon=T, action_horizon=AH, planner_train_steps=N12)
    e.load_params(planner=planner_params(D=D))
    yield e
    e.check_fault()
    e.close()


_bare = {}


def _kernel_engine(Dk, Tk):
    """A handle without weights: the two stand-alone kernels need the shapes only."""
    if (Dk, Tk) not in _bare:
        _bare[(Dk, Tk)] = HipEngine(obs_dim=Dk, action_dim=A, global_cond_dim=Dk, pred_horizon=Tk, action_horizon=AH)
    return _bare[(Dk, Tk)]


def _dev(a, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _bits(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t, np.float32)).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _cond(B, seed=1):
    return _dev(rng(seed).uniform(-1, 1, (B, D)))


def _guide(g, B, Dk=D, Tk=T, anchor=True, box=0.6):
    """Every term switched on: goal weights on about half the entries, a box narrower than [-1, 1] (the hinge is active on some entries and
    idle on others).  -> (the oracle's dict, the same guide for the engine)."""
    G = GO.make(B, Tk, Dk, target=g.uniform(-1, 1, (B, Tk, Dk)), wg=g.uniform(0, 2, (B, Tk, Dk)) * (g.uniform(size=(B, Tk, Dk)) < 0.5),
                anchor=g.uniform(-1, 1, (B, Dk)) if anchor else None, lam=g.uniform(0, 0.5, Dk), beta=g.uniform(0, 3, Dk),
                lo=-box * g.uniform(0.5, 1, Dk), hi=box * g.uniform(0.5, 1, Dk))
    return G, _ns(G)


def _ns(G):
    return SimpleNamespace(target=G["target"], weight=G["wg"], anchor=G["anchor"], lam=G["lam"], beta=G["beta"], lo=G["lo"], hi=G["hi"])


def _rows(G, sl):
    return {k: (v[sl] if k in ("target", "wg") or (k == "anchor" and v is not None) else v) for k, v in G.items()}


# ---- 1. the guided step alone -----------------------------------------------------------------------------------------------------------------
STEP_ROWS = [("ddim", 10, 0), ("ddim", 10, 9), ("ddpm", 100, 3), ("ddpm", 100, 99)]      # first / last DDIM row; a DDPM row with sigma > 0; the last


@pytest.mark.parametrize("B", [1, 3, 17])
@pytest.mark.parametrize("Dk,Tk", [(25, 8), (30, 8), (25, 16), (28, 8), (70, 16)])
def test_guide_step_kernel(Dk, Tk, B):
    """Every element against float64 (the float32 coefficient rows the computation is defined with) within guide_oracle.step_bound, the
    bound its spelled roundings imply, and bit for bit against guide_oracle.emulate_step.  No element is excluded: every function involved
    is continuous.  The padded call (x with row stride 32 / 64-byte aligned rows, the guide with the same stride: the instantiation the
    loop runs) gives the same bits and leaves the padding columns alone.  Measured on one MI355X: max |err| / bound = 0.93."""
    e = _kernel_engine(Dk, Tk)
    DPk = (Dk + 31) // 32 * 32
    seed, off = 1234, 6
    g = rng(100 * Dk + 10 * Tk + B)
    y0 = g.standard_normal((B, Tk, Dk)) * 0.7                                  # the data prediction: beyond [-1, 1] on some entries, inside on most
    eps = g.standard_normal((B, Tk, Dk)).astype(np.float32)
    nz = g.standard_normal((B, Tk, Dk)).astype(np.float32)
    worst = 0.0
    for anchor in (False, True):
        G, ns = _guide(g, B, Dk, Tk, anchor)
        rho32 = np.float32(1.0 / GO.lipschitz(G))
        for sampler, n, i in STEP_ROWS:
            k = GO.step_coefs(i, 100, n, sampler, cast32=True)
            x = (y0 / k[1] + k[2] * eps).astype(np.float32)                    # the state at this row's noise level whose data prediction is y0
            raw = (x.astype(np.float64) - k[2] * eps) * k[1]
            y = np.clip(raw, -1, 1)
            assert (np.abs(raw) > 1).any() and (np.abs(raw) < 1).any()
            assert ((y > G["hi"]) | (y < G["lo"])).any() and ((y < G["hi"]) & (y > G["lo"])).any()
            rho = np.zeros(n, np.float32)
            rho[i] = rho32                                                     # (the kernel reads entry `step` of the table)
            kw = dict(seed=seed, row_offset=off, sampler=sampler, n_steps=n)
            noises = [None] if k[6] == 0.0 else [nz, None]                     # sigma > 0: explicit noise, and the Philox draw
            for noise in noises:
                got = e.plan_guide_step(_dev(x), _dev(eps), ns, rho, i, noise=None if noise is None else _dev(noise), **kw)
                z = noise
                if noise is None and k[6] != 0.0:                              # the fused step's draw: stream 0, step i, element (row0 + r) * DP + c
                    z = philox_normal(seed, off * Tk * DPk, i, 0, B * Tk * DPk).reshape(B, Tk, DPk)[:, :, :Dk].cpu().numpy()
                ref = GO.guided_step(x, eps, G, float(rho32), k, z)
                bound = GO.step_bound(x, eps, G, float(rho32), k, z)
                g64 = got.cpu().numpy().astype(np.float64)
                ratio = float((np.abs(g64 - ref) / bound).max())
                worst = max(worst, ratio)
                assert np.isfinite(g64).all() and ratio <= 1.0, (sampler, i, anchor, ratio)
                emu = GO.emulate_step(x, eps, G, rho32, k, z)
                assert _same(got, emu), (sampler, i, anchor, int((_bits(got) != _bits(emu)).sum()))
                # padded strides, in place: the same bits, and the padding columns keep theirs
                xp = torch.full((B, Tk, DPk), 7.25, device="cuda")
                xp[:, :, :Dk] = _dev(x)
                out = e.plan_guide_step(xp, _dev(eps), ns, rho, i, noise=None if noise is None else _dev(noise), ldg=DPk, inplace=True, **kw)
                assert out is xp and _same(xp[:, :, :Dk].contiguous(), got) and bool((xp[:, :, Dk:] == 7.25).all())
    print(f"guide step D = {Dk} T = {Tk} B = {B}: max |err| / bound = {worst:.3f}")
    # the draw depends on the global row only: rows 1.. of a call at `off` are the rows of a call at off + 1
    if B > 1:
        G, ns = _guide(g, B, Dk, Tk, True)
        rho = np.full(100, 0.05, np.float32)
        kw = dict(seed=seed, sampler="ddpm", n_steps=100)
        x = (y0 * 1.5).astype(np.float32)
        whole = e.plan_guide_step(_dev(x), _dev(eps), ns, rho, 3, row_offset=off, **kw)
        part = e.plan_guide_step(_dev(x[1:]), _dev(eps[1:]), _ns(_rows(G, slice(1, None))), rho, 3, row_offset=off + 1, **kw)
        assert _same(whole[1:], part)


# ---- 2. the cost ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Dk,Tk", [(25, 8), (30, 8), (25, 16)])
def test_guide_cost_kernel(Dk, Tk):
    """J against float64 within guide_oracle.cost_bound (the summation bound of its fixed order), bitwise equal across two calls and across
    batches (B = 17 against the first 17 rows of B = 20), with several candidates per observation costed under their observation's guide row."""
    e = _kernel_engine(Dk, Tk)
    g = rng(7 * Dk + Tk)
    worst = 0.0
    for anchor in (False, True):
        G, ns = _guide(g, 20, Dk, Tk, anchor)
        y = (g.standard_normal((20, Tk, Dk)) * 0.8).astype(np.float32)
        j20 = e.plan_guide_cost(_dev(y), ns)
        assert _same(j20, e.plan_guide_cost(_dev(y), ns))
        for B in (1, 3, 17):
            jb = e.plan_guide_cost(_dev(y[:B]), _ns(_rows(G, slice(0, B))))
            assert tuple(jb.shape) == (B,) and _same(jb, j20[:B])
        ref, bound = GO.cost(y, G), GO.cost_bound(y, G)
        ratio = float((np.abs(j20.cpu().numpy().astype(np.float64) - ref) / bound).max())
        worst = max(worst, ratio)
        assert (ref > 0.1).all() and ratio <= 1.0, ratio
        # three candidates per observation: row r is costed under guide row r // 3
        G6 = _rows(G, slice(0, 6))
        y18 = (g.standard_normal((18, Tk, Dk)) * 0.8).astype(np.float32)
        j18 = e.plan_guide_cost(_dev(y18), _ns(G6), n_per=3)
        rep = {k: (np.repeat(v, 3, axis=0) if k in ("target", "wg") or (k == "anchor" and v is not None) else v) for k, v in G6.items()}
        assert _same(j18, e.plan_guide_cost(_dev(y18), _ns(rep)))
        assert (np.abs(j18.cpu().numpy() - GO.cost(y18, rep)) <= GO.cost_bound(y18, rep)).all()
    print(f"guide cost D = {Dk} T = {Tk}: max |err| / bound = {worst:.3f}")


# ---- 3. the loop -----------------------------------------------------------------------------------------------------------------------------------
def _by_hand(e, cond, x, ns, rho, sampler, n, n_train, begin=0, end=None, **kw):
    for i in range(begin, n if end is None else end):
        t = RO.step_timestep(i, n_train, n, sampler)
        x = e.plan_guide_step(x, e.unet_forward(x, t, cond), ns, rho, i, sampler=sampler, n_steps=n, **kw)
    return x


@pytest.mark.parametrize("B", [3, 17])
@pytest.mark.parametrize("sampler", ["ddim", "ddpm"])
def test_loop_composition_graph_ranges_and_batches(eng, eng12, sampler, B):
    """Eager = the hand composition unet_forward + plan_guide_step; graph (capture, replay) = eager; [0, 4) then [4, n) = [0, n); rows of
    B = 17 = the same rows of B = 20.  All bit for bit.  DDPM draws its step noise from Philox here, in the kernel and by hand alike."""
    e, n, n_train = (eng, N, 100) if sampler == "ddim" else (eng12, N12, N12)
    g = rng(300 + B)
    G20, _ = _guide(g, 20)
    G, ns = _rows(G20, slice(0, B)), _ns(_rows(G20, slice(0, B)))
    rho = (np.linspace(1.0, 0.2, n) / GO.lipschitz(G20)).astype(np.float32)
    cond20 = _cond(20)
    cond = cond20[:B].contiguous()
    kw = dict(seed=99, row_offset=11, sampler=sampler, n_steps=n)
    eager = e.plan_sample_guided(cond, ns, rho, use_graph=False, **kw)
    x_t = e.plan_sample_range(cond, 0, 0, **kw)                                # the drawn initial state
    hand = _by_hand(e, cond, x_t, ns, rho, sampler, n, n_train, seed=99, row_offset=11)
    assert torch.isfinite(eager).all() and _same(eager, hand), f"max |diff| = {float((eager - hand).abs().max()):.3e}"
    first = e.plan_sample_guided(cond, ns, rho, use_graph=True, **kw)
    replay = e.plan_sample_guided(cond, ns, rho, use_graph=True, **kw)
    assert _same(first, eager) and _same(replay, eager)
    for use_graph in (False, True):
        head = e.plan_sample_guided(cond, ns, rho, step_begin=0, step_end=4, use_graph=use_graph, **kw)
        tail = e.plan_sample_guided(cond, ns, rho, step_begin=4, step_end=n, x_init=head, use_graph=use_graph, **kw)
        assert not _same(head, eager) and _same(tail, eager)
    assert _same(e.plan_sample_guided(cond, ns, rho, step_begin=3, step_end=3, x_init=x_t, **kw), x_t)      # an empty range: the state itself
    if B == 17:
        big = e.plan_sample_guided(cond20, _ns(G20), rho, **kw)
        assert _same(big[:17], eager)
    # a graph bakes no value of the guide: another guide and other step sizes through the same captured graph
    G2, ns2 = _guide(rng(301 + B), B, anchor=True)
    rho2 = (rho * 0.5).astype(np.float32)
    assert _same(e.plan_sample_guided(cond, ns2, rho2, use_graph=True, **kw), e.plan_sample_guided(cond, ns2, rho2, use_graph=False, **kw))
    assert not _same(e.plan_sample_guided(cond, ns2, rho2, use_graph=True, **kw), eager)


@pytest.mark.parametrize("sampler,B,anchor", [("ddim", 3, True), ("ddim", 17, False), ("ddpm", 3, True)])
def test_loop_against_float64(eng, eng12, sampler, B, anchor):
    """The project's 1e-4 against tests/guide_oracle.py on np64's U-Net, explicit step noise for DDPM; an all-zero guide is within 1e-4 of
    the float64 FREE loop (with rho = 0 the guided loop is the free loop up to rounding)."""
    e, n, n_train = (eng, N, 100) if sampler == "ddim" else (eng12, N12, N12)
    g = rng(500 + B + n)
    G, ns = _guide(g, B, anchor=anchor)
    rho = (np.linspace(1.0, 0.2, n) / GO.lipschitz(G)).astype(np.float32)
    cond = g.uniform(-1, 1, (B, D)).astype(np.float32)
    x_init = g.standard_normal((B, T, D)).astype(np.float32)
    nz = g.standard_normal((n, B, T, D)).astype(np.float32) if sampler == "ddpm" else None
    P = np64.to64(planner_params(D=D))
    okw = dict(step_noise=nz, n_train=n_train, n_steps=n, sampler=sampler)
    kw = dict(x_init=_dev(x_init), step_noise=None if nz is None else _dev(nz), sampler=sampler, n_steps=n)
    got = e.plan_sample_guided(_dev(cond), ns, rho, **kw)
    ref = GO.planner_range_guided(P, cond.astype(np.float64), x_init, 0, n, G, rho.astype(np.float64), **okw)
    assert_close(got.cpu().numpy(), ref, 1e-4, f"guided {sampler}-{n} B = {B}")
    free64 = RO.planner_range(P, cond.astype(np.float64), x_init, 0, n, **okw)
    moved = float(np.median(np.abs(ref - free64)))
    print(f"guided {sampler}-{n} B = {B}: median |guided - free| = {moved:.3f}")
    assert moved > 1e-2                                                        # not a no-op
    zero = e.plan_sample_guided(_dev(cond), _ns(GO.make(B, T, D)), np.zeros(n, np.float32), **kw)
    assert_close(zero.cpu().numpy(), free64, 1e-4, f"zero guide {sampler}-{n} B = {B} against the free loop")
    still = e.plan_sample_guided(_dev(cond), ns, np.zeros(n, np.float32), **kw)          # rho = 0 with weights: the free loop too
    assert_close(still.cpu().numpy(), free64, 1e-4, f"rho = 0 {sampler}-{n} B = {B} against the free loop")


def test_free_calls_keep_their_bits_graphs_and_launches(eng):
    """The graph-key check: a free plan_sample / agent_sample has the bits and the launch counts it had before any guided call, and after
    one -- and the guided loop has exactly one launch more per step."""
    B = 3
    cond = _cond(B)
    obs_emb = cond[:, None].contiguous()
    kw = dict(seed=5, row_offset=2, sampler="ddim", n_steps=N)
    _, ns = _guide(rng(41), B)
    rho = np.full(N, 0.05, np.float32)
    before, counts = [], []
    for rnd in range(2):
        for use_graph in (False, True, True):
            free = eng.plan_sample(cond, use_graph=use_graph, **kw)
            c_free = eng.launch_counts()
            x, plan, act = eng.agent_sample(obs_emb, 1, seed=5, row_offset=2, sampler="ddim", planner_steps=N, idm_steps=N, use_graph=use_graph)
            c_joint = eng.launch_counts()
            before.append((free, x, act))
            counts.append((c_free, c_joint))
        if rnd == 0:
            for use_graph in (False, True, True):
                eng.plan_sample_guided(cond, ns, rho, use_graph=use_graph, **kw)
                c_g = eng.launch_counts()
                assert c_g[0] == counts[0][0][0] and c_g[1] == counts[0][0][1] + N, (c_g, counts[0][0])
                eng.agent_sample_guided(obs_emb, 1, ns, rho, seed=5, row_offset=2, sampler="ddim", planner_steps=N, idm_steps=N, use_graph=use_graph)
                c_g = eng.launch_counts()
                assert c_g[0] == counts[0][1][0] and c_g[1] == counts[0][1][1] + N, (c_g, counts[0][1])
    for (free, x, act), c in zip(before, counts):
        assert _same(free, before[0][0]) and _same(x, before[0][1]) and _same(act, before[0][2]) and c == counts[0]
    assert _same(before[0][0], before[0][1])                                   # (the joint call's planner state is plan_sample's)


def test_split_batch(eng):
    """B = 1040 runs as two loops (1024 + 16 rows): each part gets its rows of the guide and its own row_offset."""
    B, b1, off = B_SPLIT, 1024, 7
    g = rng(1000)
    cond = _dev(g.uniform(-1, 1, (B, D)))
    G, ns = _guide(g, B)
    rho = np.full(N, 0.5 / GO.lipschitz(G), np.float32)
    kw = dict(seed=21, sampler="ddim", n_steps=N)
    whole = eng.plan_sample_guided(cond, ns, rho, row_offset=off, **kw)
    c_whole = eng.launch_counts()
    first = eng.plan_sample_guided(cond[:b1].contiguous(), _ns(_rows(G, slice(0, b1))), rho, row_offset=off, **kw)
    c1 = eng.launch_counts()
    second = eng.plan_sample_guided(cond[b1:].contiguous(), _ns(_rows(G, slice(b1, None))), rho, row_offset=off + b1, **kw)
    c2 = eng.launch_counts()
    assert torch.isfinite(whole).all() and _same(whole[:b1], first) and _same(whole[b1:], second)
    assert c_whole == (c1[0] + c2[0], c1[1] + c2[1])
    x, plan, act = eng.agent_sample_guided(cond[:, None].contiguous(), 1, ns, rho, seed=21, row_offset=off, sampler="ddim", planner_steps=N,
                                           idm_steps=N)
    assert _same(x, whole) and _same(plan[:, 1:], x[:, :AH]) and torch.isfinite(act).all()
    eng.check_fault()


# ---- 4. properties ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 17])
def test_unit_weight_at_unit_step_lands_on_the_target(eng, B):
    """wg = 1 on a mask, lam = beta = 0, constant rho = 1: the last step computes y' = clip(rn(fma(-1, rn(y - target), y))) and x' = 1 * y'
    (DDIM's last row: c_x0 = 1, c_eps = 0), two roundings at |values| <= 1 -- within 2^-22 of the target."""
    g = rng(600 + B)
    target = g.uniform(-1, 1, (B, T, D)).astype(np.float32)
    mask = np.zeros((B, T, D), bool)
    mask[:, 3] = True
    mask[B - 1, 7, LAT:LAT + 3] = True
    gd = GD.build_guide(CFG, B, target=target, weight=mask.astype(np.float32), scale=1.0, schedule="constant")
    rho = gd.step_sizes(N, "ddim")
    assert gd.lipschitz == 1.0 and np.all(rho == 1.0)
    got = eng.plan_sample_guided(_cond(B), gd, rho, seed=3, sampler="ddim", n_steps=N).cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - target)[mask].max())
    print(f"unit weight, unit step B = {B}: max |x - target| on the mask = {err:.3e} (2^-22 = {2.0 ** -22:.3e})")
    assert err <= 2.0 ** -22
    free = eng.plan_sample(_cond(B), seed=3, sampler="ddim", n_steps=N).cpu().numpy()
    assert np.abs(free - target)[mask].max() > 0.1                             # (the free plan is nowhere near it)


@pytest.mark.parametrize("sampler", ["ddim", "ddpm"])
def test_goal_guide_lowers_its_cost_per_sample(eng, eng12, sampler):
    e, n = (eng, N) if sampler == "ddim" else (eng12, N12)
    B = 17
    g = rng(700)
    goal = g.uniform(-1, 1, (B, D)).astype(np.float32)
    gd = GD.build_guide(dict(CFG, planner_n_diffusion_steps=100 if sampler == "ddim" else N12), B, goal=goal, scale=0.5, schedule="constant", engine=e)
    rho = gd.step_sizes(n, sampler)
    kw = dict(seed=8, row_offset=1, sampler=sampler, n_steps=n)
    guided = e.plan_sample_guided(_cond(B), gd, rho, **kw)
    free = e.plan_sample(_cond(B), **kw)
    jg, jf = e.plan_guide_cost(guided, gd).cpu().numpy(), e.plan_guide_cost(free, gd).cpu().numpy()
    print(f"goal guide {sampler}: J guided / J free, per sample: min {float((jg / jf).min()):.3f} max {float((jg / jf).max()):.3f}")
    assert (jg <= jf).all()


# ---- 5. the agent ------------------------------------------------------------------------------------------------------------------------------------
def test_agent_sample_guided():
    from latent_diffusion_planning_amd.agent import _seed_of
    ag, data = make_agent("rm", planner_params(), idm_params())
    try:
        e = ag._engine
        B = 3
        batch = cfgs.synth_latent_batch(data, B, 1, 2)
        goal_obs = cfgs.synth_latent_batch(data, B, 1, 5)["obs"]
        goal = ag._goal_embedding(goal_obs, B)
        obs_emb = ag.get_obs_cond(ag._vae_encode_t(ag._postprocess(batch)["obs"])).contiguous()
        kw = dict(sampler="ddim", n_steps=N)
        gkw = dict(goal_weight=1.0, smooth=0.1, anchor=True, bound_weight=0.5, lo=-0.8, hi=0.8, schedule="sigma2")
        for gl in (goal, goal_obs):                                            # an embedding, an observation dict
            action, m = ag.sample_guided(batch, 8, goal=gl, row_offset=4, **gkw, **kw)
            assert sorted(m) == ["guide_cost", "plan", "plan_viz", "x"]
            x, plan = m["x"].tensor, m["plan"].tensor
            assert tuple(x.shape) == (B, T, D) and tuple(plan.shape) == (B, AH + 1, D) and tuple(action.shape) == (B, AH, A)
            # the engine calls by hand
            gd = GD.build_guide(ag.config, B, goal=goal, **dict(gkw, anchor=obs_emb[:, 0].contiguous()), engine=e)
            rho = gd.step_sizes(N, "ddim")
            lo, hi, amode = ag._action_bounds()
            x2, plan2, act2 = e.agent_sample_guided(obs_emb, 1, gd, rho, seed=_seed_of(8), row_offset=4, planner_steps=N, idm_steps=N, action_bounds=(lo, hi),
                                                    action_mode=amode, sampler="ddim")
            assert _same(x, x2) and _same(plan, plan2) and _same(action.tensor, act2)
            assert _same(x, e.plan_sample_guided(obs_emb[:, 0].contiguous(), gd, rho, seed=_seed_of(8), row_offset=4, **kw))
            assert _same(plan[:, 1:], x[:, :AH]) and _same(plan[:, 0], obs_emb[:, 0])
            # guide_cost is Guide.__call__ on metrics['x']
            assert _same(m["guide_cost"].tensor, gd(x[:, None].contiguous())[:, 0])
            assert np.isfinite(np.array(action)).all() and torch.isfinite(x).all()
        # a prebuilt guide gives the same call; the free call differs
        mine = ag.build_guide(B, goal=goal_obs, **gkw)
        a3, m3 = ag.sample_guided(batch, 8, guide=mine, row_offset=4, **kw)
        assert _same(m3["x"].tensor, x) and _same(a3.tensor, action.tensor) and mine.anchor is True
        free_a, free_m = ag.sample_warm(batch, 8, None, None, row_offset=4, **kw)
        assert not _same(free_m["x"].tensor, x)
        # the guide as the score of sample_best_of: costs are the guide's costs of the candidates, the winner has the lowest
        score = ag.build_guide(B, goal=goal, smooth=0.1)
        _, mb = ag.sample_best_of(batch, 8, 4, score=score, **kw)
        cand, costs = mb["candidates"].tensor, mb["costs"].tensor
        assert tuple(costs.shape) == (B, 4) and _same(costs, score(cand))
        assert np.array_equal(np.array(mb["best_index"]), costs.argmin(dim=1).cpu().numpy())
        # a training batch (frames beyond obs_horizon) also reports plan_mse
        _, m = ag.sample_guided(cfgs.synth_latent_batch(data, B, T + 1, 2), 8, goal=goal, **kw)
        assert sorted(m) == ["guide_cost", "plan", "plan_mse", "plan_viz", "x"] and np.isfinite(float(np.array(m["plan_mse"])))
        # argument errors leave the engine usable
        with pytest.raises(ValueError, match="> 1"):
            ag.sample_guided(batch, 8, goal=goal, scale=1.5, **kw)
        with pytest.raises(ValueError, match="t_goal"):
            ag.sample_guided(batch, 8, goal=goal, t_goal=T, **kw)
        with pytest.raises(ValueError, match="goal"):
            ag.sample_guided(batch, 8, goal=goal[:2], **kw)
        with pytest.raises(NotImplementedError, match="dpmpp"):
            ag.sample_guided(batch, 8, goal=goal, sampler="dpmpp", n_steps=N)
        a4, m4 = ag.sample_guided(batch, 8, guide=mine, row_offset=4, **kw)
        assert _same(m4["x"].tensor, x)
        e.check_fault()
    finally:
        ag._engine.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(eng):
    B = 3
    cond = _cond(B)
    G, ns = _guide(rng(5), B)
    rho = np.full(N, 0.05, np.float32)
    x = _dev(rng(6).standard_normal((B, T, D)))
    kw = dict(sampler="ddim", n_steps=N)

    def bad(**ch):
        return SimpleNamespace(**dict(vars(ns), **ch))
    for g2, word in ((bad(lam=-G["lam"] - 1), "lam"), (bad(beta=-G["beta"] - 1), "beta"), (bad(lo=G["hi"] + 1), "lo"),
                     (bad(lam=np.full(D, np.nan, np.float32)), "lam")):
        with pytest.raises(LDPHipError, match=word):
            eng.plan_sample_guided(cond, g2, rho, **kw)
        with pytest.raises(LDPHipError, match=word):
            eng.agent_sample_guided(cond[:, None].contiguous(), 1, g2, rho, planner_steps=N, idm_steps=N, sampler="ddim")
    for r2 in (rho[:5], np.concatenate([rho, rho]), -rho):
        with pytest.raises(LDPHipError, match="rho"):
            eng.plan_sample_guided(cond, ns, r2, **kw)
    with pytest.raises(LDPHipError, match="sampler 2"):
        eng.plan_sample_guided(cond, ns, rho, sampler="dpmpp", n_steps=N)
    with pytest.raises(LDPHipError, match="sampler 2"):
        eng.plan_guide_step(x, x, ns, rho, 0, sampler="dpmpp", n_steps=N)
    with pytest.raises(LDPHipError, match="step"):
        eng.plan_guide_step(x, x, ns, rho, N, **kw)
    for begin, end, word in ((-1, 3, "step_begin"), (4, 3, "step_end"), (0, N + 1, "step_end")):
        with pytest.raises(LDPHipError, match=word):
            eng.plan_sample_guided(cond, ns, rho, step_begin=begin, step_end=end, **kw)
    with pytest.raises(ValueError, match="target"):
        eng.plan_sample_guided(cond, bad(target=G["target"][:, :, :24]), rho, **kw)
    with pytest.raises(ValueError, match="anchor"):
        eng.plan_sample_guided(cond, bad(anchor=G["anchor"][:2]), rho, **kw)
    with pytest.raises(ValueError, match="anchor=True"):
        eng.plan_sample_guided(cond, bad(anchor=True), rho, **kw)
    with pytest.raises(ValueError, match="lam"):
        eng.plan_sample_guided(cond, bad(lam=G["lam"][:5]), rho, **kw)
    with pytest.raises(ValueError, match="rho"):
        eng.plan_guide_step(x, x, ns, rho[:5], 0, **kw)
    with pytest.raises(ValueError, match="n_per"):
        eng.plan_guide_cost(x, ns, n_per=2)
    # nothing above left the engine in a bad state
    assert torch.isfinite(eng.plan_sample_guided(cond, ns, rho, **kw)).all()
    eng.check_fault()
