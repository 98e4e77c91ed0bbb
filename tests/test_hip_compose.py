"""Composed planning on the GPU (csrc/compose.hip, the composed loop of csrc/engine.hip, LDPAgent.plan, Controller) -- DESIGN.md 4.20.
Kernel shapes as tests/test_hip_guide.py: D = 25 (odd, the group 24..27 straddles D) at T = 8 and T = 16, D = 30 (D % 4 = 2), D = 28 (fully
vectorised) and D = 70 at T = 16 (more channel groups per sample than the 256 threads); B = 1 / 3 / 17; padded and unpadded strides.  The
loops run rm_lift (T = 8, D = 25 padded to 32): DDIM-10 and DPM-Solver++-10 on the 100-step schedule, DDPM on a 12-step schedule."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from latent_diffusion_planning_amd import constrain as CN, guide as GD, schedule
from latent_diffusion_planning_amd._lib import LDPHipError, check
from latent_diffusion_planning_amd.engine import HipEngine, philox_normal
from latent_diffusion_planning_amd.replan import group_rows
from oracle import np64
from tests import cfgs, compose_oracle as XO, guide_oracle as GO, replan_oracle as RO
from tests.util import assert_close, idm_params, make_agent, planner_params, rng

pytestmark = pytest.mark.gpu

D, A, T, AH = 25, 7, 8, 4
N, N12 = 10, 12
TS = schedule.solver_timesteps(100, N, "logsnr")                              # the table "dpmpp" runs with n_steps = 10
ST_STEP, ST_INIT, ST_CONS = 0, 1, 12                                           # LDP_PHILOX_STREAM_*


@pytest.fixture(scope="module")
def eng():
    e = HipEngine(obs_dim=D, action_dim=A, global_cond_dim=D, pred_horizon=T, action_horizon=AH)
    e.load_params(planner=planner_params(D=D), idm=idm_params(D=D, A=A))
    e.set_solver_timesteps(TS)
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
    """A handle without weights: the stand-alone step needs the shapes (and the timestep table) only."""
    if (Dk, Tk) not in _bare:
        _bare[(Dk, Tk)] = HipEngine(obs_dim=Dk, action_dim=A, global_cond_dim=Dk, pred_horizon=Tk, action_horizon=AH)
        _bare[(Dk, Tk)].set_solver_timesteps(TS)
    return _bare[(Dk, Tk)]


def _dev(a, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _bits(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t, np.float32)).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _cond(B, seed=1):
    return _dev(rng(seed).uniform(-1, 1, (B, D)))


def _ns(G):
    return SimpleNamespace(target=G["target"], weight=G["wg"], anchor=G["anchor"], lam=G["lam"], beta=G["beta"], lo=G["lo"], hi=G["hi"])


def _guide(g, B, Dk=D, Tk=T, anchor=True, box=0.6):
    G = GO.make(B, Tk, Dk, target=g.uniform(-1, 1, (B, Tk, Dk)), wg=g.uniform(0, 2, (B, Tk, Dk)) * (g.uniform(size=(B, Tk, Dk)) < 0.5),
                anchor=g.uniform(-1, 1, (B, Dk)) if anchor else None, lam=g.uniform(0, 0.5, Dk), beta=g.uniform(0, 3, Dk),
                lo=-box * g.uniform(0.5, 1, Dk), hi=box * g.uniform(0.5, 1, Dk))
    return G, _ns(G)


def _rows(G, sl):
    return {k: (v[sl] if k in ("target", "wg") or (k == "anchor" and v is not None) else v) for k, v in G.items()}


def _constraint(g, B, Dk=D, Tk=T):
    """A whole goal state at one step, a partial waypoint, and scattered single entries."""
    target = g.uniform(-1, 1, (B, Tk, Dk)).astype(np.float32)
    mask = (g.uniform(size=(B, Tk, Dk)) < 0.1).astype(np.uint8)
    mask[:, 3] = 1
    mask[B - 1, Tk - 1, Dk - 3:] = 1
    return target, mask


def _draw(seed, off, B, Tk, Dk, step, stream):
    DPk = (Dk + 31) // 32 * 32
    return philox_normal(seed, off * Tk * DPk, step, stream, B * Tk * DPk).reshape(B, Tk, DPk)[:, :, :Dk].cpu().numpy()


# ---- 1. the composed step alone ---------------------------------------------------------------------------------------------------------
# (sampler, n_steps, step, second): a DDPM row with sigma > 0, the first and the last DDIM row (the step to level n), a first-order, a
# second-order and the last solver row
STEP_ROWS = [("ddpm", 100, 3, False), ("ddim", 10, 0, False), ("ddim", 10, 9, False), ("dpmpp", 10, 4, False), ("dpmpp", 10, 4, True),
             ("dpmpp", 10, 9, False)]


@pytest.mark.parametrize("B", [1, 3, 17])
@pytest.mark.parametrize("Dk,Tk", [(25, 8), (30, 8), (28, 8), (25, 16), (70, 16)])
def test_compose_step_kernel(eng, Dk, Tk, B):
    """Every combination of {ddpm with sigma > 0, ddim, dpmpp first and second order} x {guide off, on, on with anchor} x {no constraint,
    clamp, repaint}, the last step included: bit for bit against compose_oracle.emulate_step; against float64 (the float32 coefficient rows
    the computation is defined with) within compose_oracle.step_bound, max |err| / bound <= 1 with no element excluded (where the bound is
    0 -- a clamped entry -- the value is the target itself); bit for bit against the hand composition of the existing stand-alone calls
    (DDPM / DDIM: plan_guide_step, with a rho = 0 table for guide off, then plan_constrain -- which needs a finalized planner, so at
    D = 25, T = 8 only; dpmpp without a guide: plan_solver_step, then torch.where for clamp); the padded in-place call (row stride 32 / 96
    for the state, the history, the guide and the constraint) gives the same bits and leaves every padding column alone.
    Measured on one MI355X: max |err| / bound = 0.979 (D = 70, T = 16, B = 17; 0.85 - 0.98 over the fifteen cases)."""
    e = eng if (Dk, Tk) == (D, T) else _kernel_engine(Dk, Tk)
    DPk = (Dk + 31) // 32 * 32
    seed, off = 4321, 5
    g = rng(1000 * Dk + 10 * Tk + B)
    y0 = g.standard_normal((B, Tk, Dk)) * 0.7
    eps = g.standard_normal((B, Tk, Dk)).astype(np.float32)
    nz = g.standard_normal((B, Tk, Dk)).astype(np.float32)
    hist = g.uniform(-1, 1, (B, Tk, Dk)).astype(np.float32)
    target, mask = _constraint(g, B, Dk, Tk)
    worst = 0.0
    for sampler, n, i, second in STEP_ROWS:
        solver = sampler == "dpmpp"
        k = XO.step_row(sampler, i, 100, n, TS, cast32=True)
        x = (y0 / k["inv_a"] + k["s"] * eps).astype(np.float32)                # the state at this row's level whose data prediction is y0
        kw = dict(seed=seed, row_offset=off, sampler=sampler, n_steps=n)
        for gi, anchor in enumerate((None, False, True)):
            G = ns = None
            rho32, rho = np.float32(0.0), None
            if anchor is not None:
                G, ns = _guide(g, B, Dk, Tk, anchor)
                rho32 = np.float32(1.0 / GO.lipschitz(G))
                rho = np.zeros(n, np.float32)
                rho[i] = rho32
            for mode in (None, "clamp", "repaint"):
                # explicit step noise with the guide off, the Philox draw otherwise (DDPM); the repaint draw is always Philox
                noise = nz if (k["sigma"] != 0.0 and G is None) else None
                z = noise if noise is not None else (_draw(seed, off, B, Tk, Dk, i, ST_STEP) if k["sigma"] != 0.0 else None)
                cons = ckw = None
                if mode is not None:
                    zc = _draw(seed, off, B, Tk, Dk, i + 1, ST_CONS)
                    cons = XO.constraint(target, mask, mode, i + 1, sampler, 100, n, TS, zc, cast32=True)
                    ckw = dict(target=_dev(target), mask=_dev(mask, np.uint8), mode=mode)
                okw = dict(G=G, rho=float(rho32), z=z, h_prev=hist, second=second, cons=cons, solver=solver)
                ekw = dict(guide=ns, rho=rho, noise=None if noise is None else _dev(noise), x0_prev=_dev(hist) if second else None,
                           second=second, **(ckw or {}), **kw)
                got = e.plan_compose_step(_dev(x), _dev(eps), i, **ekw)
                got, got_h = got if solver else (got, None)
                emu, emu_h = XO.emulate_step(x, eps, k, **okw)
                what = (sampler, i, second, anchor, mode)
                assert _same(got, emu), (what, int((_bits(got) != _bits(emu)).sum()))
                ref, ref_h = XO.compose_step(x, eps, k, **okw)
                bx, bh = XO.step_bound(x, eps, k, **okw)
                err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
                assert np.isfinite(err).all() and (err[bx == 0.0] == 0.0).all(), what
                ratio = float((err[bx > 0.0] / bx[bx > 0.0]).max())
                if solver:
                    assert _same(got_h, emu_h), what
                    ratio = max(ratio, float((np.abs(got_h.cpu().numpy().astype(np.float64) - ref_h) / bh).max()))
                worst = max(worst, ratio)
                assert ratio <= 1.0, (what, ratio)
                if mode is not None:                                           # masked entries at the last level are the target itself
                    on = mask != 0
                    if mode == "clamp" or i + 1 == n:
                        assert _same(got.cpu().numpy()[on], target[on]), what
                # the hand composition of the existing stand-alone calls
                if not solver and (mode is None or e is eng):
                    zero = _ns(GO.make(B, Tk, Dk))
                    hand = e.plan_guide_step(_dev(x), _dev(eps), ns or zero, rho if rho is not None else np.zeros(n, np.float32), i,
                                             noise=None if noise is None else _dev(noise), **kw)
                    if mode is not None:
                        hand = e.plan_constrain(hand, _dev(target), _dev(mask, np.uint8), i + 1, mode=mode, **kw)
                    assert _same(got, hand), what
                if solver and G is None and mode != "repaint":
                    hx, hh = e.plan_solver_step(_dev(x), _dev(eps), i, n, _dev(hist) if second else None)
                    if mode == "clamp":
                        hx = torch.where(_dev(mask, np.uint8) != 0, _dev(target), hx)
                    assert _same(got, hx) and _same(got_h, hh), what
                # padded strides, in place: the same bits, and the padding columns keep theirs
                if gi != 1:                                                    # (guide off and guide with anchor: half the cases carry no more)
                    xp = torch.full((B, Tk, DPk), 7.25, device="cuda")
                    xp[:, :, :Dk] = _dev(x)
                    hp = None
                    if solver and second:
                        hp = torch.full((B, Tk, DPk), 3.5, device="cuda")
                        hp[:, :, :Dk] = _dev(hist)
                    pkw = dict(ekw, x0_prev=hp, ldg=DPk, ldc=DPk, inplace=True)
                    out = e.plan_compose_step(xp, _dev(eps), i, **pkw)
                    out, out_h = out if solver else (out, None)
                    assert out is xp and _same(xp[:, :, :Dk].contiguous(), got) and bool((xp[:, :, Dk:] == 7.25).all()), what
                    if hp is not None:
                        assert out_h is hp and _same(hp[:, :, :Dk].contiguous(), got_h) and bool((hp[:, :, Dk:] == 3.5).all()), what
    print(f"compose step D = {Dk} T = {Tk} B = {B}: max |err| / bound = {worst:.3f}")


def test_compose_step_rows_depend_on_the_global_row_only(eng):
    """Both Philox draws are keyed by the global row: rows 1.. of a call at `off` are the rows of a call at off + 1."""
    B, off = 3, 6
    g = rng(77)
    G, ns = _guide(g, B)
    target, mask = _constraint(g, B)
    x, eps = g.standard_normal((B, T, D)).astype(np.float32), g.standard_normal((B, T, D)).astype(np.float32)
    rho = np.full(100, 0.05, np.float32)
    kw = dict(seed=9, sampler="ddpm", n_steps=100, mode="repaint")
    whole = eng.plan_compose_step(_dev(x), _dev(eps), 3, guide=ns, rho=rho, target=target, mask=mask, row_offset=off, **kw)
    part = eng.plan_compose_step(_dev(x[1:]), _dev(eps[1:]), 3, guide=_ns(_rows(G, slice(1, None))), rho=rho, target=target[1:], mask=mask[1:],
                                 row_offset=off + 1, **kw)
    assert _same(whole[1:], part)


# ---- 2. the loops --------------------------------------------------------------------------------------------------------------------------
def _setup(eng, eng12, sampler):
    return (eng12, N12, N12) if sampler == "ddpm" else (eng, N, 100)


def _timestep(sampler, i, n, n_train):
    return int(TS[i]) if sampler == "dpmpp" else RO.step_timestep(i, n_train, n, sampler)


def _c_begin(e, x, target, mask, mode, level, sampler, n, n_train, seed, off):
    """C_level by hand: the stand-alone call on the uniform grid; under dpmpp the table-level coefficients and the same draw."""
    if sampler != "dpmpp":
        return e.plan_constrain(x, _dev(target), _dev(mask, np.uint8), level, mode=mode, seed=seed, row_offset=off, sampler=sampler, n_steps=n)
    B = x.shape[0]
    zc = _draw(seed, off, B, T, D, level, ST_CONS)
    a, s = CN.table_level_coefs(n_train, TS)[level]
    v = target if mode == "clamp" or level == n else GO.fma32(a, target, np.float32(s) * zc.astype(np.float32))
    return torch.where(_dev(mask, np.uint8) != 0, _dev(v), x)


def _by_hand(e, cond, x, sampler, n, n_train, parts, seed, off, begin=0, end=None):
    target, mask, mode = parts.get("target"), parts.get("mask"), parts.get("mode", "repaint")
    if target is not None:
        x = _c_begin(e, x, target, mask, mode, begin, sampler, n, n_train, seed, off)
    h = None
    for i in range(begin, n if end is None else end):
        eps = e.unet_forward(x, _timestep(sampler, i, n, n_train), cond)
        out = e.plan_compose_step(x, eps, i, x0_prev=h, second=h is not None and i < n - 1, seed=seed, row_offset=off, sampler=sampler,
                                  n_steps=n, **parts)
        x, h = out if sampler == "dpmpp" else (out, None)
    return x


LOOP_CASES = [("ddim", "gc"), ("ddpm", "gc"), ("dpmpp", "gc"), ("dpmpp", "g"), ("dpmpp", "c")]


@pytest.mark.parametrize("B", [3, 17])
@pytest.mark.parametrize("sampler,which", LOOP_CASES)
def test_loop_composition_graph_ranges_batches_and_launches(eng, eng12, sampler, which, B):
    """Eager = the hand composition unet_forward + plan_compose_step behind C_begin; graph (capture, replay) = eager; [0, 4) then [4, n) =
    [0, n) under DDIM / DDPM (under dpmpp the history starts empty with every call: the ranges do NOT compose); rows of B = 17 = the same
    rows of B = 20; the launch count is the guided loop's (one launch behind every U-Net evaluation) plus 1 with a constraint; the masked
    entries of the result are the target itself.  All bit for bit."""
    e, n, n_train = _setup(eng, eng12, sampler)
    g = rng(300 + B)
    G20, _ = _guide(g, 20)
    t20, m20 = _constraint(g, 20)
    rho = (np.linspace(1.0, 0.2, n) / GO.lipschitz(G20)).astype(np.float32)
    cond20 = _cond(20)
    cond = cond20[:B].contiguous()
    seed, off = 99, 11
    kw = dict(seed=seed, row_offset=off, sampler=sampler, n_steps=n)

    def parts(rows, mode="repaint"):
        p = {}
        if "g" in which:
            p.update(guide=_ns(_rows(G20, rows)), rho=rho)
        if "c" in which:
            p.update(target=t20[rows], mask=m20[rows], mode=mode)
        return p
    for mode in ("repaint", "clamp") if "c" in which else ("repaint",):
        p = parts(slice(0, B), mode)
        eager = e.plan_sample_composed(cond, use_graph=False, **p, **kw)
        c_eager = e.launch_counts()
        x_t = e.plan_sample_range(cond, 0, 0, seed=seed, row_offset=off, sampler="ddpm" if sampler == "ddpm" else "ddim", n_steps=n)
        hand = _by_hand(e, cond, x_t, sampler, n, n_train, p, seed, off)
        assert torch.isfinite(eager).all() and _same(eager, hand), f"max |diff| = {float((eager - hand).abs().max()):.3e}"
        first = e.plan_sample_composed(cond, use_graph=True, **p, **kw)
        replay = e.plan_sample_composed(cond, use_graph=True, **p, **kw)
        assert _same(first, eager) and _same(replay, eager) and e.launch_counts() == c_eager
        if "c" in which:
            on = m20[:B] != 0
            assert _same(eager.cpu().numpy()[on], t20[:B][on])
        # launches: (e - b) U-Net evaluations + (e - b) + 1 with a constraint -- the guided / solver loop has the first two
        if sampler == "dpmpp":
            e.plan_sample(cond, use_graph=False, **kw)
        else:
            e.plan_sample_guided(cond, _ns(_rows(G20, slice(0, B))), rho, use_graph=False, **kw)
        c_ref = e.launch_counts()
        assert c_eager == (c_ref[0], c_ref[1] + (1 if "c" in which else 0)), (c_eager, c_ref)
        for use_graph in (False, True):
            head = e.plan_sample_composed(cond, step_begin=0, step_end=4, use_graph=use_graph, **p, **kw)
            assert e.launch_counts()[1] < c_eager[1]
            tail = e.plan_sample_composed(cond, step_begin=4, step_end=n, x_init=head, use_graph=use_graph, **p, **kw)
            assert not _same(head, eager) and _same(tail, eager) == (sampler != "dpmpp")
    eager = e.plan_sample_composed(cond, **parts(slice(0, B)), **kw)
    if B == 17:
        big = e.plan_sample_composed(cond20, **parts(slice(0, 20)), **kw)
        assert _same(big[:17], eager)
    # a graph bakes nothing of a guide, a constraint or a seed: other ones through the same captured graph
    G2, _ = _guide(rng(301 + B), B)
    t2, m2 = _constraint(rng(302 + B), B)
    p2 = {}
    if "g" in which:
        p2.update(guide=_ns(G2), rho=(rho * 0.5).astype(np.float32))
    if "c" in which:
        p2.update(target=t2, mask=m2, mode="repaint")
    kw2 = dict(kw, seed=seed + 1)
    other = e.plan_sample_composed(cond, use_graph=True, **p2, **kw2)
    assert _same(other, e.plan_sample_composed(cond, use_graph=False, **p2, **kw2)) and not _same(other, eager)


F64_CASES = [("ddim", "gc", "repaint", 0), ("dpmpp", "c", "repaint", 0), ("dpmpp", "g", None, 0), ("dpmpp", "gc", "clamp", 4),
             ("ddim", "gc", "clamp", 4), ("ddpm", "gc", "repaint", 0)]


@pytest.mark.parametrize("sampler,which,mode,warm", F64_CASES)
def test_loop_against_float64(eng, eng12, sampler, which, mode, warm):
    """The project's 1e-4 against tests/compose_oracle.py on np64's U-Net: guide + constraint, constraint + dpmpp, guide + dpmpp, and all
    three with a warm start (the last `warm` steps from the shifted, noised previous plan; under dpmpp the warm level is the table entry)."""
    e, n, n_train = _setup(eng, eng12, sampler)
    B, seed, off = 3, 17, 2
    g = rng(500 + n + warm + len(which))
    G, ns = _guide(g, B)
    target, mask = _constraint(g, B)
    rho = (np.linspace(1.0, 0.2, n) / GO.lipschitz(G)).astype(np.float32)
    cond = g.uniform(-1, 1, (B, D)).astype(np.float32)
    nz = g.standard_normal((n, B, T, D)).astype(np.float32) if sampler == "ddpm" else None
    p, okw = {}, dict(sampler=sampler, n_train=n_train, n_steps=n, ts=TS if sampler == "dpmpp" else None, step_noise=nz, seed=seed,
                      row_offset=off)
    if "g" in which:
        p.update(guide=ns, rho=rho)
        okw.update(G=G, rho=rho.astype(np.float64))
    if "c" in which:
        p.update(target=target, mask=mask, mode=mode)
        okw.update(target=target, mask=mask, mode=mode)
    begin = 0
    if warm:
        begin = n - warm
        prev = g.uniform(-1, 1, (B, T, D)).astype(np.float32)
        p.update(x_store=_dev(prev), shift=AH)
        x0 = RO.warm_init(prev, AH, _timestep(sampler, begin, n, n_train), _draw(seed, off, B, T, D, 0, ST_INIT), n_train)
    else:
        x_init = g.standard_normal((B, T, D)).astype(np.float32)
        p.update(x_init=_dev(x_init))
        x0 = x_init
    got = e.plan_sample_composed(_dev(cond), step_begin=begin, step_noise=None if nz is None else _dev(nz), seed=seed, row_offset=off,
                                 sampler=sampler, n_steps=n, **p)
    P = np64.to64(planner_params(D=D))
    ref = XO.planner_range_composed(P, cond.astype(np.float64), x0, begin, n, **okw)
    assert_close(got.cpu().numpy(), ref, 1e-4, f"composed {sampler}-{n} {which} {mode} warm = {warm}")
    if warm:
        assert _same(p["x_store"], _dev(prev))                                 # plan_sample_composed reads the table, it does not write it


def test_single_parts_are_the_dedicated_calls_and_existing_calls_keep_bits_and_launches(eng):
    """A composed call with only a guide, or only a constraint, under DDIM is plan_sample_guided / plan_sample_constrained bit for bit; an
    empty mask with nothing else under dpmpp is plan_sample(sampler="dpmpp"); and the free, guided, constrained and solver calls have the
    bits and the launch counts after composed calls that they had before."""
    B = 3
    g = rng(41)
    cond = _cond(B)
    obs_emb = cond[:, None].contiguous()
    _, ns = _guide(g, B)
    target, mask = _constraint(g, B)
    rho = np.full(N, 0.05, np.float32)
    kw = dict(seed=5, row_offset=2, n_steps=N)

    def existing(use_graph):
        out = [eng.plan_sample(cond, sampler="ddim", use_graph=use_graph, **kw)]
        cnt = [eng.launch_counts()]
        out.append(eng.plan_sample_guided(cond, ns, rho, sampler="ddim", use_graph=use_graph, **kw))
        cnt.append(eng.launch_counts())
        out.append(eng.plan_sample_constrained(cond, target, mask, mode="repaint", sampler="ddim", use_graph=use_graph, **kw))
        cnt.append(eng.launch_counts())
        out.append(eng.plan_sample(cond, sampler="dpmpp", use_graph=use_graph, **kw))
        cnt.append(eng.launch_counts())
        out.append(eng.agent_sample(obs_emb, 1, seed=5, row_offset=2, sampler="ddim", planner_steps=N, idm_steps=N, use_graph=use_graph)[2])
        cnt.append(eng.launch_counts())
        return out, cnt
    before = [existing(ug) for ug in (False, True, True)]
    free, guided, constrained, solver, _ = before[0][0]
    for use_graph in (False, True, True):
        ckw = dict(use_graph=use_graph, **kw)
        assert _same(eng.plan_sample_composed(cond, guide=ns, rho=rho, sampler="ddim", **ckw), guided)
        assert eng.launch_counts() == before[0][1][1]
        assert _same(eng.plan_sample_composed(cond, target=target, mask=mask, mode="repaint", sampler="ddim", **ckw), constrained)
        assert eng.launch_counts() == before[0][1][2]
        assert _same(eng.plan_sample_composed(cond, sampler="ddim", **ckw), free) and eng.launch_counts() == before[0][1][0]
        empty = eng.plan_sample_composed(cond, target=target, mask=np.zeros_like(mask), mode="repaint", sampler="dpmpp", **ckw)
        assert _same(empty, solver) and _same(eng.plan_sample_composed(cond, sampler="dpmpp", **ckw), solver)
        both = eng.plan_sample_composed(cond, guide=ns, rho=rho, target=target, mask=mask, sampler="dpmpp", **ckw)
        assert not _same(both, solver) and eng.launch_counts() == (before[0][1][3][0], before[0][1][3][1] + 1)
        x, plan, act = eng.agent_sample_composed(obs_emb, 1, guide=ns, rho=rho, target=target, mask=mask, sampler="dpmpp", seed=5, row_offset=2,
                                                 planner_steps=N, idm_steps=N, use_graph=use_graph)
        assert _same(x, both) and _same(plan[:, 1:], x[:, :AH]) and torch.isfinite(act).all()
    after = [existing(ug) for ug in (False, True, True)]
    for outs, cnts in before + after:
        assert all(_same(a, b) for a, b in zip(outs, before[0][0])) and cnts == before[0][1]


def test_split_batch(eng):
    """B = 1040 runs as two loops (1024 + 16 rows): each part gets its rows of the guide, the constraint and the warm table, and its own
    row_offset."""
    B, b1, off = 1040, 1024, 7
    g = rng(1000)
    cond = _dev(g.uniform(-1, 1, (B, D)))
    G, ns = _guide(g, B)
    target, mask = _constraint(g, B)
    store = _dev(g.uniform(-1, 1, (B, T, D)))
    rho = np.full(N, 0.5 / GO.lipschitz(G), np.float32)
    kw = dict(seed=21, sampler="dpmpp", n_steps=N, step_begin=6, shift=AH, mode="repaint", rho=rho)
    whole = eng.plan_sample_composed(cond, guide=ns, target=target, mask=mask, x_store=store, row_offset=off, **kw)
    c_whole = eng.launch_counts()
    first = eng.plan_sample_composed(cond[:b1].contiguous(), guide=_ns(_rows(G, slice(0, b1))), target=target[:b1], mask=mask[:b1],
                                     x_store=store[:b1].contiguous(), row_offset=off, **kw)
    c1 = eng.launch_counts()
    second = eng.plan_sample_composed(cond[b1:].contiguous(), guide=_ns(_rows(G, slice(b1, None))), target=target[b1:], mask=mask[b1:],
                                      x_store=store[b1:].contiguous(), row_offset=off + b1, **kw)
    c2 = eng.launch_counts()
    assert torch.isfinite(whole).all() and _same(whole[:b1], first) and _same(whole[b1:], second)
    assert c_whole == (c1[0] + c2[0], c1[1] + c2[1])
    slots = torch.arange(B - 1, -1, -1, dtype=torch.int32, device="cuda")      # a device slot table: every row reads the mirrored row
    flipped = eng.plan_sample_composed(cond, guide=ns, target=target, mask=mask, x_store=store.flip(0).contiguous(), slot=slots, row_offset=off, **kw)
    assert _same(flipped, whole)
    eng.check_fault()


def test_refusals(eng):
    B = 3
    cond = _cond(B)
    G, ns = _guide(rng(5), B)
    target, mask = _constraint(rng(6), B)
    rho = np.full(N, 0.05, np.float32)
    x = _dev(rng(6).standard_normal((B, T, D)))
    store = torch.zeros(4, T, D, device="cuda")
    kw = dict(sampler="dpmpp", n_steps=N)

    def bad(**ch):
        return SimpleNamespace(**dict(vars(ns), **ch))
    for g2, word in ((bad(lam=-G["lam"] - 1), "lam"), (bad(beta=-G["beta"] - 1), "beta"), (bad(lo=G["hi"] + 1), "lo"),
                     (bad(lam=np.full(D, np.inf, np.float32)), "lam")):
        with pytest.raises(LDPHipError, match=word):
            eng.plan_sample_composed(cond, guide=g2, rho=rho, target=target, mask=mask, **kw)
        with pytest.raises(LDPHipError, match=word):
            eng.agent_sample_composed(cond[:, None].contiguous(), 1, guide=g2, rho=rho, planner_steps=N, idm_steps=N, sampler="dpmpp")
    for r2 in (rho[:5], np.concatenate([rho, rho]), -rho, np.full(N, np.nan, np.float32)):
        with pytest.raises(LDPHipError, match="rho"):
            eng.plan_sample_composed(cond, guide=ns, rho=r2, **kw)
    with pytest.raises(LDPHipError, match="mode"):
        eng.plan_sample_composed(cond, target=target, mask=mask, mode=7, **kw)
    with pytest.raises(LDPHipError, match="slot"):
        eng.plan_sample_composed(cond, x_store=store, slot=[0, 4, 1], step_begin=5, **kw)
    with pytest.raises(LDPHipError, match="x_init"):
        eng.plan_sample_composed(cond, x_store=store, x_init=x, step_begin=5, **kw)
    with pytest.raises(LDPHipError, match="ldp_solver_timesteps"):          # (the binding registers a table by itself: the bare C call, n = 7)
        check(eng.lib.ldp_plan_sample_composed(eng._h, cond.data_ptr(), None, None, None, 0, 0, 2, 7, 0, 7, x.data_ptr(), B, 0, None))
    with pytest.raises(LDPHipError, match="step"):
        eng.plan_compose_step(x, x, N, **kw)
    with pytest.raises(LDPHipError, match="x0_prev"):
        eng.plan_compose_step(x, x, 3, second=True, **kw)
    with pytest.raises(LDPHipError, match="step_begin"):
        eng.agent_sample_composed(cond[:, None].contiguous(), 1, step_begin=3, planner_steps=N, idm_steps=N, sampler="ddim")
    with pytest.raises(ValueError, match="go together"):
        eng.plan_sample_composed(cond, guide=ns, **kw)
    with pytest.raises(ValueError, match="both required"):
        eng.plan_sample_composed(cond, target=target, **kw)
    with pytest.raises(ValueError, match="x_store"):
        eng.plan_sample_composed(cond, shift=2, **kw)
    assert torch.isfinite(eng.plan_sample_composed(cond, guide=ns, rho=rho, target=target, mask=mask, **kw)).all()
    eng.check_fault()


# ---- 3. the agent ----------------------------------------------------------------------------------------------------------------------------
def test_agent_plan_and_controller():
    from latent_diffusion_planning_amd.agent import _seed_of
    ag, data = make_agent("rm", planner_params(), idm_params())
    try:
        e = ag._engine
        B = 3
        batch = cfgs.synth_latent_batch(data, B, 1, 2)
        goal = ag._goal_embedding(cfgs.synth_latent_batch(data, B, 1, 5)["obs"], B)
        obs_emb = ag.get_obs_cond(ag._vae_encode_t(ag._postprocess(batch)["obs"])).contiguous()
        lo, hi, amode = ag._action_bounds()
        akw = dict(action_bounds=(lo, hi), action_mode=amode)
        # plan = agent_sample_composed by hand, all three parts under dpmpp
        gd = ag.build_guide(B, smooth=0.1, anchor=True, bound_weight=0.5, lo=-0.8, hi=0.8, scale=0.5)
        _, m0 = ag.plan(batch, 8, n_steps=N)
        prev = m0["x"].tensor
        action, m = ag.plan(batch, 8, guide=gd, goal=goal, mode="repaint", prev=prev, warm_steps=4, sampler="dpmpp", n_steps=N, row_offset=4)
        assert sorted(m) == ["guide_cost", "plan", "plan_viz", "x"]
        x = m["x"].tensor
        ts = e.solver_tables[N]
        tg, mk = CN.build_constraint(ag.config, B, goal=goal)
        gd2 = GD.Guide(gd.cfg, B, gd.target, gd.weight, obs_emb[:, 0].contiguous(), gd.lam, gd.beta, gd.lo, gd.hi, gd.scale, gd.schedule, e, gd.wmax)
        store = prev.clone()
        x2, plan2, act2 = e.agent_sample_composed(obs_emb, 1, guide=gd2, rho=gd.step_sizes_on(ts), target=tg, mask=mk, mode="repaint",
                                                  x_store=store, shift=AH, step_begin=N - 4, seed=_seed_of(8), row_offset=4, sampler="dpmpp",
                                                  planner_steps=N, idm_steps=N, **akw)
        assert _same(x, x2) and _same(m["plan"].tensor, plan2) and _same(action.tensor, act2) and _same(store, x2)
        assert _same(m["guide_cost"].tensor, e.plan_guide_cost(x, gd2)) and _same(x[:, AH - 1], goal)
        assert _same(prev, m0["x"].tensor)                                     # (the caller's prev is not written)
        # a warm start alone is sample_warm, bit for bit
        aw, mw = ag.sample_warm(batch, 8, prev, 4, n_steps=N, row_offset=4)
        ap, mp = ag.plan(batch, 8, prev=prev, warm_steps=4, n_steps=N, row_offset=4)
        assert _same(mw["x"].tensor, mp["x"].tensor) and _same(aw.tensor, ap.tensor) and _same(mw["plan"].tensor, mp["plan"].tensor)

        # a smoothness-only guide at the descent bound next to a clamp goal: every sample's cost is below sample_constrained's.  First on the
        # float64 oracle, for these inputs (the drawn x_T read back from the device)
        sm = ag.build_guide(B, smooth=0.25, schedule="constant")               # L = 1, scale None: rho = 1 / L
        rho = sm.step_sizes(N, "ddim")
        assert sm.lipschitz == 1.0 and np.all(rho == 1.0)
        G = GO.make(B, T, D, lam=0.25)
        cond = obs_emb[:, 0].contiguous()
        x_t = e.plan_sample_range(cond, 0, 0, seed=_seed_of(8), sampler="ddim", n_steps=N).cpu().numpy()
        P = np64.to64(planner_params())
        o = dict(sampler="ddim", n_steps=N, target=tg.cpu().numpy(), mask=mk, mode="clamp")
        c64 = cond.cpu().numpy().astype(np.float64)
        j_c = GO.cost(XO.planner_range_composed(P, c64, x_t, 0, N, **o), G)
        j_g = GO.cost(XO.planner_range_composed(P, c64, x_t, 0, N, G=G, rho=rho.astype(np.float64), **o), G)
        print(f"smoothness guide next to a clamp goal, float64 oracle: J guided / J constrained per sample = {(j_g / j_c).round(3).tolist()}")
        assert (j_g < j_c).all()
        _, mg = ag.plan(batch, 8, guide=sm, goal=goal, mode="clamp", n_steps=N)
        _, mc = ag.sample_constrained(batch, 8, goal=goal, mode="clamp", sampler="ddim", n_steps=N)
        jg, jc = np.array(mg["guide_cost"]), e.plan_guide_cost(mc["x"].tensor, sm).cpu().numpy()
        print(f"smoothness guide next to a clamp goal, GPU: J guided / J constrained per sample = {(jg / jc).round(3).tolist()}")
        assert (jg < jc).all() and _same(mg["x"].tensor[:, AH - 1], goal) and _same(mc["x"].tensor[:, AH - 1], goal)
        assert_close(jg, j_g, 1e-4 * max(1.0, float(j_g.max())), "guide_cost against the oracle")

        # Controller: three calls with a slot reset in between make the warm and cold engine calls group_rows predicts, and write their slots
        calls = []
        real = e.agent_sample_composed

        def spy(emb, oh, **kw):
            calls.append((int(emb.shape[0]), kw.get("row_offset"), kw.get("step_begin", 0), kw.get("x_store") is not None,
                          None if kw.get("slot") is None else [int(v) for v in kw["slot"].cpu()]))
            return real(emb, oh, **kw)
        e.agent_sample_composed = spy
        ct = ag.controller(4, warm_steps=4, sampler="dpmpp", n_steps=N)
        plan_of = []
        for rnd, slots in enumerate(([0, 1, 2], [2, 0, 3], [1, 3, 0])):
            if rnd == 2:
                ct.reset([3])
            order, n_warm = group_rows(ct.valid, slots)
            del calls[:]
            a, mm = ct.act(batch, 8 + rnd, slots, guide=ag.build_guide(B, smooth=0.25, scale=0.5), goal=goal, mode="clamp")
            want = ([(n_warm, 0, N - 4, True, [slots[i] for i in order[:n_warm]])] if n_warm else []) + \
                   ([(B - n_warm, n_warm, 0, False, None)] if n_warm < B else [])
            assert calls == want, (calls, want)
            xs = mm["x"].tensor
            for row, s in enumerate(slots):
                assert _same(ct.table[s], xs[row])
            assert _same(xs[:, AH - 1], goal) and torch.isfinite(a.tensor).all()
            plan_of.append(xs)
        assert ct.calls == dict(warm=2, cold=3) and ct.valid == [True] * 4
        del e.agent_sample_composed
        e.check_fault()
    finally:
        ag._engine.close()
