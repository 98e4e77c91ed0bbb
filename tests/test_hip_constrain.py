"""Constrained planning on the GPU (csrc/constrain.hip, the constrained loop of csrc/engine.hip, LDPAgent.sample_constrained) --
DESIGN.md 4.17.  rm_lift shapes (T = 8, D = 25 padded to 32, action_horizon = 4): B = 3 sits inside one 16-row bucket, B = 17 spans two,
and D = 25 is what sends the stand-alone call down the unaligned scalar path while the loops run the 16-byte path on the padded state --
test 3 holds the two against each other bit for bit.  B_SPLIT = 1040 is the smallest batch the engine runs as two loops (1024 + 16)."""
import numpy as np
import pytest
import torch

from latent_diffusion_planning_amd.engine import HipEngine, philox_normal
from latent_diffusion_planning_amd._lib import LDPHipError
from oracle import np64
from tests import cfgs, constrain_oracle as CO
from tests.util import assert_close, idm_params, make_agent, planner_params, rng

pytestmark = pytest.mark.gpu

D, A, T, AH, DP, LAT = 25, 7, 8, 4, 32, 16
N = 10                                                                         # DDIM-10 unless a test says otherwise
MODES = ("clamp", "repaint")
B_SPLIT = 1040


@pytest.fixture(scope="module")
def eng():
    e = HipEngine(obs_dim=D, action_dim=A, global_cond_dim=D, pred_horizon=T, action_horizon=AH)
    e.load_params(planner=planner_params(D=D), idm=idm_params(D=D, A=A))
    yield e
    e.check_fault()
    e.close()


def _dev(a, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _cond(B, seed=1):
    return _dev(rng(seed).uniform(-1, 1, (B, D)))


def _z(seed, row_offset, B, level):
    """The LDP_PHILOX_STREAM_CONSTRAIN draw of rows row_offset .. row_offset + B at `level`, as the device computes it."""
    return philox_normal(seed, row_offset * T * DP, level, 12, B * T * DP).reshape(B, T, DP)[:, :, :D].contiguous()


def _mask(kind, B):
    m = np.zeros((B, T, D), np.uint8)
    if kind == "element":
        m[B - 1, 5, 13] = 1
    elif kind == "row":
        m[B // 2, 2] = 1
    elif kind == "mod4":
        m[:, :, np.arange(D) % 4 == 1] = 1
    elif kind == "last":
        m[:, :, 24] = 255                                                      # any non-zero byte constrains
    elif kind == "all":
        m[:] = 1
    elif kind == "goal":                                                       # a whole state at t = 3 plus three lowdim columns at t = 7 of one row
        m[:, 3] = 1
        m[B - 1, 7, LAT:LAT + 3] = 1
    else:
        raise ValueError(kind)
    return m


def _inputs(B, seed):
    g = rng(seed)
    return g.standard_normal((B, T, D)).astype(np.float32), g.uniform(-1, 1, (B, T, D)).astype(np.float32)


# ---- 1. the kernel alone ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 17])
@pytest.mark.parametrize("kind", ["element", "row", "mod4", "last", "all"])
def test_constrain_kernel(eng, kind, B):
    """Unmasked elements keep their bits; clamp (and repaint at the last level) writes target's bits; repaint below it is within
    2^-23 (|a target| + |s z|) of a target + s z in float64 with the float32 coefficients the computation is defined with -- the two
    roundings of fma(a, target, rn(s z)), the bound test_warm_init_against_float64 derives for the same arithmetic (1.5 x against the
    uncast float64 coefficients)."""
    seed, off = 1234, 6
    x, target = _inputs(B, 10 + B)
    m = _mask(kind, B)
    on = m != 0
    kw = dict(seed=seed, row_offset=off, sampler="ddim", n_steps=N)
    for level in (0, 4, N):
        for mode in MODES:
            got = eng.plan_constrain(_dev(x), _dev(target), _dev(m, np.uint8), level, mode=mode, **kw)
            gb, g64 = _bits(got), got.cpu().numpy().astype(np.float64)
            assert np.array_equal(gb[~on], x.view(np.uint32)[~on]), (kind, level, mode)
            if mode == "clamp" or level == N:
                assert np.array_equal(gb[on], target.view(np.uint32)[on]), (kind, level, mode)
            else:
                z = _z(seed, off, B, level).cpu().numpy().astype(np.float64)
                a64, s64 = CO.level_coefs(level, 100, N, "ddim")
                a, s = float(np.float32(a64)), float(np.float32(s64))
                t64 = target.astype(np.float64)
                bound = 2.0 ** -23 * (np.abs(a * t64) + np.abs(s * z))
                ratio = float((np.abs(g64 - (a * t64 + s * z)) / bound)[on].max())
                ratio64 = float((np.abs(g64 - CO.constrain(x, target, m, level, mode, n_steps=N, sampler="ddim", z=z)) / bound)[on].max())
                print(f"constrain {kind} B = {B} level {level}: max |err| / bound = {ratio:.3f} (uncast coefficients: {ratio64:.3f})")
                assert np.isfinite(g64).all() and ratio <= 1.0 and ratio64 <= 1.5
            # a NaN in target under a zero mask does not reach the state: the same bits as with zeros there
            bad, zero = target.copy(), target.copy()
            bad[~on], zero[~on] = np.nan, 0.0
            assert _same(eng.plan_constrain(_dev(x), _dev(bad), _dev(m, np.uint8), level, mode=mode, **kw),
                         eng.plan_constrain(_dev(x), _dev(zero), _dev(m, np.uint8), level, mode=mode, **kw))
    # the draw depends on the global row only: rows 1.. of a call at `off` are the rows of a call at off + 1
    whole = eng.plan_constrain(_dev(x), _dev(target), _dev(m, np.uint8), 4, mode="repaint", **kw)
    part = eng.plan_constrain(_dev(x[1:]), _dev(target[1:]), _dev(m[1:], np.uint8), 4, mode="repaint", **dict(kw, row_offset=off + 1))
    assert _same(whole[1:], part)


# ---- 2. the empty mask ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 17])
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("sampler,n", [("ddim", 10), ("ddpm", 100)])
def test_empty_mask_is_the_free_loop(eng, sampler, n, use_graph, B):
    cond = _cond(B)
    kw = dict(seed=77, row_offset=5, sampler=sampler, n_steps=n, use_graph=use_graph)
    want = eng.plan_sample_range(cond, 0, n, **kw)
    nan_target = torch.full((B, T, D), float("nan"), device="cuda")            # a select: nothing of target reaches the state
    for mode in MODES:
        got = eng.plan_sample_constrained(cond, nan_target, torch.zeros(B, T, D, dtype=torch.uint8, device="cuda"), mode=mode, **kw)
        assert torch.isfinite(got).all() and _same(got, want), mode


# ---- 3. wiring: the fused loop is the stand-alone pieces composed by hand ----------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 17])
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("mode", MODES)
def test_fused_loop_equals_the_pieces_by_hand(eng, mode, use_graph, B):
    cond = _cond(B)
    _, target = _inputs(B, 30 + B)
    tg, mk = _dev(target), _dev(_mask("goal", B), np.uint8)
    kw = dict(seed=99, row_offset=11, sampler="ddim", n_steps=N)
    fused = eng.plan_sample_constrained(cond, tg, mk, mode=mode, use_graph=use_graph, **kw)
    x = eng.plan_sample_range(cond, 0, 0, **kw)                               # the drawn initial state
    x = eng.plan_constrain(x, tg, mk, 0, mode=mode, **kw)
    for i in range(N):
        x = eng.plan_sample_range(cond, i, i + 1, x_init=x, use_graph=use_graph, **kw)
        x = eng.plan_constrain(x, tg, mk, i + 1, mode=mode, **kw)
    assert torch.isfinite(fused).all() and _same(fused, x), f"max |diff| = {float((fused - x).abs().max()):.3e}"
    on = mk != 0
    assert _same(fused[on], tg[on])
    # an empty constrained range is C_begin alone
    x0 = _dev(rng(3).standard_normal((B, T, D)))
    got = eng.plan_sample_constrained(cond, tg, mk, mode=mode, step_begin=4, step_end=4, x_init=x0, use_graph=use_graph, **kw)
    assert _same(got, eng.plan_constrain(x0, tg, mk, 4, mode=mode, **kw))


# ---- 4. range composition -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 17])
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("mode", MODES)
def test_constrained_ranges_compose_bitwise(eng, mode, use_graph, B):
    cond = _cond(B)
    _, target = _inputs(B, 40 + B)
    tg, mk = _dev(target), _dev(_mask("goal", B), np.uint8)
    kw = dict(mode=mode, seed=7, row_offset=2, sampler="ddim", n_steps=N, use_graph=use_graph)
    whole = eng.plan_sample_constrained(cond, tg, mk, **kw)
    head = eng.plan_sample_constrained(cond, tg, mk, step_begin=0, step_end=6, **kw)
    tail = eng.plan_sample_constrained(cond, tg, mk, step_begin=6, step_end=N, x_init=head, **kw)
    assert torch.isfinite(whole).all() and not _same(head, whole)
    assert _same(tail, whole), f"max |diff| = {float((tail - whole).abs().max()):.3e}"


# ---- 5. against float64 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler,n,begin,B,mode", [("ddim", 10, 0, 3, "clamp"), ("ddim", 10, 0, 3, "repaint"), ("ddim", 10, 6, 17, "repaint"),
                                                    ("ddpm", 100, 90, 3, "repaint")])
def test_constrained_loop_against_float64(eng, sampler, n, begin, B, mode):
    """The project's 1e-4 against tests/constrain_oracle.py.  A tail [begin, n) starts from the constrained head the GPU computed, so with
    composition (test 4) its result is the whole constrained loop's: the steering figure below is always against the whole free loop.
    The float64 oracle gives a median of 0.14 (clamp) / 0.21 (repaint) for DDIM-10 at B = 3."""
    seed, off = 17, 3
    g = rng(500 + n + B)
    cond = g.uniform(-1, 1, (B, D)).astype(np.float32)
    x_init = g.standard_normal((B, T, D)).astype(np.float32)
    target = g.uniform(-1, 1, (B, T, D)).astype(np.float32)
    nz = g.standard_normal((n, B, T, D)).astype(np.float32) if sampler == "ddpm" else None
    m = _mask("goal", B)
    tg, mk = _dev(target), _dev(m, np.uint8)
    kw = dict(seed=seed, row_offset=off, sampler=sampler, n_steps=n, step_noise=None if nz is None else _dev(nz))
    start = _dev(x_init) if begin == 0 else eng.plan_sample_constrained(_dev(cond), tg, mk, mode=mode, step_begin=0, step_end=begin,
                                                                          x_init=_dev(x_init), **kw)
    got = eng.plan_sample_constrained(_dev(cond), tg, mk, mode=mode, step_begin=begin, step_end=n, x_init=start, **kw)
    ref = CO.planner_range_constrained(np64.to64(planner_params(D=D)), cond.astype(np.float64), start.cpu().numpy(), begin, n, target, m, mode,
                                       step_noise=nz, n_train=100, n_steps=n, sampler=sampler, seed=seed, row_offset=off)
    assert_close(got.cpu().numpy(), ref, 1e-4, f"constrained {sampler}-{n} [{begin}, {n}) B = {B} {mode}")
    on = m != 0
    assert np.array_equal(_bits(got)[on], target.view(np.uint32)[on])           # the constraint is met exactly
    free = eng.plan_sample(_dev(cond), x_init=_dev(x_init), **kw)
    moved = float(np.median(np.abs(got.cpu().numpy() - free.cpu().numpy())[~on]))
    print(f"constrained {sampler}-{n} [{begin}, {n}) B = {B} {mode}: median |constrained - free| over the free entries = {moved:.3f}")
    assert moved > 1e-2                                                        # not a no-op: the constraint steers the rest of the plan


# ---- 6. launch counts -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 17])
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_one_launch_per_level(eng, use_graph, B):
    cond = _cond(B)
    _, target = _inputs(B, 60 + B)
    tg, mk = _dev(target), _dev(_mask("goal", B), np.uint8)
    x0 = torch.zeros(B, T, D, device="cuda")
    kw = dict(sampler="ddim", n_steps=N, use_graph=use_graph)
    for begin, end in ((0, N), (6, N), (2, 5)):
        for mode in MODES:
            for _ in range(2):                                                 # (graph: capture, then replay)
                eng.plan_sample_range(cond, begin, end, x_init=x0, **kw)
                conv0, all0 = eng.launch_counts()
                eng.plan_sample_constrained(cond, tg, mk, mode=mode, step_begin=begin, step_end=end, x_init=x0, **kw)
                conv1, all1 = eng.launch_counts()
                assert conv0 > 0 and conv1 == conv0 and all1 == all0 + (end - begin) + 1, (begin, end, mode, conv0, conv1, all0, all1)
    # the joint call: the planner loop's n + 1 launches more, nothing else
    obs_emb = _dev(rng(9).uniform(-1, 1, (B, 1, D)))
    for _ in range(2):
        eng.agent_sample(obs_emb, 1, sampler="ddim", planner_steps=N, idm_steps=N, use_graph=use_graph)
        conv0, all0 = eng.launch_counts()
        eng.agent_sample_constrained(obs_emb, 1, tg, mk, sampler="ddim", planner_steps=N, idm_steps=N, use_graph=use_graph)
        conv1, all1 = eng.launch_counts()
        assert conv1 == conv0 and all1 == all0 + N + 1, (conv0, conv1, all0, all1)


# ---- 7. a batch that the engine splits -------------------------------------------------------------------------------------------------------
def test_split_batch(eng):
    """B = 1040 runs as two loops (1024 + 16 rows): each part gets its rows of target and mask and its own row_offset."""
    B, b1, off = B_SPLIT, 1024, 7
    g = rng(1000)
    cond = _dev(g.uniform(-1, 1, (B, D)))
    tg = _dev(g.uniform(-1, 1, (B, T, D)))
    m = _mask("goal", B)
    m[:, 5, np.arange(D) % 4 == 1] = (np.arange(B) % 3 == 0)[:, None]          # rows differ, so a part with the wrong rows would show
    mk = _dev(m, np.uint8)
    kw = dict(mode="repaint", seed=21, sampler="ddim", n_steps=N)
    whole = eng.plan_sample_constrained(cond, tg, mk, row_offset=off, **kw)
    conv_whole, all_whole = eng.launch_counts()
    first = eng.plan_sample_constrained(cond[:b1].contiguous(), tg[:b1].contiguous(), mk[:b1].contiguous(), row_offset=off, **kw)
    conv1, all1 = eng.launch_counts()
    second = eng.plan_sample_constrained(cond[b1:].contiguous(), tg[b1:].contiguous(), mk[b1:].contiguous(), row_offset=off + b1, **kw)
    conv2, all2 = eng.launch_counts()
    assert torch.isfinite(whole).all() and _same(whole[:b1], first) and _same(whole[b1:], second)
    assert conv1 > 0 and conv2 > 0 and conv_whole == conv1 + conv2 and all_whole == all1 + all2
    on = mk != 0
    assert _same(whole[on], tg[on])
    # the joint call splits the same way
    obs_emb = cond[:, None].contiguous()
    x, plan, act = eng.agent_sample_constrained(obs_emb, 1, tg, mk, mode="repaint", seed=21, row_offset=off, sampler="ddim", planner_steps=N,
                                                idm_steps=N)
    assert _same(x, whole) and _same(plan[:, 1:], x[:, :AH]) and torch.isfinite(act).all()
    eng.check_fault()


# ---- 8. the joint call ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 17])
@pytest.mark.parametrize("mode", MODES)
def test_joint_call(eng, mode, B):
    seed, off = 99, 11
    g = rng(600 + B)
    obs_emb = _dev(g.uniform(-1, 1, (B, 1, D)))
    tg, mk = _dev(g.uniform(-1, 1, (B, T, D))), _dev(_mask("goal", B), np.uint8)
    want = eng.plan_sample_constrained(obs_emb[:, 0].contiguous(), tg, mk, mode=mode, seed=seed, row_offset=off, sampler="ddim", n_steps=N)
    first = {}
    for use_graph in (False, True, True):                                      # eager, capture, replay
        x, plan, act = eng.agent_sample_constrained(obs_emb, 1, tg, mk, mode=mode, seed=seed, row_offset=off, sampler="ddim",
                                                    planner_steps=N, idm_steps=N, use_graph=use_graph)
        assert _same(x, want)
        assert _same(plan[:, 1:], x[:, :AH]) and _same(plan[:, 0], obs_emb[:, 0])
        # the IDM loop is agent_sample's, on the constrained plan
        tr = torch.cat([plan[:, :-1], plan[:, 1:]], dim=-1).reshape(B * AH, 2 * D).contiguous()
        a = eng.idm_sample(tr, seed=seed, row_offset=off * AH, sampler="ddim", n_steps=N).reshape(B, AH, A)
        assert _same(act, a) and torch.isfinite(act).all() and torch.isfinite(x).all()
        first.setdefault("act", act)
        assert _same(act, first["act"])


# ---- 9. LDPAgent.sample_constrained --------------------------------------------------------------------------------------------------------
def test_agent_sample_constrained():
    ag, data = make_agent("rm", planner_params(), idm_params())
    try:
        eng = ag._engine
        B = 3
        batch = cfgs.synth_latent_batch(data, B, 1, 2)
        goal_obs = cfgs.synth_latent_batch(data, B, 1, 5)["obs"]
        goal = ag._goal_embedding(goal_obs, B)
        kw = dict(sampler="ddim", n_steps=N)
        for mode in MODES:
            for gl in (goal, goal_obs):                                        # an embedding, an observation dict
                action, m = ag.sample_constrained(batch, 8, goal=gl, mode=mode, **kw)
                assert sorted(m) == ["plan", "plan_viz", "x"]
                x, plan = m["x"].tensor, m["plan"].tensor
                assert tuple(x.shape) == (B, T, D) and tuple(plan.shape) == (B, AH + 1, D) and tuple(action.shape) == (B, AH, A)
                assert _same(x[:, AH - 1], goal) and _same(plan[:, AH], goal)  # the default t_goal is the last executed state of the plan
                assert np.isfinite(np.array(action)).all() and torch.isfinite(x).all()
        # a partial goal at several steps
        action, m = ag.sample_constrained(batch, 8, goal=goal, goal_dims="lowdim", t_goal=[1, 3, 7], **kw)
        x = m["x"].tensor
        for t in (1, 3, 7):
            assert _same(x[:, t, LAT:], goal[:, LAT:]) and not _same(x[:, t, :LAT], goal[:, :LAT])
        free_a, free_m = ag.sample_warm(batch, 8, None, None, **kw)            # the cold call that also returns 'x'
        assert not _same(x, free_m["x"].tensor)
        # an explicit target with a broadcast mask
        tg = _dev(rng(4).uniform(-1, 1, (B, T, D)))
        mk = np.zeros((T, D), bool)
        mk[6, 20:] = True
        action, m = ag.sample_constrained(batch, 8, target=tg, mask=mk, mode="clamp", **kw)
        assert _same(m["x"].tensor[:, 6, 20:], tg[:, 6, 20:])
        # the empty constraint is the free call
        action, m = ag.sample_constrained(batch, 8, **kw)
        assert _same(m["x"].tensor, free_m["x"].tensor) and _same(m["plan"].tensor, free_m["plan"].tensor)
        assert _same(action.tensor, free_a.tensor)
        # a training batch (frames beyond obs_horizon) also reports plan_mse
        _, m = ag.sample_constrained(cfgs.synth_latent_batch(data, B, T + 1, 2), 8, goal=goal, **kw)
        assert sorted(m) == ["plan", "plan_mse", "plan_viz", "x"] and np.isfinite(float(np.array(m["plan_mse"])))
        with pytest.raises(ValueError, match="mode"):
            ag.sample_constrained(batch, 8, goal=goal, mode="blend", **kw)
        with pytest.raises(ValueError, match="t_goal"):
            ag.sample_constrained(batch, 8, goal=goal, t_goal=T, **kw)
        with pytest.raises(ValueError, match="goal"):
            ag.sample_constrained(batch, 8, goal=goal[:2], **kw)
        eng.check_fault()
    finally:
        ag._engine.close()


# ---- 10. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals(eng):
    B = 3
    cond = _cond(B)
    x, target = _inputs(B, 5)
    xd, tg, mk = _dev(x), _dev(target), _dev(_mask("goal", B), np.uint8)
    kw = dict(sampler="ddim", n_steps=N)
    with pytest.raises(ValueError, match="mode"):
        eng.plan_constrain(xd, tg, mk, 0, mode="blend", **kw)
    for bad in (0, 3, -1):                                                     # the library's own check of the integer
        with pytest.raises(LDPHipError, match="mode"):
            eng.plan_constrain(xd, tg, mk, 0, mode=bad, **kw)
        with pytest.raises(LDPHipError, match="mode"):
            eng.plan_sample_constrained(cond, tg, mk, mode=bad, **kw)
    for level in (-1, N + 1):
        with pytest.raises(LDPHipError, match="level"):
            eng.plan_constrain(xd, tg, mk, level, **kw)
    for begin, end, word in ((-1, 3, "step_begin"), (4, 3, "step_end"), (0, N + 1, "step_end")):
        with pytest.raises(LDPHipError, match=word):
            eng.plan_sample_constrained(cond, tg, mk, step_begin=begin, step_end=end, **kw)
    with pytest.raises(ValueError, match="target"):
        eng.plan_constrain(xd, tg[:, :, :24], mk, 0, **kw)
    with pytest.raises(ValueError, match="mask"):
        eng.plan_sample_constrained(cond, tg, mk[:2], **kw)
    with pytest.raises(ValueError, match="mask"):
        eng.plan_constrain(xd, tg, mk.float(), 0, **kw)
    with pytest.raises(ValueError, match="target and mask"):
        eng.plan_sample_constrained(cond, tg, None, **kw)
    obs_emb = cond[:, None].contiguous()
    with pytest.raises(ValueError, match="warm start"):
        eng.agent_sample_constrained(obs_emb, 1, tg, mk, planner_steps=N, idm_steps=N, sampler="ddim", x_store=torch.zeros(B, T, D, device="cuda"))
    # nothing above left the engine in a bad state
    assert torch.isfinite(eng.plan_sample_constrained(cond, tg, mk, **kw)).all()
    eng.check_fault()
