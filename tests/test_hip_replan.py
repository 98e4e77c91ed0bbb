"""Warm-started replanning on the GPU (csrc/replan.hip, the step range of csrc/engine.hip, LDPAgent.replanner) -- DESIGN.md 4.16.
rm_lift shapes (T = 8, D = 25 padded to 32, action_horizon = 4); B = 3 sits inside one 16-row bucket, B = 17 spans two tiles.  Neither
is split by the engine's batch_split(), which leaves every batch below 64 tiles whole: B_SPLIT = 1040 (65 tiles) is the smallest batch
that runs as two loops, 1024 + 16 rows, and test 10 is the one that takes that branch."""
import numpy as np
import pytest
import torch

from latent_diffusion_planning_amd.engine import HipEngine, philox_normal
from latent_diffusion_planning_amd._lib import LDPHipError
from oracle import np64
from tests import cfgs, replan_oracle as RO
from tests.util import assert_close, idm_params, make_agent, planner_params, rng

pytestmark = pytest.mark.gpu

D, A, T, AH, DP = 25, 7, 8, 4, 32
SHIFTS = (0, AH, T - 1, T + 3)
RANGE_CASES = [("ddim", 10, 6), ("ddpm", 100, 90)]
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


def _eps(seed, row_offset, B):
    """The LDP_PHILOX_STREAM_INIT draw of rows row_offset .. row_offset + B: element (global row * T + j) * 32 + c, step 0, stream 1."""
    return philox_normal(seed, row_offset * T * DP, 0, 1, B * T * DP).reshape(B, T, DP)[:, :, :D].contiguous()


def _t_begin(sampler, n, begin):
    return RO.step_timestep(begin, 100, n, sampler)


# ---- 1. range composition, bitwise ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 17])
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("sampler,n,m", RANGE_CASES)
def test_range_composition_is_bitwise(eng, sampler, n, m, use_graph, B):
    cond = _cond(B)
    kw = dict(seed=77, row_offset=5, sampler=sampler, n_steps=n, use_graph=use_graph)
    whole = eng.plan_sample(cond, **kw)
    head = eng.plan_sample_range(cond, 0, m, **kw)
    tail = eng.plan_sample_range(cond, m, n, x_init=head, **kw)
    assert torch.isfinite(whole).all() and not _same(head, whole)
    assert _same(tail, whole), f"max |diff| = {float((tail - whole).abs().max()):.3e}"
    # the whole range through the new entry point is the old call
    assert _same(eng.plan_sample_range(cond, 0, n, **kw), whole)


# ---- 2. the empty range ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 17])
def test_empty_range_returns_the_initial_state(eng, B):
    cond = _cond(B)
    got = eng.plan_sample_range(cond, 0, 0, seed=31, row_offset=9, sampler="ddim", n_steps=10)
    assert _same(got, _eps(31, 9, B))                                          # x_T as philox_normal gives it for the same key
    x0 = _dev(rng(2).standard_normal((B, T, D)))
    assert _same(eng.plan_sample_range(cond, 4, 4, x_init=x0, sampler="ddim", n_steps=10), x0)
    for begin, end, word in ((-1, 3, "step_begin"), (11, 11, "step_begin"), (4, 3, "step_end"), (0, 11, "step_end")):
        with pytest.raises(LDPHipError, match=word):
            eng.plan_sample_range(cond, begin, end, sampler="ddim", n_steps=10)


# ---- 3. warm init: the shift ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 17])
@pytest.mark.parametrize("shift", SHIFTS)
def test_warm_init_copies_the_shifted_rows(eng, shift, B):
    """At the last step (t = 0) s = sqrt(1 - abar_0) = 0.02 while a = 0.9998: with x_prev holding small integers that name their own
    (slot, position, channel), (x - s * eps) / a rounds back to that integer -- so every output element names the element it was copied from."""
    n_slots = B + 4
    code = (np.arange(n_slots)[:, None, None] * 64 + np.arange(T)[None, :, None] * 8 + (np.arange(D)[None, None, :] % 8)).astype(np.float32)
    a, s = RO.warm_coefs(0)
    eps = _eps(5, 2, B).cpu().numpy().astype(np.float64)
    assert s * np.abs(eps).max() < 0.25                                        # the noise cannot move a value half way to the next integer
    perm = rng(B).permutation(n_slots)[:B]
    for slot in (None, perm.tolist(), _dev(perm, np.int32)):
        got = eng.plan_warm_init(_dev(code), 9, slot=slot, shift=shift, B=B, seed=5, row_offset=2, sampler="ddim", n_steps=10)
        back = np.rint((got.cpu().numpy().astype(np.float64) - s * eps) / a)
        src = np.arange(B) if slot is None else perm
        want = code[src][:, np.minimum(np.arange(T) + shift, T - 1)]
        assert np.array_equal(back, want)
    with pytest.raises(LDPHipError, match="step_begin"):
        eng.plan_warm_init(_dev(code), 10, B=B, sampler="ddim", n_steps=10)
    with pytest.raises(LDPHipError, match="shift"):
        eng.plan_warm_init(_dev(code), 9, B=B, shift=-1, sampler="ddim", n_steps=10)
    with pytest.raises(LDPHipError, match=r"slot\[1\]"):
        eng.plan_warm_init(_dev(code), 9, slot=[0, n_slots] + list(range(1, B - 1)), sampler="ddim", n_steps=10)


# ---- 4. warm init: the noise ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 17])
@pytest.mark.parametrize("sampler,n,begin", [("ddim", 10, 6), ("ddpm", 100, 90), ("ddim", 10, 0)])
def test_warm_init_against_float64(eng, sampler, n, begin, B):
    """Every element within 2^-23 (|a xs| + |s eps|) of a xs + s eps in float64, with a and s the coefficients the computation is defined
    with (sqrt(abar_t), sqrt(1 - abar_t) from the ddpm_tables restatement in float64, cast to float32).  The bound is the
    two fp32 roundings of fma(a, xs, rn(s eps)): rn(s eps) errs by at most 2^-24 |s eps|, the fused sum by at most 2^-24 of its result,
    which is at most |a xs| + |s eps| (1 + 2^-24)."""
    x_prev = rng(40 + B).standard_normal((B, T, D)).astype(np.float32)
    t = _t_begin(sampler, n, begin)
    a64, s64 = RO.warm_coefs(t)
    a, s = float(np.float32(a64)), float(np.float32(s64))
    eps = _eps(123, 4, B).cpu().numpy().astype(np.float64)
    got = eng.plan_warm_init(_dev(x_prev), begin, seed=123, row_offset=4, sampler=sampler, n_steps=n).cpu().numpy().astype(np.float64)
    xs = RO.shift_hold(x_prev, AH).astype(np.float64)
    ref = a * xs + s * eps
    bound = 2.0 ** -23 * (np.abs(a * xs) + np.abs(s * eps))
    ratio = float((np.abs(got - ref) / bound).max())
    # against the uncast float64 coefficients (np64.ddpm_add_noise itself) the casts add up to 2^-24 relative per term: 1.5 x the bound at most
    ratio64 = float((np.abs(got - RO.warm_init(x_prev, AH, t, eps)) / bound).max())
    print(f"warm init {sampler}-{n} begin {begin} (t = {t}) B = {B}: max |err| / bound = {ratio:.3f} (uncast coefficients: {ratio64:.3f})")
    assert np.isfinite(got).all() and ratio <= 1.0 and ratio64 <= 1.5


# ---- 5. the tail against the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler,n,k,B", [("ddim", 10, 4, 3), ("ddim", 10, 4, 17), ("ddpm", 100, 10, 3)])
def test_resample_tail_against_the_oracle(eng, sampler, n, k, B):
    """(DDPM at B = 3 only: ten float64 U-Net evaluations of 17 plans would take the test beyond a few seconds.)"""
    begin, seed, off = n - k, 17, 3
    g = rng(500 + n + B)
    obs_emb = g.uniform(-1, 1, (B, 1, D)).astype(np.float32)
    x_prev = np.clip(g.standard_normal((B, T, D)) * 0.5, -1, 1).astype(np.float32)
    nz = g.standard_normal((n, B, T, D)).astype(np.float32) if sampler == "ddpm" else None
    store = _dev(x_prev)
    x, plan, _ = eng.agent_resample(_dev(obs_emb), 1, store, begin, x_noise=None if nz is None else _dev(nz), seed=seed, row_offset=off,
                                    sampler=sampler, planner_steps=n, idm_steps=n)
    eps = _eps(seed, off, B).cpu().numpy().astype(np.float64)
    xw = RO.warm_init(x_prev, AH, _t_begin(sampler, n, begin), eps)
    ref = RO.planner_range(np64.to64(planner_params(D=D)), obs_emb[:, 0].astype(np.float64), xw, begin, n, step_noise=nz, n_train=100,
                           n_steps=n, sampler=sampler)
    assert_close(x.cpu().numpy(), ref, 1e-4, f"resample {sampler}-{n} tail {k}: x")
    assert_close(plan.cpu().numpy(), np.concatenate([obs_emb[:, :1].astype(np.float64), ref[:, :AH]], axis=1), 1e-4, "plan")
    assert _same(store, x)


# ---- 6. the joint call and the range call agree ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 17])
def test_resample_is_warm_init_plus_range(eng, B):
    n, begin, seed, off = 10, 6, 99, 11
    g = rng(600 + B)
    obs_emb = _dev(g.uniform(-1, 1, (B, 1, D)))
    x_prev = _dev(g.standard_normal((B, T, D)))
    xw = eng.plan_warm_init(x_prev, begin, seed=seed, row_offset=off, sampler="ddim", n_steps=n)
    want = eng.plan_sample_range(obs_emb[:, 0].contiguous(), begin, n, x_init=xw, seed=seed, row_offset=off, sampler="ddim", n_steps=n)
    got = {}
    for use_graph in (False, True, True):                                      # eager, capture, replay
        x, plan, act = eng.agent_resample(obs_emb, 1, x_prev.clone(), begin, seed=seed, row_offset=off, sampler="ddim", planner_steps=n,
                                          idm_steps=n, use_graph=use_graph)
        assert _same(x, want)
        assert _same(plan[:, 1:], x[:, :AH]) and _same(plan[:, 0], obs_emb[:, 0])
        got.setdefault("plan", plan), got.setdefault("act", act)
        assert _same(plan, got["plan"]) and _same(act, got["act"]) and torch.isfinite(act).all()


# ---- 7. in-place slots ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 17])
def test_resample_writes_its_slots_in_place(eng, B):
    n_slots = B + 5
    g = rng(700 + B)
    # the table sits inside a larger allocation: a write past a row's D columns (the state's padding) or past the table would show
    buf = torch.full(((n_slots + 2) * T * D,), 7.5, device="cuda")
    table = buf[T * D:(n_slots + 1) * T * D].view(n_slots, T, D)
    table.copy_(_dev(g.standard_normal((n_slots, T, D))))
    before = table.clone()
    perm = g.permutation(n_slots)[:B]
    obs_emb = _dev(g.uniform(-1, 1, (B, 1, D)))
    x, _, _ = eng.agent_resample(obs_emb, 1, table, 6, slot=perm.tolist(), seed=4, sampler="ddim", planner_steps=10, idm_steps=10)
    assert _same(table[_dev(perm, np.int64)], x) and torch.isfinite(x).all() and float(x.abs().max()) > 0
    rest = np.setdiff1d(np.arange(n_slots), perm)
    assert _same(table[_dev(rest, np.int64)], before[_dev(rest, np.int64)])
    assert bool((buf[:T * D] == 7.5).all()) and bool((buf[(n_slots + 1) * T * D:] == 7.5).all())
    # the rows were read through the same table: row b started from slot perm[b]'s previous state
    xw = eng.plan_warm_init(before, 6, slot=perm.tolist(), seed=4, sampler="ddim", n_steps=10)
    assert _same(eng.plan_sample_range(obs_emb[:, 0].contiguous(), 6, 10, x_init=xw, seed=4, sampler="ddim", n_steps=10), x)
    # a device-side slot table gives the same bits
    t2 = before.clone()
    x2, _, _ = eng.agent_resample(obs_emb, 1, t2, 6, slot=_dev(perm, np.int32), seed=4, sampler="ddim", planner_steps=10, idm_steps=10)
    assert _same(x2, x) and _same(t2, table)
    with pytest.raises(LDPHipError, match="slot"):
        eng.agent_resample(obs_emb, 1, t2, 6, slot=[n_slots] + list(range(B - 1)), sampler="ddim", planner_steps=10, idm_steps=10)
    with pytest.raises(LDPHipError, match="step_begin"):
        eng.agent_resample(obs_emb, 1, t2, 10, sampler="ddim", planner_steps=10, idm_steps=10)


# ---- 8. the Replanner ---------------------------------------------------------------------------------------------------------------------
def test_replanner_equals_the_two_engine_calls_by_hand():
    ag, data = make_agent("rm", planner_params(), idm_params())
    try:
        eng = ag._engine
        rp = ag.replanner(6, warm_steps=4, sampler="ddim", n_steps=10)
        rp.act(cfgs.synth_latent_batch(data, 2, 1, 1), 5, [2, 0])              # slots 2 and 0 now hold a plan
        table0 = rp.table.clone()
        batch = cfgs.synth_latent_batch(data, 3, 1, 2)
        slots = [0, 5, 2]                                                      # warm, cold, warm -> reordered [row 0, row 2, row 1]
        action, m = rp.act(batch, 8, slots)
        emb = ag.get_obs_cond(ag._vae_encode_t(ag._postprocess(batch)["obs"])).contiguous()[[0, 2, 1]].contiguous()
        lo, hi, mode = ag._action_bounds()
        kw = dict(seed=8, sampler="ddim", planner_steps=10, idm_steps=10, action_bounds=(lo, hi), action_mode=mode)
        hand = table0.clone()
        xw, pw, aw = eng.agent_resample(emb[:2], 1, hand, 6, slot=[0, 2], shift=AH, row_offset=0, **kw)
        xc, pc, ac = eng.agent_sample(emb[2:], 1, row_offset=2, **kw)
        for got, parts in ((m["x"], (xw, xc)), (m["plan"], (pw, pc)), (action, (aw, ac))):
            want = torch.cat(parts)[[0, 2, 1]]                                 # back to the caller's order: rows (0, 1, 2) = positions (0, 2, 1)
            assert _same(got.tensor, want)
        assert _same(rp.table[[0, 2]], xw) and _same(rp.table[5], xc[0]) and _same(rp.table[[1, 3, 4]], table0[[1, 3, 4]])
        assert rp.valid == [True, False, True, False, False, True] and rp.calls == dict(warm=1, cold=2)
        assert np.isfinite(np.array(action)).all()
        eng.check_fault()
    finally:
        ag._engine.close()


# ---- 9. the cost scales with the steps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 17])
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_conv_launches_scale_with_the_executed_steps(eng, use_graph, B):
    n, begin = 10, 6
    cond = _cond(B)
    eng.plan_sample(cond, sampler="ddim", n_steps=n, use_graph=use_graph)
    cold, _ = eng.launch_counts()
    for b0 in (begin, 8, 0):
        for _ in range(2):                                                     # (graph: capture, then replay)
            eng.plan_sample_range(cond, b0, n, x_init=torch.zeros(B, T, D, device="cuda"), sampler="ddim", n_steps=n, use_graph=use_graph)
            warm, _ = eng.launch_counts()
            assert cold > 0 and warm * n == cold * (n - b0), (cold, warm, b0)
    # the joint call: what it saves is the planner launches of the skipped steps (the IDM loop is untouched)
    obs_emb = _dev(rng(9).uniform(-1, 1, (B, 1, D)))
    eng.agent_sample(obs_emb, 1, sampler="ddim", planner_steps=n, idm_steps=n, use_graph=use_graph)
    cold_joint, _ = eng.launch_counts()
    eng.agent_resample(obs_emb, 1, torch.zeros(B, T, D, device="cuda"), begin, sampler="ddim", planner_steps=n, idm_steps=n, use_graph=use_graph)
    warm_joint, _ = eng.launch_counts()
    assert (cold_joint - warm_joint) * n == cold * begin, (cold_joint, warm_joint, cold)


# ---- 10. a batch that the engine splits ----------------------------------------------------------------------------------------------------
def test_split_batch_resample_and_range(eng):
    """B = 1040 runs as two loops (1024 + 16 rows): the second part of ldp_agent_resample takes the rest of the slot table (or, without
    one, the rows of x_store behind the first part) and both parts write back in place; ldp_plan_sample_range forwards its range to both."""
    B, n, begin, seed, off = B_SPLIT, 10, 6, 21, 7
    n_slots = B + 8
    g = rng(1000)
    obs_emb = _dev(g.uniform(-1, 1, (B, 1, D)))
    cond = obs_emb[:, 0].contiguous()
    before = _dev(np.clip(g.standard_normal((n_slots, T, D)) * 0.5, -1, 1))
    perm = g.permutation(n_slots)[:B]
    kw = dict(seed=seed, row_offset=off, sampler="ddim")
    eng.plan_sample(cond, n_steps=n, **kw)
    whole_convs, _ = eng.launch_counts()
    eng.plan_sample(cond[:1024].contiguous(), n_steps=n, **kw)
    first, _ = eng.launch_counts()
    eng.plan_sample(cond[1024:].contiguous(), n_steps=n, **kw)
    second, _ = eng.launch_counts()
    assert first > 0 and second > 0 and whole_convs == first + second          # the batch really ran as two loops: 1024 rows, then 16
    for slot in (perm.tolist(), None):
        table = before.clone()
        x, plan, act = eng.agent_resample(obs_emb, 1, table, begin, slot=slot, planner_steps=n, idm_steps=n, **kw)
        xw = eng.plan_warm_init(before, begin, slot=slot, B=B, n_steps=n, **kw)
        want = eng.plan_sample_range(cond, begin, n, x_init=xw, n_steps=n, **kw)
        assert torch.isfinite(x).all() and torch.isfinite(act).all() and _same(x, want)
        rows = np.arange(B) if slot is None else perm
        assert _same(table[_dev(rows, np.int64)], x) and _same(plan[:, 1:], x[:, :AH])
        rest = np.setdiff1d(np.arange(n_slots), rows)
        assert _same(table[_dev(rest, np.int64)], before[_dev(rest, np.int64)])
    # a bad entry in the SECOND part of a host table is refused before the first part is enqueued: the table is untouched
    bad = perm.copy()
    bad[1030] = n_slots
    table = before.clone()
    with pytest.raises(LDPHipError, match=r"slot\[1030\]"):
        eng.agent_resample(obs_emb, 1, table, begin, slot=bad.tolist(), planner_steps=n, idm_steps=n, **kw)
    torch.cuda.synchronize()
    assert _same(table, before)
    # range composition at this size
    whole = eng.plan_sample(cond, n_steps=n, **kw)
    head = eng.plan_sample_range(cond, 0, begin, n_steps=n, **kw)
    assert _same(eng.plan_sample_range(cond, begin, n, x_init=head, n_steps=n, **kw), whole) and not _same(head, whole)
    eng.check_fault()
