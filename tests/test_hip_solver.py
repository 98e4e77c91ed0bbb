"""The DPM-Solver++(2M) sampler on the GPU (csrc/solver.hip, the sampler-2 branch of the planner loop, HipEngine / LDPAgent plumbing) --
DESIGN.md 4.18.  test_hip_constrain.py's shapes (T = 8, action_horizon = 4): D = 25 padded to 32 sends the stand-alone call down the scalar
path while the loop runs 16-byte accesses on the padded state and history and 32-bit ones on the unpadded eps -- test 3 holds the two
against each other bit for bit; D = 32 runs the all-vector path once.  B = 3 sits inside one 16-row bucket, B = 17 spans two; B = 1040
is the smallest batch the engine runs as two loops."""
import numpy as np
import pytest
import torch

from latent_diffusion_planning_amd import schedule as S
from latent_diffusion_planning_amd._lib import LDPHipError
from latent_diffusion_planning_amd.engine import HipEngine
from oracle import np64
from tests import cfgs, solver_oracle as SO
from tests.util import assert_close, idm_params, make_agent, planner_params, rng

pytestmark = pytest.mark.gpu

D, A, T, AH = 25, 7, 8, 4
N_TRAIN = 100
EINVAL, ESTATE = -1, -2
U = 2.0 ** -24                                                                 # unit round-off of float32
SCHED = S.make_schedule(N_TRAIN)


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


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def _emulate(x, eps, p, k, second):
    """The kernel's arithmetic, rounding for rounding, on float64 hardware: every product of two float32 numbers is exact in float64, so
    each line rounds once to float32 where the kernel does (a float64 sum of such terms rounds at 2^-53 first: it can only matter on an
    exact float32 tie).  k: one float32 coefficient row."""
    x, eps, p = (np.asarray(a, np.float64) for a in (x, eps, p))
    sg, inv_a, c_x, c_d, w = (float(k[j]) for j in (2, 1, 3, 4, 5))
    a1 = _f32(x - sg * eps)
    x0 = np.clip(_f32(a1.astype(np.float64) * inv_a), np.float32(-1), np.float32(1))
    d = x0
    if second:
        d1 = _f32(x0.astype(np.float64) - p)
        d = _f32(w * d1.astype(np.float64) + x0.astype(np.float64))
    m = _f32(c_d * d.astype(np.float64))
    return _f32(c_x * x + m.astype(np.float64)), x0


def _exact_and_bound(x, eps, p, k, second):
    """The update in float64 with the coefficient row k, and the bound on what the float32 kernel may differ from it."""
    x, eps, p = (np.asarray(a, np.float64) for a in (x, eps, p))
    sg, inv_a, c_x, c_d, w = (float(k[j]) for j in (2, 1, 3, 4, 5))
    a1 = x - sg * eps
    x0 = np.clip(a1 * inv_a, -1.0, 1.0)
    A1 = np.abs(x) + np.abs(sg * eps)                                          # >= |a1|
    e0 = 2.0 * U * abs(inv_a) * A1
    d, DV, ed = x0, np.abs(x0), e0
    if second:
        d = x0 + w * (x0 - p)
        D1 = np.abs(x0) + np.abs(p)                                            # >= |d1|
        DV = np.abs(x0) + abs(w) * D1                                          # >= |Dv|
        ed = U * DV + abs(w) * U * D1 + (1.0 + abs(w)) * e0
    M = abs(c_d) * DV                                                          # >= |m|
    out = c_x * x + c_d * d
    return out, x0, (U * (np.abs(c_x * x) + 2.0 * M) + abs(c_d) * ed) * (1.0 + 1e-5)


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 17])
@pytest.mark.parametrize("Dk", [25, 32])
def test_solver_kernel(Dk, B):
    """One update against float64 with the float32 coefficient row the computation is defined with.  The bound, with u = 2^-24 and every
    operation rounded once (four roundings in a first-order step, six in a second-order one).  Each rounding errs by at most u times its
    result, and a result is at most the sum of the magnitudes of its terms -- the bound is stated in those, as test_constrain_kernel's
    2^-23 (|a target| + |s z|) is: A1 = |x| + |sg eps|, D1 = |x0| + |x0_prev|, DV = |x0| + |w| D1 (first order: |x0|), M = |c_D| DV.
      a1 = rn(x - sg eps), pre = rn(a1 inv_a):   |pre - exact| <= u (inv_a A1 + inv_a A1) =: e0; the clamp is 1-Lipschitz, so e0 bounds x0 too;
      d1 = rn(x0 - x0_prev), Dv = rn(w d1 + x0): |Dv - exact| <= u DV + |w| u D1 + (1 + |w|) e0 =: eD             (first order: eD = e0);
      m = rn(c_D Dv), out = rn(c_x x + m):       |out - exact| <= u (|c_x x| + M) + u M + |c_D| eD,
    evaluated on the float64 values (the second-order terms in u are covered by a factor 1 + 1e-5).  The cast of a coefficient to float32
    is a relative error of at most u in one of these same terms, which is why the bound is kept in this form for the second figure.
    Required: max |err| / bound <= 1, and <= 1.5 against the uncast float64 coefficients.  x0_out must hold the bits of the emulated clamped x0; the in-place form must give the
    same bits; the step to the clean level ignores the history."""
    n = 10
    e = HipEngine(obs_dim=Dk, action_dim=A, global_cond_dim=Dk, pred_horizon=T, action_horizon=AH)
    try:
        ts = e.set_solver_timesteps(S.solver_timesteps(N_TRAIN, n))
        rows32, rows64 = S.solver_coefficients(SCHED, ts), S.solver_coefficients(SCHED, ts, dtype=np.float64)
        g = rng(100 + Dk + B)
        for step in (0, 4, 9):
            k = rows32[step]
            x = g.standard_normal((B, T, Dk)).astype(np.float32)
            eps = g.standard_normal((B, T, Dk)).astype(np.float32)
            p = g.uniform(-1, 1, (B, T, Dk)).astype(np.float32)
            x[0, 0] = (np.float64(k[2]) * eps[0, 0] + 3.0 / np.float64(k[1])).astype(np.float32)       # x0 = +3 before the clip
            x[1, 1] = (np.float64(k[2]) * eps[1, 1] - 3.0 / np.float64(k[1])).astype(np.float32)       # x0 = -3
            for hist in (False, True):
                second = hist and step < n - 1
                got_x, got_x0 = e.plan_solver_step(_dev(x), _dev(eps), step, n, _dev(p) if hist else None)
                want, want_x0, bound = _exact_and_bound(x, eps, p, k, second)
                want64, _, _ = _exact_and_bound(x, eps, p, rows64[step], second)
                gx = got_x.cpu().numpy().astype(np.float64)
                ratio = float((np.abs(gx - want) / bound).max())
                ratio64 = float((np.abs(gx - want64) / bound).max())
                print(f"solver D = {Dk} B = {B} step {step} history {hist}: max |err| / bound = {ratio:.3f} (uncast coefficients: {ratio64:.3f})")
                assert np.isfinite(gx).all() and ratio <= 1.0 and ratio64 <= 1.5
                em_x, em_x0 = _emulate(x, eps, p, k, second)
                assert np.array_equal(_bits(got_x0), em_x0.view(np.uint32))
                assert float(got_x0[0, 0].min()) == 1.0 and float(got_x0[1, 1].max()) == -1.0 and float(got_x0.abs().max()) <= 1.0
                # in place: x_out = x, x0_out = x0_prev
                xi, pi = _dev(x), _dev(p)
                if hist:
                    rx, r0 = e.plan_solver_step(xi, _dev(eps), step, n, pi, inplace=True)
                    assert rx.data_ptr() == xi.data_ptr() and r0.data_ptr() == pi.data_ptr()
                    assert _same(rx, got_x) and _same(r0, got_x0)
                if step == n - 1 and hist:
                    nx, n0 = e.plan_solver_step(_dev(x), _dev(eps), step, n, None)
                    assert _same(nx, got_x) and _same(n0, got_x0)
        with pytest.raises(LDPHipError, match="step") as ei:
            e.plan_solver_step(_dev(x), _dev(eps), n, n)
        assert ei.value.code == EINVAL
        e.check_fault()
    finally:
        e.close()


# ---- 2. second order on the device ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 10, 20])
def test_second_order_on_the_device(eng, n):
    """plan_solver_step driven with the analytic eps-model of data N(0, 0.3^2) (its factor per timestep from the host, the product in torch
    on the device): the result is within 0.25 x the oracle's DDIM error (same grid) of the closed-form solution, and within 1e-5 relative
    RMS of the float64 solver."""
    s = 0.3
    ts = eng.set_solver_timesteps(S.solver_timesteps(N_TRAIN, n))
    alpha, sigma, _ = SO.levels(N_TRAIN)
    x_t = rng(0).uniform(-2.0, 2.0, (3, T, D)).astype(np.float32)
    x, hist = _dev(x_t), None
    for i, t in enumerate(ts):
        eps = x * float(sigma[t] / (alpha[t] ** 2 * s * s + sigma[t] ** 2))
        x, hist = eng.plan_solver_step(x, eps, i, n, hist)
    got = x.cpu().numpy()
    exact = SO.gaussian_exact(x_t, int(ts[0]), s)
    ddim, two_m = SO.gaussian_errors(ts, s, x_t)
    err, dev64 = SO.rel_rms(got, exact), SO.rel_rms(got, SO.solve(SO.gaussian_eps(s), x_t, ts))
    print(f"n = {n}: device 2M error {err:.5f} (oracle 2M {two_m:.5f}, oracle DDIM {ddim:.5f}); against the float64 solver {dev64:.2e}")
    assert err <= 0.25 * ddim and dev64 <= 1e-5


# ---- 3. the loop is the composition ---------------------------------------------------------------------------------------------------------
def _by_hand(eng, cond, x, ts, begin=0, end=None):
    hist = None
    for i in range(begin, len(ts) if end is None else end):
        x, hist = eng.plan_solver_step(x, eng.unet_forward(x, int(ts[i]), cond), i, len(ts), hist)
    return x


@pytest.mark.parametrize("B", [3, 17])
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_loop_is_the_composition(eng, use_graph, B):
    n = 5
    ts = eng.set_solver_timesteps(S.solver_timesteps(N_TRAIN, n))
    cond = _cond(B)
    kw = dict(seed=99, row_offset=11, n_steps=n)
    fused = eng.plan_sample(cond, sampler="dpmpp", use_graph=use_graph, **kw)
    x_t = eng.plan_sample_range(cond, 0, 0, sampler="dpmpp", **kw)             # the drawn initial state
    assert _same(x_t, eng.plan_sample_range(cond, 0, 0, sampler="ddim", **kw))
    x = _by_hand(eng, cond, x_t, ts)
    assert torch.isfinite(fused).all() and _same(fused, x), f"max |diff| = {float((fused - x).abs().max()):.3e}"


# ---- 4. the loop against float64 ------------------------------------------------------------------------------------------------------------
_ref = {}


def _reference_17():
    """One float64 loop of 17 rows, shared: rows are independent, so its first three rows are the B = 3 reference."""
    if not _ref:
        g = rng(700)
        _ref["cond"] = g.uniform(-1, 1, (17, D)).astype(np.float32)
        _ref["x_init"] = g.standard_normal((17, T, D)).astype(np.float32)
        _ref["ts"] = S.solver_timesteps(N_TRAIN, 10)
        _ref["out"] = SO.planner_solver(np64.to64(planner_params(D=D)), _ref["cond"].astype(np.float64), _ref["x_init"], _ref["ts"])
    return _ref


@pytest.mark.parametrize("B", [3, 17])
def test_loop_against_float64(eng, B):
    r = _reference_17()
    n = 10
    eng.set_solver_timesteps(r["ts"])
    cond, x_init = _dev(r["cond"][:B]), _dev(r["x_init"][:B])
    kw = dict(sampler="dpmpp", n_steps=n, row_offset=4)
    eager = eng.plan_sample(cond, x_init=x_init, seed=1, use_graph=False, **kw)
    assert_close(eager.cpu().numpy(), r["out"][:B], 1e-4, f"dpmpp-10 B = {B}")
    first = eng.plan_sample(cond, x_init=x_init, seed=1, use_graph=True, **kw)
    replay = eng.plan_sample(cond, x_init=x_init, seed=1, use_graph=True, **kw)
    assert _same(first, eager) and _same(replay, eager)
    # a drawn x_T: the seed reaches a replayed graph
    a = eng.plan_sample(cond, seed=1, use_graph=True, **kw)
    b = eng.plan_sample(cond, seed=2, use_graph=True, **kw)
    c = eng.plan_sample(cond, seed=1, use_graph=True, **kw)
    assert not _same(a, b) and _same(a, c) and _same(a, eng.plan_sample(cond, seed=1, use_graph=False, **kw))
    if B == 17:
        # A row does not depend on the batch around it.  Bit for bit inside one launch regime: the 17 rows inside a call of 20 (both run
        # two 16-row tiles).  Against the B = 3 call only to round-off: a U-Net evaluation over one tile splits K over more work-groups
        # than one over two tiles (engine.hpp bucket_rows: "a row's bits depend on its 16-bucket"), under every sampler -- the DDIM
        # figure is printed next to this sampler's (measured on one MI355X: 1.9e-6 here, 4.3e-6 for DDIM-10).  Both calls are within 1e-4
        # of the same float64 rows, hence within 2e-4 of each other.
        c20 = _dev(np.concatenate([r["cond"], r["cond"][:3]]))
        x20 = _dev(np.concatenate([r["x_init"], r["x_init"][:3]]))
        big = eng.plan_sample(c20, x_init=x20, seed=1, **kw)
        assert _same(big[:17], eager)
        assert _same(eng.plan_sample(c20, seed=1, **kw)[:17], a)
        c3, x3 = cond[:3].contiguous(), x_init[:3].contiguous()
        small = eng.plan_sample(c3, x_init=x3, seed=1, **kw)
        dk = dict(kw, sampler="ddim")
        d_ddim = float((eng.plan_sample(cond, x_init=x_init, **dk)[:3] - eng.plan_sample(c3, x_init=x3, **dk)).abs().max())
        d = float((eager[:3] - small).abs().max())
        d_drawn = float((a[:3] - eng.plan_sample(c3, seed=1, **kw)).abs().max())
        print(f"rows 0..2 of B = 17 against the B = 3 call: max |diff| {d:.2e} (drawn x_T: {d_drawn:.2e}; DDIM-10: {d_ddim:.2e})")
        assert_close(small.cpu().numpy(), r["out"][:3], 1e-4, "dpmpp-10 B = 3 rows")
        assert d <= 2e-4
        rk = dict(seed=1, **kw)                                                # the drawn x_T itself is keyed by the global row: its bits agree
        assert _same(eng.plan_sample_range(cond, 0, 0, **rk)[:3], eng.plan_sample_range(c3, 0, 0, **rk))


# ---- 5. a batch that the engine splits --------------------------------------------------------------------------------------------------------
def test_split_batch(eng):
    B, b1, off, n = 1040, 1024, 7, 5
    eng.set_solver_timesteps(S.solver_timesteps(N_TRAIN, n))
    g = rng(1000)
    cond = _dev(g.uniform(-1, 1, (B, D)))
    x_init = _dev(g.standard_normal((B, T, D)))
    kw = dict(sampler="dpmpp", n_steps=n, seed=21)
    whole = eng.plan_sample(cond, x_init=x_init, row_offset=off, **kw)
    conv_whole, all_whole = eng.launch_counts()
    first = eng.plan_sample(cond[:b1].contiguous(), x_init=x_init[:b1].contiguous(), row_offset=off, **kw)
    conv1, all1 = eng.launch_counts()
    second = eng.plan_sample(cond[b1:].contiguous(), x_init=x_init[b1:].contiguous(), row_offset=off + b1, **kw)
    conv2, all2 = eng.launch_counts()
    assert torch.isfinite(whole).all() and _same(whole[:b1], first) and _same(whole[b1:], second)
    assert conv1 > 0 and conv_whole == conv1 + conv2 and all_whole == all1 + all2
    eng.check_fault()


# ---- 6. table handling -------------------------------------------------------------------------------------------------------------------------
def test_table_handling(eng):
    B, n = 3, 5
    cond = _cond(B)
    x0 = _dev(rng(3).standard_normal((B, T, D)))
    # no table: LDP_ESTATE (the Python wrapper would register one, so it is told that it holds one)
    eng.solver_tables[7] = None
    try:
        with pytest.raises(LDPHipError, match="ldp_solver_timesteps") as ei:
            eng.plan_sample(cond, sampler="dpmpp", n_steps=7)
        assert ei.value.code == ESTATE
        with pytest.raises(LDPHipError, match="ldp_solver_timesteps") as ei:
            eng.plan_solver_step(x0, x0, 0, 7)
        assert ei.value.code == ESTATE
    finally:
        del eng.solver_tables[7]
    for bad, word in (([5, 5, 0], r"ts\[1\]"), ([5, 6, 0], r"ts\[1\]"), ([5, 3, 1], r"ts\[2\]"), ([100, 0], r"ts\[0\]"), ([3, -1], r"ts\[1\]"),
                      ([], "n_steps"), (list(range(100, -1, -1)), "n_steps")):
        with pytest.raises(LDPHipError, match=word) as ei:
            eng.set_solver_timesteps(bad)
        assert ei.value.code == EINVAL, bad
    ts_a, ts_b = S.solver_timesteps(N_TRAIN, n), S.solver_timesteps(N_TRAIN, n, "uniform")
    eng.set_solver_timesteps(ts_a)
    kw = dict(sampler="dpmpp", n_steps=n, x_init=x0)
    out_a = eng.plan_sample(cond, **kw)
    captured = eng.get_option("graphs_captured")
    eng.set_solver_timesteps(ts_a)                                             # the same table again: nothing happens
    assert _same(eng.plan_sample(cond, **kw), out_a) and eng.get_option("graphs_captured") == captured
    eng.set_solver_timesteps(ts_b)                                             # another one: the graphs go, the results follow it
    out_b = eng.plan_sample(cond, **kw)
    assert eng.get_option("graphs_captured") == captured + 1
    assert not _same(out_b, out_a) and _same(out_b, _by_hand(eng, cond, x0, ts_b))
    assert _same(out_b, eng.plan_sample(cond, use_graph=False, **kw))
    # a range that starts at begin > 0 starts first order, and ranges therefore do not compose bit for bit
    eng.set_solver_timesteps(ts_a)
    for use_graph in (False, True):
        one = eng.plan_sample_range(cond, 2, 3, use_graph=use_graph, **kw)
        assert _same(one, _by_hand(eng, cond, x0, ts_a, 2, 3))
    head = eng.plan_sample_range(cond, 0, 2, **kw)
    tail = eng.plan_sample_range(cond, 2, n, **dict(kw, x_init=head))
    assert _same(tail, _by_hand(eng, cond, head, ts_a, 2, n)) and not _same(tail, out_a)
    # entry points the sampler is not built for: LDP_EINVAL
    tg, mk = torch.zeros(B, T, D, device="cuda"), torch.zeros(B, T, D, dtype=torch.uint8, device="cuda")
    obs_emb = cond[:, None].contiguous()
    store = torch.zeros(B, T, D, device="cuda")
    skw = dict(sampler="dpmpp", n_steps=n)
    jkw = dict(sampler="dpmpp", planner_steps=n, idm_steps=n)
    for call in (lambda: eng.idm_sample(torch.zeros(B * AH, 2 * D, device="cuda"), **skw),
                 lambda: eng.plan_warm_init(store, 2, **skw),
                 lambda: eng.agent_resample(obs_emb, 1, store, 2, **jkw),
                 lambda: eng.plan_constrain(x0, tg, mk, 0, **skw),
                 lambda: eng.plan_sample_constrained(cond, tg, mk, **skw),
                 lambda: eng.agent_sample_constrained(obs_emb, 1, tg, mk, **jkw)):
        with pytest.raises(LDPHipError, match="not built") as ei:
            call()
        assert ei.value.code == EINVAL
    assert torch.isfinite(eng.plan_sample(cond, **kw)).all()                   # nothing above left the engine in a bad state
    eng.check_fault()


# ---- 7. agents ------------------------------------------------------------------------------------------------------------------------------------
def test_ldp_agent():
    from latent_diffusion_planning_amd.agent import _seed_of
    ag, data = make_agent("rm", planner_params(), idm_params())
    try:
        eng = ag._engine
        B, n, rng_key = 3, 10, 8
        batch = cfgs.synth_latent_batch(data, B, 1, 2)
        oh = ag.config["obs_horizon"]
        action, m = ag.sample(batch, rng_key, sampler="dpmpp", n_steps=n)      # (the parent commit: KeyError 'dpmpp')
        conv_s, all_s = eng.launch_counts()
        assert eng.solver_tables[n].tolist() == S.solver_timesteps(N_TRAIN, n).tolist()
        obs_emb = ag.get_obs_cond(ag._vae_encode_t(ag._postprocess(batch)["obs"])).contiguous()
        plan = m["plan"].tensor
        assert tuple(plan.shape) == (B, AH + 1, D) and _same(plan[:, 0], obs_emb[:, oh - 1])
        lo, hi, mode = ag._action_bounds()
        seed = _seed_of(rng_key)
        x, plan2, act2 = eng.agent_sample(obs_emb, oh, seed=seed, sampler="dpmpp", planner_steps=n, idm_steps=n, action_bounds=(lo, hi),
                                          action_mode=mode)
        assert _same(action.tensor, act2) and _same(plan, plan2) and _same(plan[:, 1:], x[:, :AH])
        # the planner part against float64, from the x_T the call drew
        cond = obs_emb[:, :oh].reshape(B, -1).contiguous()
        x_t = eng.plan_sample_range(cond, 0, 0, seed=seed, sampler="dpmpp", n_steps=n)
        ref = SO.planner_solver(np64.to64(planner_params()), cond.cpu().numpy().astype(np.float64), x_t.cpu().numpy(), eng.solver_tables[n])
        assert_close(x.cpu().numpy(), ref, 1e-4, "LDPAgent.sample dpmpp-10: planner state")
        # the IDM loop is DDIM-10 on that plan
        tr = torch.cat([plan[:, :-1], plan[:, 1:]], dim=-1).reshape(B * AH, 2 * D).contiguous()
        a = eng.idm_sample(tr, seed=seed, sampler="ddim", n_steps=n).reshape(B, AH, A)
        norm = eng.agent_sample(obs_emb, oh, seed=seed, sampler="dpmpp", planner_steps=n, idm_steps=n)[2]
        assert _same(norm, a)
        # ten evaluations plus ten solver launches: DDIM-10's launches and ten more
        ag.sample(batch, rng_key, sampler="ddim", n_steps=n)
        conv_d, all_d = eng.launch_counts()
        assert conv_s == conv_d > 0 and all_s == all_d + n, (conv_s, conv_d, all_s, all_d)
        # timesteps=: a named grid, a sequence; a wrong length and idm_steps that do not divide the IDM's training steps are refused
        uni = ag.sample(batch, rng_key, sampler="dpmpp", n_steps=n, timesteps="uniform")[1]["plan"].tensor
        assert eng.solver_tables[n].tolist() == S.solver_timesteps(N_TRAIN, n, "uniform").tolist() and not _same(uni, plan)
        seq = ag.sample(batch, rng_key, sampler="dpmpp", n_steps=n, timesteps=S.solver_timesteps(N_TRAIN, n).tolist())[1]["plan"].tensor
        assert _same(seq, plan)
        with pytest.raises(ValueError, match="n_steps"):
            ag.sample(batch, rng_key, sampler="dpmpp", n_steps=n, timesteps=[3, 2, 0])
        with pytest.raises(ValueError, match="idm_steps"):
            ag.sample(batch, rng_key, sampler="dpmpp", n_steps=7)
        assert np.isfinite(np.array(ag.get_action(batch, rng_key, sampler="dpmpp", n_steps=7, idm_steps=10))).all()
        # best of N: candidate 0 of a one-observation call is sample()'s row
        one = cfgs.synth_latent_batch(data, 1, 1, 2)
        _, m1 = ag.sample(one, rng_key, sampler="dpmpp", n_steps=n)
        _, mb = ag.sample_best_of(one, rng_key, 4, sampler="dpmpp", n_steps=n)
        cand = mb["candidates"].tensor
        assert tuple(cand.shape) == (1, 4, T, D) and _same(cand[0, 0, :AH], m1["plan"].tensor[0, 1:])
        # not built
        with pytest.raises(NotImplementedError, match="dpmpp"):
            ag.sample_warm(batch, rng_key, None, None, sampler="dpmpp", n_steps=n)
        with pytest.raises(NotImplementedError, match="dpmpp"):
            ag.sample_constrained(batch, rng_key, sampler="dpmpp", n_steps=n)
        with pytest.raises(NotImplementedError, match="dpmpp"):
            ag.replanner(4, 2, sampler="dpmpp", n_steps=n)
        eng.check_fault()
    finally:
        ag._engine.close()


def test_dp_vae_agent():
    from latent_diffusion_planning_amd.dp_vae_agent import DPVAEAgent
    from tests import dp_oracle
    from tests.golden.make_golden_dp import AH as DAH, OH, T as DT
    data = cfgs.BY_NAME["rm"]
    ag = DPVAEAgent.create(0, None, data["shape_meta"], **dp_oracle.dp_kwargs(data, OH, DT, DAH))
    try:
        batch = cfgs.synth_latent_batch(data, 5, OH, 11)
        act, extra = ag.sample(batch, 7, sampler="dpmpp", n_steps=10)
        eng = ag._engine
        emb = ag._frame_emb(ag._vae_encode_t(ag._postprocess(batch)["obs"]))
        from latent_diffusion_planning_amd.agent import _seed_of
        lo, hi, mode = ag._action_bounds()
        want = eng.policy_sample(emb, OH, ag.config["vae_feature_dim"], seed=_seed_of(7), sampler="dpmpp", n_steps=10, action_bounds=(lo, hi),
                                 action_mode=mode)
        assert extra == {} and _same(act.tensor, want) and torch.isfinite(want).all()
        ddim = eng.policy_sample(emb, OH, ag.config["vae_feature_dim"], seed=_seed_of(7), sampler="ddim", n_steps=10, action_bounds=(lo, hi),
                                 action_mode=mode)
        assert not _same(want, ddim)
        eng.check_fault()
    finally:
        ag._engine.close()
