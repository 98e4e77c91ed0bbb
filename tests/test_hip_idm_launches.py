"""Every fused IDM launch against float64, in each kernel it can run (csrc/idm.hip; cases, inputs and the dispatch rule:
tests/idm_launch_cases.py).  -m gpu.

Which instantiation a call ran is read from the handle's launch counters (`stat_idm_*`) before and after the eager call: exactly
the expected counter moves, by the expected number of launches.  The rule is the planner suite's (planner_stage_cases.stage_error):
|got - ref64| <= max(1e-5, 3 err32) max(1, max|ref64|) with err32 the error of the float32 evaluation of the same function (for loops: of the
float32 loop) on the same rows; rows never couple (LayerNorm is per row), so the references are computed on the rows of
planner_stage_cases.ref_rows only.  The references run on the device's own time-embedding frequencies (torch32 exact_freqs: exp rounded to
float32 once, what libm's expf fills the device's table with): the float32 exp of the goldens' oracle is an ulp off in up to 59 of 128
entries, by library and machine, which moves k f by up to 7.6e-6 and a DDIM-5 action by 1.2e-5 -- more than the whole bound.  Measured
figures per instantiation: DESIGN 4.2."""
import contextlib

import pytest
import torch

from oracle import torch32
from tests import idm_launch_cases as LC
from tests.util import idm_params, idm_params_heavy, planner_params

pytestmark = pytest.mark.gpu

_engines, _params, _refs = {}, {}, {}


def _ip(config):
    D, A, heavy = LC.CONFIGS[config]
    return (idm_params_heavy if heavy else idm_params)(D=D, A=A)


def _new_engine(config):
    from latent_diffusion_planning_amd.engine import HipEngine
    D, A, _ = LC.CONFIGS[config]
    e = HipEngine(obs_dim=D, action_dim=A, global_cond_dim=D, pred_horizon=8, action_horizon=4)
    e.load_params(planner=planner_params(D=D), idm=_ip(config))
    return e


@pytest.fixture(scope="module")
def engines():
    """One engine per configuration, created at its first use, closed with the module."""
    def get(config):
        if config not in _engines:
            _engines[config] = _new_engine(config)
        return _engines[config]
    yield get
    for e in _engines.values():
        e.close()
    _engines.clear()
    _refs.clear()


@contextlib.contextmanager
def options(eng, opts):
    try:
        for k, v in opts.items():
            eng.set_option(k, v)
        yield
    finally:
        for k in opts:
            eng.set_option(k, LC.DEFAULTS[k])


def counters(eng):
    return {n: eng.get_option(n) for n in LC.COUNTERS}


def moved(before, after):
    return {n: after[n] - before[n] for n in LC.COUNTERS if after[n] != before[n]}


def clean(eng):
    torch.cuda.synchronize()
    assert eng.poll_fault_kinds() == 0 and eng.get_option("range_fallback") == 0


def reference(config, R, what, n_steps=0):
    """(rows, ref64, ref32) of one call on the reference rows of an R-row batch, computed once per (config, R, call)."""
    key = (config, R, what, n_steps)
    if key not in _refs:
        rows = LC.ref_rows(R)
        s, a, k, nz = LC.inputs(config, R, steps=100 if what == "ddpm" else 0)
        s, a, k, nz = s[rows], a[rows], k[rows], nz[:, rows]
        out = []
        for dt in (torch.float64, torch.float32):
            if (config, dt) not in _params:
                _params[(config, dt)] = torch32.TorchParams(_ip(config), dtype=dt)
            P = _params[(config, dt)]
            with torch.no_grad():
                if what == "forward_k":
                    out.append(torch32.idm_forward(P, s.to(dt), a.to(dt), 63, exact_freqs=True))
                elif what == "forward_rows":
                    out.append(torch32.idm_forward(P, s.to(dt), a.to(dt), k, exact_freqs=True))
                elif what == "ddim":
                    out.append(torch32.idm_sample(P, s.to(dt), a.to(dt), None, n_steps=n_steps, sampler="ddim", exact_freqs=True))
                else:
                    out.append(torch32.idm_sample(P, s.to(dt), a.to(dt), nz.to(dt), n_steps=100, sampler="ddpm", exact_freqs=True))
        _refs[key] = (rows, out[0], out[1])
    return _refs[key]


def check(got, config, R, what, n_steps=0, label=""):
    rows, ref64, ref32 = reference(config, R, what, n_steps)
    e = LC.stage_error(got[rows].cpu(), ref64, ref32)
    print(f"IDMERR {label} {what}{n_steps or ''} err={e['err']:.3e} err32={e['err32']:.3e} bound={e['bound']:.3e} row={rows[e['row']]}")
    assert e["ok"], f"{label} {what}{n_steps or ''}: err {e['err']:.3e} > bound {e['bound']:.3e} (err32 {e['err32']:.3e}) at row {rows[e['row']]}"


def attested(eng, kind, R, opts, call, n_steps=0, explicit_noise=False):
    """Run `call` eagerly and assert that exactly the expected counter moved, by the expected number of launches."""
    want = LC.expected_counts(kind, R, opts, eng.get_option("n_cu"), bool(eng.get_option("range_fallback")), n_steps, explicit_noise)
    c0 = counters(eng)
    got = call()
    m = moved(c0, counters(eng))
    assert m == want, f"{kind} R={R} {opts}: launches {m}, expected {want}"
    return got, next(iter(want))


# ---- a. one evaluation: IF_IN, IF_RED x 2, tail + IF_EPSOUT ---------------------------------------------------------------------------------
@pytest.mark.parametrize("c", LC.CASES, ids=LC.case_id)
def test_one_evaluation(engines, c):
    config, R, opts = c[0], c[1], dict(c[2])
    eng = engines(config)
    s, a, k, _ = LC.inputs(config, R)
    s, a = s.cuda(), a.cuda()
    with options(eng, opts):
        got, name = attested(eng, "forward", R, opts, lambda: eng.idm_forward(s, a, 63))
        check(got, config, R, "forward_k", label=f"{LC.case_id(c)} {name}")
        got, name = attested(eng, "forward", R, opts, lambda: eng.idm_forward(s, a, k))
        check(got, config, R, "forward_rows", label=f"{LC.case_id(c)} {name}")
        clean(eng)


# ---- b. the fused step: IF_IN | IF_TAIL | IF_STEP, and the final tail ----------------------------------------------------------------------
@pytest.mark.parametrize("c", LC.CASES, ids=LC.case_id)
def test_ddim_loops(engines, c):
    """n_steps 1, 2, 5: the loop without a fused scheduler update and both parities of the state ping-pong (the result is read from the
    buffer the last tail wrote: state_cur = n_steps & 1).  The eager loop attests its counter; the captured one equals it bit for bit."""
    config, R, opts = c[0], c[1], dict(c[2])
    eng = engines(config)
    s, a, _, _ = LC.inputs(config, R)
    s, a = s.cuda(), a.cuda()
    with options(eng, opts):
        for n in LC.DDIM_STEPS:
            got, name = attested(eng, "sample", R, opts, lambda: eng.idm_sample(s, a_init=a, sampler="ddim", n_steps=n, use_graph=False), n_steps=n)
            graph = eng.idm_sample(s, a_init=a, sampler="ddim", n_steps=n, use_graph=True)
            assert torch.equal(graph, got), f"{LC.case_id(c)} DDIM-{n}: captured loop differs from the eager one"
            assert torch.equal(eng.idm_sample(s, a_init=a, sampler="ddim", n_steps=n, use_graph=True), got), f"{LC.case_id(c)} DDIM-{n}: replay differs"
            check(got, config, R, "ddim", n, label=f"{LC.case_id(c)} {name}")
        clean(eng)


@pytest.mark.parametrize("c", LC.DDPM_CASES, ids=LC.case_id)
def test_ddpm_loop_with_explicit_noise(engines, c):
    config, R, opts = c[0], c[1], dict(c[2])
    eng = engines(config)
    s, a, _, nz = LC.inputs(config, R, steps=100)
    s, a, nz = s.cuda(), a.cuda(), nz.cuda()
    with options(eng, opts):
        got, name = attested(eng, "sample", R, opts, lambda: eng.idm_sample(s, a_init=a, step_noise=nz, sampler="ddpm", n_steps=100, use_graph=False),
                             n_steps=100, explicit_noise=True)
        assert torch.equal(eng.idm_sample(s, a_init=a, step_noise=nz, sampler="ddpm", n_steps=100, use_graph=True), got)
        check(got, config, R, "ddpm", label=f"{LC.case_id(c)} {name}")
        clean(eng)


# ---- c. Philox ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_offset", [0, 1000])
@pytest.mark.parametrize("c", LC.DDPM_CASES, ids=LC.case_id)
def test_philox_key_of_the_in_kernel_noise(engines, c, row_offset):
    """The noise a DDPM loop draws inside the block kernels (idm.hip, the IF_STEP prologue; idm_pre): philox_normal at key = seed with the top
    bit flipped (seed ^ 2^63), element (row_offset + row) * AP + column with AP = 32 padded action columns, counter word 2 = the index of
    the executed step, stream 0; the initial a_T is the same key and element at step 0 of stream 1.  The loop given exactly those draws as
    explicit a_init / step_noise equals the in-kernel one bit for bit (the last step, t = 0, draws nothing: sigma = 0)."""
    from latent_diffusion_planning_amd.engine import philox_normal
    config, R, opts = c[0], c[1], dict(c[2])
    A, seed, key = LC.CONFIGS[config][1], 12345, 12345 ^ (1 << 63)
    eng = engines(config)
    s = LC.inputs(config, R)[0].cuda()

    def draws(step, stream):
        return philox_normal(key, row_offset * LC.AP, step, stream, R * LC.AP).reshape(R, LC.AP)[:, :A].contiguous()
    with options(eng, opts):
        inside, _ = attested(eng, "sample", R, opts, lambda: eng.idm_sample(s, seed=seed, row_offset=row_offset, sampler="ddpm", n_steps=100, use_graph=False),
                             n_steps=100)
        a_T, nz = draws(0, 1), torch.stack([draws(i, 0) for i in range(100)])
        given = eng.idm_sample(s, a_init=a_T, step_noise=nz, row_offset=row_offset, sampler="ddpm", n_steps=100, use_graph=False)
        assert torch.equal(inside, given), f"{LC.case_id(c)} row_offset {row_offset}: {int((inside != given).any(dim=1).sum())} of {R} rows differ"
        assert torch.isfinite(inside).all() and not torch.equal(inside,eng.idm_sample(s, seed=seed + 1, row_offset=row_offset, sampler="ddpm", n_steps=100))
        clean(eng)


# ---- the ringed variant streams the same fragments in the same order ------------------------------------------------------------------------------
@pytest.mark.parametrize("c", LC.RINGED_CASES + [x for x in LC.ALOHA_CASES if x[1] == 250 and dict(x[2]).get("idm_hs")], ids=LC.case_id)
def test_ringed_equals_plain_bit_for_bit(engines, c):
    config, R, opts = c[0], c[1], dict(c[2])
    eng = engines(config)
    s, a, k, _ = LC.inputs(config, R)
    s, a = s.cuda(), a.cuda()
    outs = []
    for o in (opts, dict(opts, idm_noring=1)):
        with options(eng, o):
            fwd, name = attested(eng, "forward", R, o, lambda: eng.idm_forward(s, a, k))
            loop, _ = attested(eng, "sample", R, o, lambda: eng.idm_sample(s, a_init=a, sampler="ddim", n_steps=5, use_graph=False), n_steps=5)
            outs.append((name, fwd, loop))
    assert "_ring" in outs[0][0] and outs[1][0] == outs[0][0].replace("_ring", "")
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2])
    clean(eng)


# ---- d. rows do not depend on the batch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config,R,Rs,opts", LC.SUBBATCH, ids=lambda v: str(v).replace(" ", ""))
def test_rows_do_not_depend_on_the_batch(engines, config, R, Rs, opts):
    eng = engines(config)
    s, a, k, _ = LC.inputs(config, R)
    s, a = s.cuda(), a.cuda()
    with options(eng, opts):
        big, nb = attested(eng, "forward", R, opts, lambda: eng.idm_forward(s, a, k))
        small, ns = attested(eng, "forward", Rs, opts, lambda: eng.idm_forward(s[:Rs], a[:Rs], k[:Rs]))
        assert nb.replace("_ring", "") == ns.replace("_ring", "")
        assert torch.equal(big[:Rs], small), f"one evaluation: {int((big[:Rs] != small).any(dim=1).sum())} rows differ"
        big = eng.idm_sample(s, a_init=a, sampler="ddim", n_steps=5, use_graph=False)
        small = eng.idm_sample(s[:Rs], a_init=a[:Rs], sampler="ddim", n_steps=5, use_graph=False)
        assert torch.equal(big[:Rs], small), f"DDIM-5: {int((big[:Rs] != small).any(dim=1).sum())} rows differ"
        clean(eng)


# ---- e. workspace stride -------------------------------------------------------------------------------------------------------------------
def test_a_grown_workspace_changes_no_bit():
    """The partials are indexed with Rp = ws_R, which only grows: an R = 37 call runs with Rp = 64 on a fresh handle and with Rp = 320 after
    an R = 300 call."""
    config = "rm"
    eng = _new_engine(config)
    try:
        s, a, k, _ = LC.inputs(config, 300)
        s, a = s.cuda(), a.cuda()

        def run():
            out = []
            for cfg, opts in LC.STRIDE:
                assert cfg == config
                with options(eng, opts):
                    fwd, name = attested(eng, "forward", 37, opts, lambda: eng.idm_forward(s[:37], a[:37], k[:37]))
                    out += [fwd, eng.idm_sample(s[:37], a_init=a[:37], sampler="ddim", n_steps=5, use_graph=False),
                            eng.idm_sample(s[:37], a_init=a[:37], sampler="ddim", n_steps=5, use_graph=True)]
                    check(fwd, config, 37, "forward_rows", label=f"stride {name}")
            return out
        fresh = run()
        eng.idm_forward(s, a, k)
        grown = run()
        assert all(torch.equal(x, y) for x, y in zip(fresh, grown)), [bool(torch.equal(x, y)) for x, y in zip(fresh, grown)]
        clean(eng)
    finally:
        eng.close()


# ---- f. placement ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", LC.PLACEMENT, ids=LC.case_id)
def test_slice_major_placement_changes_no_bit(engines, c):
    config, R, opts = c[0], c[1], dict(c[2])
    eng = engines(config)
    s, a, k, _ = LC.inputs(config, R)
    s, a = s.cuda(), a.cuda()
    outs = []
    for o in (opts, dict(opts, idm_rt_major=0)):
        with options(eng, o):
            fwd, name = attested(eng, "forward", R, o, lambda: eng.idm_forward(s, a, k))
            outs.append((name, fwd, eng.idm_sample(s, a_init=a, sampler="ddim", n_steps=2, use_graph=False)))
    assert outs[0][0] == outs[1][0] and torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2])
    check(outs[1][1], config, R, "forward_rows", label=f"{LC.case_id(c)} rt_major=0 {outs[1][0]}")
    clean(eng)


# ---- g. the fallback path -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", LC.FALLBACK, ids=LC.case_id)
def test_fallback_kernels_at_the_rows_that_select_them(engines, c):
    """What a handle runs at large batches once the fp16-plane kernel is off (idm_f16 = 0, or for good after a range fault): the 16-row kernel
    with the split of the default rule, in the instantiation that has the non-temporal path only (from 128 row tiles)."""
    config, R, opts = c[0], c[1], dict(c[2])
    eng = engines(config)
    s, a, k, _ = LC.inputs(config, R)
    s, a = s.cuda(), a.cuda()
    with options(eng, opts):
        got, name = attested(eng, "forward", R, opts, lambda: eng.idm_forward(s, a, k))
        assert name.endswith("_nt") and "_ring" not in name
        check(got, config, R, "forward_rows", label=f"{LC.case_id(c)} {name}")
        clean(eng)
    if R == 2048:                                     # the same kernel through the sticky fallback itself
        try:
            eng.set_option("range_fallback", 1)
            c0 = counters(eng)
            again = eng.idm_forward(s, a, k)
            assert moved(c0, counters(eng)) == {name: LC.NB + 1} == LC.expected_counts("forward", R, {}, eng.get_option("n_cu"), True)
            assert torch.equal(again, got)
        finally:
            eng.set_option("range_fallback", 0)
        clean(eng)


def test_counters_are_read_only(engines):
    from latent_diffusion_planning_amd._lib import LDPHipError
    eng = engines("rm")
    for n in LC.COUNTERS:
        with pytest.raises(LDPHipError):
            eng.set_option(n, 0)
    for n in ("stat_idm_f32_hs2_ring", "stat_idm_f32_hs3", "stat_idm_f16_hs8", "stat_idm_"):
        with pytest.raises(LDPHipError):
            eng.get_option(n)
