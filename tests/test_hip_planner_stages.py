"""Every launch of the planner U-Net on its own against float64, on the tile it really runs.  -m gpu.

`HipEngine.unet_trace` (ldp_unet_trace) runs the code of unet_forward and copies what every launch wrote out behind the launch.  For stage k the
float64 stage function of oracle/torch32.py (`unet_stages`) is applied to the GPU's OWN tapped inputs of that stage, so nothing is inherited
from earlier stages, and the bound is the project's rule:

    |got - ref64| <= max(1e-5, 3 * err32) * max(1, max|ref64|)

with err32 the error of the float32 evaluation of the same stage function on the same input (tests/planner_stage_cases.stage_error: the
function tests/test_planner_stages_cpu.py shows able to fail).  Samples never couple, so the reference runs on at most 48 rows of a batch
(`ref_rows`); every tap is checked finite, and its padding zero, over all rows.  The trace table says which plan every stage ran on;
`expected_dispatch` states the regime rule of INTEGRATION 2 / DESIGN 4.5 / 4.7 and every table is held against it; the plans the cases reach
are held against tests/planner_stage_coverage.py.

Measured on the MI355X (worst err / bound per arithmetic form and stage kind): DESIGN.md 4.7.2.
"""
import pytest
import torch

from latent_diffusion_planning_amd import weights as W
from oracle import torch32
from tests import planner_stage_cases as PC
from tests.planner_stage_coverage import COVERAGE, REACHED
from tests.util import planner_params_heavy

pytestmark = pytest.mark.gpu

_engines, _params, _reached, _worst = {}, {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


def _model_params(model):
    if model not in _params:
        D, G, T, dims, heavy = PC.MODELS[model]
        pp = planner_params_heavy(D=D) if heavy else W.init_planner_params(W.PlannerSpec(D, G, down_dims=dims), 0)
        _params[model] = (pp, torch32.TorchParams(pp, dtype=torch.float64), torch32.TorchParams(pp, dtype=torch.float32))
    return _params[model]


def _engine(model):
    if model not in _engines:
        from latent_diffusion_planning_amd.engine import HipEngine
        D, G, T, dims, _ = PC.MODELS[model]
        e = HipEngine(obs_dim=D, action_dim=7, global_cond_dim=G, pred_horizon=T, action_horizon=min(4, T), down_dims=list(dims))
        e.load_params(planner=_model_params(model)[0])
        _engines[model] = e
    return _engines[model]


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


class _Options:
    def __init__(self, eng, opts):
        self.eng, self.opts = eng, dict(opts)

    def __enter__(self):
        for k, v in self.opts.items():
            self.eng.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            self.eng.set_option(k, PC.DEFAULTS[k])


def _trace(c, first=0, B=None):
    model, Bc, opts = c
    eng = _engine(model)
    x, k, cond = PC.inputs(model, Bc if B is None else B, first=first)
    with _Options(eng, opts):
        eps, rows = eng.unet_trace(x.cuda(), k, cond.cuda())
    eng.check_fault()
    return (x, k, cond), eps, rows


def _plan_sig(r):
    return r["plan"], r["cs"], r["kw"], r["tile"]


def _bct(t, sel, ch, dtype):
    """rows `sel` of a stored (B, T, stride) tap -> (n, C, T) on the host"""
    return t[sel][..., :ch].permute(0, 2, 1).to("cpu", dtype).contiguous()


def _stage_map(stages, rows):
    """oracle stage -> (table row, 't' | 't_res'); the oracle's 'film' stage is the sum of rows 1 and 2"""
    conv = [i for i, r in enumerate(rows) if r["kind"] not in ("input", "film_g", "film_t")]
    assert [rows[i]["kind"] for i in (0, 1, 2)] == ["input", "film_g", "film_t"]
    m, ci = [], 0
    for kind, *_ in stages:
        if kind == "input":
            m.append((0, "t"))
        elif kind == "film":
            m.append((2, "film"))
        elif kind == "proj":
            m.append((m[-1][0], "t_res"))
        else:
            m.append((conv[ci], "t"))
            ci += 1
    assert ci == len(conv), "the trace has launches the oracle has no stage for"
    assert [rows[g]["kind"] for (g, w), s in zip(m, stages) if w == "t"] == [s[0] for (g, w), s in zip(m, stages) if w == "t"]
    return m


def _check_case(c):
    """Traces the case, checks every stage against float64 on its own tapped inputs, the table against `expected_dispatch`, the wiring, the
    exact properties.  -> rows.  Misses are collected and reported together."""
    model, B, opts = c
    tag = PC.case_id(c)
    D, G, T, dims, _ = PC.MODELS[model]
    _, P64, P32 = _model_params(model)
    eng = _engine(model)
    (x, k, cond), eps, rows = _trace(c)
    _, eps2, rows2 = _trace(c)
    with _Options(eng, opts):
        plain = eng.unet_forward(x.cuda(), k, cond.cuda())
    eng.check_fault()
    bad = []
    if eng.get_option("range_fallback") != 0:
        bad.append("range_fallback set")
    if not torch.equal(rows[-1]["t"], eps) or rows[-1]["kind"] != "head":
        bad.append("the last tap is not the returned eps")
    if not torch.equal(eps, plain):
        bad.append("the traced call's eps differs from unet_forward's")
    if not (torch.equal(eps, eps2) and len(rows) == len(rows2) and all(
            torch.equal(a["t"], b["t"]) and (a["t_res"] is None or torch.equal(a["t_res"], b["t_res"])) and _plan_sig(a) == _plan_sig(b)
            for a, b in zip(rows, rows2))):
        bad.append("a second traced call gave other bits")
    for i, r in enumerate(rows):
        for t in (r["t"], r["t_res"]):
            if t is None:
                continue
            if not bool(torch.isfinite(t).all()):
                bad.append(f"stage {i} {r['kind']}: non-finite tap")
            if t.shape[-1] > r["channels"] and bool((t[..., r["channels"]:] != 0).any()):
                bad.append(f"stage {i} {r['kind']}: padded channels are not zero")

    stages = torch32.unet_stages(P64, down_dims=dims)
    smap = _stage_map(stages, rows)
    sel = PC.ref_rows(B)
    sel_t = torch.tensor(sel, device="cuda")
    ksel, csel = k[sel], cond[sel]
    # the FiLM parts: each against its own float64 / float32 evaluation; what a first half reads is their sum (the epilogue adds them in fp32)
    n_blocks = sum(1 for s in stages if s[0] == "res1")
    ft, fg = rows[2]["t"][sel_t][:, 0].cpu(), rows[1]["t"][sel_t][:, 0].cpu()
    ft64, fg64 = torch32.unet_film_parts(P64, ksel, csel.double(), n_blocks)
    ft32, fg32 = torch32.unet_film_parts(P32, ksel, csel, n_blocks)
    keys, ncu = set(), _ncu()

    def judge(i, kind, name, r, got, ref64, ref32, plan=""):
        e = PC.stage_error(got, ref64, ref32)
        form = PC.FORMS[r["plan"][8]] if r["plan"][0] >= 0 else "valu"
        print(f"{tag} stage {i:2d} {kind:9s} {name:42s} T{r['t'].shape[1]:<2d} c{r['t'].shape[2]:<4d} {form:4s} {plan} err {e['err']:.3e} err32 {e['err32']:.3e} "
              f"bound {e['bound']:.3e} ratio {e['err'] / e['bound']:.3f} row {sel[e['row']]}")
        w = _worst.setdefault((form, kind), dict(err=0.0, ratio=0.0, err32=0.0, n=0))
        w["err"], w["ratio"], w["err32"], w["n"] = max(w["err"], e["err"]), max(w["ratio"], e["err"] / e["bound"]), max(w["err32"], e["err32"]), w["n"] + 1
        if not e["ok"]:
            bad.append(f"stage {i} {name} [{form} {plan}]: err {e['err']:.3e} > bound {e['bound']:.3e} (err32 {e['err32']:.3e}, row {sel[e['row']]})")

    judge(1, "film_g", "Mish(cond) @ W[E:]", rows[1], fg, fg64, fg32.double())
    judge(2, "film_t", "Mish(temb(k)) @ W[:E] + b", rows[2], ft, ft64, ft32.double())
    film64, film32 = ft.double() + fg.double(), ft + fg

    def tap(j, dtype):
        g, which = smap[j]
        if which == "film":
            return film64 if dtype == torch.float64 else film32
        r = rows[g]
        return _bct(r["t_res"] if which == "t_res" else r["t"], sel_t, r["channels"], dtype)

    for j, (kind, name, inputs, fn) in enumerate(stages):
        g, which = smap[j]
        r = rows[g]
        if kind == "input":
            if not torch.equal(r["t"][..., :D].cpu(), x):
                bad.append("the padded state is not the call's x")
            continue
        if kind == "film":
            continue
        # the wiring the table records is the oracle's
        if which == "t":
            acts = [i for i in inputs if stages[i][0] != "film"]
            want = dict(xa=smap[acts[0]][0], xb=-1, res=-1, res_is_proj=False)
            if kind == "res2":
                want.update(res=smap[acts[1]][0], res_is_proj=stages[acts[1]][0] == "proj")
            elif len(acts) == 2:
                want["xb"] = smap[acts[1]][0]
            got_w = {f: r[f] for f in want}
            if got_w != want:
                bad.append(f"stage {g} {name}: wired {got_w}, the oracle {want}")
                continue
            if kind == "res1" and (smap[inputs[-1]][1] != "film" or r["film_off"] != sum(2 * rows[smap[q][0]]["t"].shape[2] for q in range(j) if stages[q][0] == "res1")):
                bad.append(f"stage {g} {name}: FiLM slice at column {r['film_off']}")
            keys.add(r["plan"])
            want_d, got_d = PC.expected_dispatch(r, B, dict(opts), ncu), PC.dispatch_of(r)
            if want_d != got_d:
                bad.append(f"stage {g} {name}: ran (form, mb, cs, K split) = {got_d}, the regime rule says {want_d}")
        ref64 = fn(P64, *[tap(i, torch.float64) for i in inputs])
        ref32 = fn(P32, *[tap(i, torch.float32) for i in inputs]).double()
        got = tap(j, torch.float64) if kind != "head" else r["t"][sel_t].permute(0, 2, 1).to("cpu", torch.float64)
        p = r["plan"]
        judge(g, kind, name, r, got, ref64, ref32, f"{PC.plan_text(p)} cs{r['cs']} kw{r['kw']} tile{r['tile']}")
    print(f"{tag}: plans reached: " + " ".join(sorted(PC.plan_text(p) for p in keys)))
    _reached[tag] = keys
    owed = [PC.plan_text(p) for p, (how, what) in COVERAGE.items() if how == REACHED and what == tag and p not in keys]
    if owed:
        bad.append(f"tests/planner_stage_coverage.py names this case for {owed}: not launched")
    assert not bad, f"{tag}: {len(bad)} miss(es):\n  " + "\n  ".join(bad)
    return rows


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", PC.BASE_CASES, ids=PC.case_id)
def test_stages(c):
    """Every batch-size regime of every model on the default options: up to 128 plans quarter groups with the K split, up to 256 half
    groups, 257 .. 512 the eight-wave fp16 tiles, 513 .. 992 four waves, from 993 two row blocks; pred_horizon 16; obs_dim 30 / 40,
    global_cond_dim 50, the diffusion policies' and the hierarchical agent's U-Nets; the heavy weight set (activations ~5e3)."""
    _check_case(c)


@pytest.mark.parametrize("c", PC.FORM_CASES, ids=PC.case_id)
def test_stages_on_the_other_forms(c):
    """Every batch above 256 plans also on three bf16 planes (planner_split_f16 = 0) and on the exact-fp32 tiles (planner_split = 0); 200
    and 64 plans under planner_split = 2: exact fp32 while the groups are halved, the split forms with the column split off."""
    rows = _check_case(c)
    forms = {PC.FORMS[r["plan"][8]] for r in rows if r["plan"][0] >= 0}
    o = dict(c[2])
    if o.get("planner_split") == 0:
        assert forms == {"f32"}
    elif o.get("planner_split_f16") == 0:
        assert forms == {"f32", "bf16"}
    else:                                   # planner_split = 2 below 257 plans: split operands only where no group is split over work-groups
        assert ("f16" in forms) == bool(o.get("no_csplit")), forms


def _downstream(rows, moved):
    """stages that read a moved stage, directly or not"""
    dirty = set(moved)
    for i, r in enumerate(rows):
        if any(j in dirty for j in (r["xa"], r["xb"], r["res"]) if j is not None and j >= 0):
            dirty.add(i)
    return dirty


@pytest.mark.parametrize("name,value,model,B,base", PC.OPTION_CASES,
                         ids=[PC.case_id(PC.case(m, B, **dict(b, **{o: v}))) for o, v, m, B, b in PC.OPTION_CASES])
def test_stages_under_option(name, value, model, B, base):
    """Each option that changes a plan, at a batch where it does: every stage still meets the bound and the regime rule, the stages that changed
    plan are the ones the option is about, and no tap that reads none of them changed a bit."""
    _, _, rows0 = _trace(PC.case(model, B, **base))
    rows = _check_case(PC.case(model, B, **dict(base, **{name: value})))
    moved = [i for i in range(len(rows)) if _plan_sig(rows[i]) != _plan_sig(rows0[i])]
    pred, exact = PC.ABOUT[name]
    about = [i for i, r in enumerate(rows0) if r["plan"][0] >= 0 and pred(r)]
    print(f"{name}={value} {model} B={B}: stages moved {moved}, the option is about {about}")
    assert (moved == about) if exact else (moved and set(moved) <= set(about)), (moved, about)
    dirty = _downstream(rows, moved)
    diff = [i for i in range(len(rows)) if i not in dirty and not (torch.equal(rows[i]["t"], rows0[i]["t"]) and (
        rows[i]["t_res"] is None or torch.equal(rows[i]["t_res"], rows0[i]["t_res"])))]
    assert not diff, f"taps that read no moved stage changed: {diff}"


@pytest.mark.parametrize("name,value,model,B", PC.BITWISE_OPTIONS, ids=[f"{m}-B{B}-{o}={v}" for o, v, m, B in PC.BITWISE_OPTIONS])
def test_placement_options_change_no_bit(name, value, model, B):
    """by_sample 0 / 1000 and place2d only say which XCD a work-group lands on: every tap equals the default's bit for bit."""
    _, eps0, rows0 = _trace(PC.case(model, B))
    _, eps, rows = _trace(PC.case(model, B, **{name: value}))
    assert [r["plan"] for r in rows] == [r["plan"] for r in rows0]
    assert any(a["by_sample"] != b["by_sample"] for a, b in zip(rows, rows0)), "the option changed no placement: the case checks nothing"
    diff = [i for i, (a, b) in enumerate(zip(rows, rows0)) if not torch.equal(a["t"], b["t"]) or (a["t_res"] is not None and not torch.equal(a["t_res"], b["t_res"]))]
    assert not diff and torch.equal(eps, eps0), diff


@pytest.mark.parametrize("model,B,first", PC.SUBBATCH, ids=[f"{m}-B{B}-from{f}" for m, B, f in PC.SUBBATCH])
def test_rows_do_not_depend_on_the_batch(model, B, first):
    """Rows [first, B) traced inside the batch and as a batch of their own in the same regime (257 .. 512 | 513 .. 992 | >= 993 plans): the
    same plans and the same bits in every tap."""
    _, _, big = _trace(PC.case(model, B))
    _, _, sub = _trace(PC.case(model, B), first=first, B=B - first)
    assert [_plan_sig(r)[:1] + _plan_sig(r)[3:] for r in big] == [_plan_sig(r)[:1] + _plan_sig(r)[3:] for r in sub], "the two batches are not of one regime"
    bad = []
    for i, (a, b) in enumerate(zip(big, sub)):
        for ta, tb in ((a["t"], b["t"]), (a["t_res"], b["t_res"])):
            if ta is not None and not torch.equal(ta[first:], tb):
                bad.append(f"stage {i} {a['kind']} {PC.plan_text(a['plan']) if a['plan'][0] >= 0 else ''}: max |diff| {float((ta[first:] - tb).abs().max()):.3e}")
    assert not bad, f"{len(bad)} tap(s) differ:\n  " + "\n  ".join(bad)


def test_the_cases_reach_what_the_coverage_table_says():
    """The union of the plans the cases reach is exactly the REACHED half of tests/planner_stage_coverage.py (cases of this module that did not
    run in this session are traced here, unchecked)."""
    for c in PC.all_cases():
        if PC.case_id(c) not in _reached:
            _, _, rows = _trace(c)
            _reached[PC.case_id(c)] = {r["plan"] for r in rows if r["plan"][0] >= 0}
    union = set().union(*_reached.values())
    want = {p for p, (how, _) in COVERAGE.items() if how == REACHED}
    print(f"{len(union)} plans reached by {len(_reached)} cases; {len(COVERAGE) - len(want)} instantiations no U-Net evaluation can reach")
    assert union == want, (sorted(PC.plan_text(p) for p in union - want), sorted(PC.plan_text(p) for p in want - union))
    for (form, kind), w in sorted(_worst.items()):
        print(f"worst {form:4s} {kind:9s}: {w['n']:5d} comparisons, err {w['err']:.3e}, err / bound {w['ratio']:.3f}, err32 {w['err32']:.3e}")
