"""The optimiser kernels of csrc/train.hip on their own -- adam_kernel<kEma>, sumsq1_kernel / sumsq2_kernel, pack_leaf / unpack_leaf and the
host bookkeeping around them (Module::step, gpart_fresh, ema_on) -- against float64, element by element (tests/optim_oracle.py).  -m gpu.

No network, no tape: the state goes into the arenas leaf by leaf (train_load, train_write), the count through train_step_count, and one
train_apply is one launch.  Modules: the IDM (D = 25, A = 7: the smallest arena, leaves padded to INP and AP, total not a multiple of
1024), encoder0 (11 M floats, EMA on), the planner (leaves padded to cin_p, CP, DP) for the norm and the leaf I/O.

Error rule, per quantity: worst measure over EVERY real element <= max(k * 2^-24, 3 * err32), err32 = the same measure of the
float32 restatement on the same inputs (computed here on the CPU), k = the rounded operations on the quantity's path.  No element is
excluded.  An arena's elements are drawn from a pool of 32768 element states (optim_oracle.pool_index); the kernels are element-wise."""
import functools
import json
from collections import OrderedDict

import numpy as np
import pytest
import torch

from latent_diffusion_planning_amd import weights as W
from tests import optim_oracle as O
from tests.util import idm_params, planner_params

pytestmark = pytest.mark.gpu

D, A, T = 25, 7, 8
F32, F64 = np.float32, np.float64
SHAPES = {"idm": W.idm_shapes(W.IDMSpec(D, A)), "encoder0": W.resnet_shapes(), "planner": W.planner_shapes(W.PlannerSpec(D, D))}
SIZES = {m: OrderedDict((k, int(np.prod(s))) for k, s in sh.items()) for m, sh in SHAPES.items()}
N_REAL = {m: sum(s.values()) for m, s in SIZES.items()}
EINVAL, ESTATE, EKEY = -1, -2, -5
ENC_DECAY = 0.999


def _new_engine():
    from latent_diffusion_planning_amd.engine import HipEngine
    return HipEngine(obs_dim=D, action_dim=A, global_cond_dim=D, pred_horizon=T, action_horizon=4)


@pytest.fixture(scope="module")
def eng():
    """IDM without an EMA (adam_kernel<false>), encoder0 with one (adam_kernel<true>), the planner where a test loads it."""
    e = _new_engine()
    e.train_load("idm", idm_params(D=D, A=A))
    e.train_load("encoder0", W.init_resnet_params(seed=5))
    e.train_ema("encoder0", ENC_DECAY)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_ema():
    """A second handle whose IDM keeps an EMA."""
    e = _new_engine()
    e.train_load("idm", idm_params(D=D, A=A))
    e.train_ema("idm", O.TRAJ_DECAY)
    yield e
    e.close()


def _planner(e):
    if not getattr(e, "_optim_planner", False):
        e.train_load("planner", planner_params(D=D))
        e._optim_planner = True


@functools.lru_cache(maxsize=None)
def _index(module):
    idx = O.pool_index(SIZES[module], O.POOL, 7 + len(module))
    return idx, np.concatenate(list(idx.values()))


def _tree(module, pool_arr):
    idx, _ = _index(module)
    return OrderedDict((k, np.asarray(pool_arr, F32)[idx[k]].reshape(SHAPES[module][k])) for k in SHAPES[module])


def _flat(module, tree):
    return np.concatenate([np.asarray(tree[k]).reshape(-1) for k in SHAPES[module]])


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _write_state(e, module, st, count, ema=None):
    """Every arena leaf by leaf (a leaf's padding is written as zeros with it), then the count in front of step `count`."""
    for which, key in ((e.TRAIN_PARAMS, "p"), (e.TRAIN_GRADS, "g"), (e.TRAIN_MU, "mu"), (e.TRAIN_NU, "nu")):
        e.train_write(module, which, _tree(module, st[key]))
    if ema is not None:
        e.train_write(module, e.TRAIN_EMA, _tree(module, ema))
    e.train_step_count(module, set_to=count - 1)


def _read(e, module, which):
    return _flat(module, e.train_read(module, which, SHAPES[module]))


def _arenas(e, module, ema=False):
    ws = [e.TRAIN_PARAMS, e.TRAIN_MU, e.TRAIN_NU] + ([e.TRAIN_EMA] if ema else [])
    return [e.train_arena(module, w).clone() for w in ws]


def _real_mask(e, module):
    """Which arena positions hold real elements (device bool tensor): ones written into every leaf of a zeroed gradient arena.  (That
    pack_leaf puts them in the right places is what the leaf I/O tests below check.)"""
    cache = e.__dict__.setdefault("_optim_masks", {})
    if module not in cache:
        e.train_arena(module, e.TRAIN_GRADS).zero_()
        e.train_write(module, e.TRAIN_GRADS, {k: np.ones(s, F32) for k, s in SHAPES[module].items()})
        cache[module] = e.train_arena(module, e.TRAIN_GRADS) != 0
    return cache[module]


def _padding_is_zero(e, module, ema):
    pad = ~_real_mask(e, module)
    assert int(pad.sum()) > 0
    for w in [e.TRAIN_PARAMS, e.TRAIN_MU, e.TRAIN_NU] + ([e.TRAIN_EMA] if ema else []):
        assert not bool((e.train_arena(module, w)[pad] != 0).any()), f"{module}: padding of arena {w} is not zero after the step"


def _case_state(count, arm, ema):
    st = dict(O.reachable_state(O.POOL, count, O.STATE_SEED[count]))
    e_old = None
    if arm == "zero":                                      # p = 0: the update itself is read at full relative precision
        st["p"] = np.zeros(O.POOL, F32)
        if ema:
            e_old = np.zeros(O.POOL, F32)                  # ... and so is (1 - d) * p_new
    elif ema:
        z = O._rng(5 + count).standard_normal(O.POOL)
        e_old = (st["p"].astype(F64) * (1.0 + 1e-3 * z)).astype(F32)
    return st, e_old


def _report(what, rows):
    """rows: {quantity: (worst, err32, bound, exact_bad)} -> one JSON line, then the assertions."""
    print(json.dumps({"case": what, **{q: dict(worst=float(f"{w:.3e}"), err32=float(f"{e:.3e}"), bound=float(f"{b:.3e}")) for q, (w, e, b, _) in rows.items()}}))
    for q, (w, e, b, bad) in rows.items():
        assert bad == 0, f"{what}: {bad} entries of {q} had to be exact and are not"
        assert np.isfinite(w) and w <= b, f"{what}: {q} worst {w:.3e} > bound {b:.3e} (err32 {e:.3e})"


def _one_launch(e, module, count, lr, arm, ema_decay):
    ema = ema_decay is not None
    st, e_old = _case_state(count, arm, ema)
    lr32 = float(F32(lr))
    ref = O.adam_step64(st["p"], st["g"], st["mu"], st["nu"], lr32, count)
    r32 = O.adam_step32(st["p"], st["g"], st["mu"], st["nu"], lr32, count)
    e32 = O.step_errors(r32, ref, st)
    _write_state(e, module, st, count, ema=e_old)
    e.train_apply(module, lr)
    assert e.train_step_count(module) == count
    _, flat = _index(module)
    got = dict(p=_read(e, module, e.TRAIN_PARAMS), mu=_read(e, module, e.TRAIN_MU), nu=_read(e, module, e.TRAIN_NU))
    assert all(np.isfinite(v).all() for v in got.values())
    on = lambda d: {k: v[flat] for k, v in d.items() if isinstance(v, np.ndarray)}
    eg = O.step_errors(got, on(ref), on(st))
    rows = {q: (eg[q][0], e32[q][0], O.bound(q, e32[q][0]), eg[q][1]) for q in ("mu", "nu", "update")}
    if lr == 0:
        assert np.array_equal(_bits(got["p"]), _bits(st["p"][flat])), "lr = 0 changed the parameters"
        assert not np.array_equal(_bits(got["nu"]), _bits(st["nu"][flat])), "lr = 0: the moments must still advance"
    if ema:
        got_e = _read(e, module, e.TRAIN_EMA)
        x32 = O.ema_error(O.ema32(e_old, r32["p"], ema_decay), e_old, r32["p"], ema_decay)
        xg = O.ema_error(got_e, e_old[flat], got["p"], ema_decay)
        rows["ema"] = (xg[0], x32[0], O.bound("ema", x32[0]), xg[1])
    _padding_is_zero(e, module, ema)
    _report(f"{module} count={count} lr={lr:g} p={arm}", rows)


# ---- (a) one launch, every element ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", ["trained", "zero"])
@pytest.mark.parametrize("lr", O.LRS)
@pytest.mark.parametrize("count", O.COUNTS)
def test_one_adam_launch_on_the_idm_matches_float64_per_element(eng, count, lr, arm):
    assert N_REAL["idm"] % 1024 != 0 and int(eng.train_arena("idm", 0).numel()) % 1024 != 0      # the last stripe is a partial one
    _one_launch(eng, "idm", count, lr, arm, None)


@pytest.mark.parametrize("count,lr,arm", [(1, 1e-4, "trained"), (2, 1e-6, "zero"), (10, 1e-4, "zero"), (1000, 0.0, "trained"), (500000, 1e-4, "trained")])
def test_one_adam_and_ema_launch_on_encoder0_matches_float64_per_element(eng, count, lr, arm):
    assert N_REAL["encoder0"] == 11176512
    _one_launch(eng, "encoder0", count, lr, arm, ENC_DECAY)


# ---- (b) the count ----------------------------------------------------------------------------------------------------------------------
def _trees(st):
    return {k: _tree("idm", st[k]) for k in ("p", "g", "mu", "nu")}


def test_the_count_advances_by_one_per_apply(eng):
    st = O.reachable_state(O.POOL, 7, O.STATE_SEED[7])
    _write_state(eng, "idm", st, 7)
    for k in range(3):
        assert eng.train_step_count("idm") == 6 + k
        eng.train_apply("idm", 1e-4)
    assert eng.train_step_count("idm") == 9


def test_a_restored_count_steps_like_the_count_set_by_hand(eng):
    """train_load(params, mu, nu, step = k) + apply = the same state written leaf by leaf + train_step_count(k) + apply, bitwise."""
    st = O.reachable_state(O.POOL, 8, O.STATE_SEED[8])
    t = _trees(st)
    eng.train_load("idm", t["p"], mu=t["mu"], nu=t["nu"], step=7)
    assert eng.train_step_count("idm") == 7
    eng.train_write("idm", eng.TRAIN_GRADS, t["g"])
    eng.train_apply("idm", 1e-4)
    a = _arenas(eng, "idm")
    eng.train_load("idm", idm_params(D=D, A=A))            # another state in between
    _write_state(eng, "idm", st, 8)
    eng.train_apply("idm", 1e-4)
    assert eng.train_step_count("idm") == 8
    for x, y in zip(a, _arenas(eng, "idm")):
        assert torch.equal(x, y)
    ref = O.adam_step64(st["p"], st["g"], st["mu"], st["nu"], float(F32(1e-4)), 8)          # and it is step 8 that ran, not step 1
    got = dict(p=_read(eng, "idm", 0), mu=_read(eng, "idm", 2), nu=_read(eng, "idm", 3))
    _, flat = _index("idm")
    err = O.step_errors(got, {k: v[flat] for k, v in ref.items()}, {k: st[k][flat] for k in ("p", "g", "mu", "nu")})
    assert err["update"][0] <= 1e-5, err                   # (bias corrections of count 1 instead of 8 are off by a factor of 1.8)


def test_two_applies_equal_one_apply_and_a_restored_second(eng):
    st = O.reachable_state(O.POOL, 7, O.STATE_SEED[7])
    _write_state(eng, "idm", st, 7)
    eng.train_apply("idm", 1e-4)
    eng.train_apply("idm", 1e-4)
    two = _arenas(eng, "idm")
    _write_state(eng, "idm", st, 7)
    eng.train_apply("idm", 1e-4)
    mid = {w: eng.train_read("idm", w, SHAPES["idm"]) for w in (eng.TRAIN_PARAMS, eng.TRAIN_MU, eng.TRAIN_NU)}
    eng.train_load("idm", mid[eng.TRAIN_PARAMS], mu=mid[eng.TRAIN_MU], nu=mid[eng.TRAIN_NU], step=7)
    eng.train_write("idm", eng.TRAIN_GRADS, _tree("idm", st["g"]))
    eng.train_apply("idm", 1e-4)
    assert eng.train_step_count("idm") == 8
    for x, y in zip(two, _arenas(eng, "idm")):
        assert torch.equal(x, y)


# ---- (c) the EMA ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decay", [0.0, 0.99, 0.9999, 1.0])
def test_ema_decays(eng_ema, decay):
    count, lr = 10, 1e-4
    st, e_old = _case_state(count, "trained", True)
    eng_ema.train_ema("idm", decay)
    _write_state(eng_ema, "idm", st, count, ema=e_old)
    eng_ema.train_apply("idm", lr)
    _, flat = _index("idm")
    p_new, got = _read(eng_ema, "idm", eng_ema.TRAIN_PARAMS), _read(eng_ema, "idm", eng_ema.TRAIN_EMA)
    if decay == 0.0:
        assert np.array_equal(_bits(got), _bits(p_new)), "decay 0: the EMA is not the new parameters"
    if decay == 1.0:
        assert np.array_equal(_bits(got), _bits(e_old[flat])), "decay 1: the EMA moved"
    r32 = O.adam_step32(st["p"], st["g"], st["mu"], st["nu"], float(F32(lr)), count)
    x32 = O.ema_error(O.ema32(e_old, r32["p"], decay), e_old, r32["p"], decay)
    xg = O.ema_error(got, e_old[flat], p_new, decay)
    _padding_is_zero(eng_ema, "idm", True)
    _report(f"idm ema decay={decay:g}", {"ema": (xg[0], x32[0], O.bound("ema", x32[0]), xg[1])})


@pytest.mark.parametrize("count", [1, 1000])
def test_ema_on_and_off_leave_the_same_bits(eng, eng_ema, count):
    """adam_kernel<true> and adam_kernel<false> from one state: P, MU, NU and the norm taken from the partials they leave."""
    st, e_old = _case_state(count, "trained", True)
    eng_ema.train_ema("idm", 0.999)
    _write_state(eng, "idm", st, count)
    _write_state(eng_ema, "idm", st, count, ema=e_old)
    eng.train_apply("idm", 1e-4)
    eng_ema.train_apply("idm", 1e-4)
    n_off, n_on = eng.train_grad_norm(["idm"]), eng_ema.train_grad_norm(["idm"])
    for x, y in zip(_arenas(eng, "idm"), _arenas(eng_ema, "idm")):
        assert torch.equal(x, y)
    assert _bits(n_off.cpu().numpy()) == _bits(n_on.cpu().numpy())


def test_init_and_load_reseed_the_ema(eng_ema):
    st, e_old = _case_state(10, "trained", True)
    eng_ema.train_ema("idm", 0.99)
    P, E = (lambda: eng_ema.train_arena("idm", eng_ema.TRAIN_PARAMS)), (lambda: eng_ema.train_arena("idm", eng_ema.TRAIN_EMA))
    assert torch.equal(P(), E())                           # train_ema seeds it
    _write_state(eng_ema, "idm", st, 10, ema=e_old)
    eng_ema.train_apply("idm", 1e-4)
    assert not torch.equal(P(), E())
    eng_ema.train_init(["idm"])                            # from the parameters last uploaded
    assert torch.equal(P(), E()) and eng_ema.train_step_count("idm") == 0
    assert np.array_equal(_bits(_read(eng_ema, "idm", eng_ema.TRAIN_EMA)), _bits(_flat("idm", idm_params(D=D, A=A))))
    eng_ema.train_apply("idm", 1e-4)
    t = _tree("idm", st["p"])
    eng_ema.train_load("idm", t)
    assert torch.equal(P(), E())
    assert np.array_equal(_bits(_read(eng_ema, "idm", eng_ema.TRAIN_EMA)), _bits(_flat("idm", t)))


# ---- (d) the gradient norm ------------------------------------------------------------------------------------------------------------
def _norm_refs(e, modules):
    """float64 and the striped float32 restatement over the gradient arenas as they lie on the device -> (n64, bound, the restatement's
    relative error); bound = max(1e-5 -- what the whole-step tests use --, 3 * that error)."""
    imgs = [e.train_arena(m, e.TRAIN_GRADS).cpu().numpy() for m in modules]
    n64 = float(np.sqrt(sum(O.grad_norm64(a) ** 2 for a in imgs)))
    n32 = float(np.sqrt(sum(float(O.grad_norm32_striped(a)) ** 2 for a in imgs)))
    return n64, max(1e-5, 3.0 * abs(n32 - n64) / n64), abs(n32 - n64) / n64


def _write_grads(e, module, seed):
    g = O.GradStream(O.POOL, seed, zero_from=0)(3)
    e.train_write(module, e.TRAIN_GRADS, _tree(module, g))
    return g


@pytest.mark.parametrize("modules", [["idm"], ["encoder0"], ["idm", "encoder0"]])
def test_grad_norm_matches_float64(eng, modules):
    for i, m in enumerate(modules):
        _write_grads(eng, m, 300 + i)
    got = float(eng.train_grad_norm(modules))
    n64, bound, e32 = _norm_refs(eng, modules)
    print(json.dumps({"case": "grad_norm " + "+".join(modules), "rel_err": float(f"{abs(got - n64) / n64:.3e}"), "err32": float(f"{e32:.3e}"), "bound": bound}))
    assert abs(got - n64) <= bound * n64
    if len(modules) == 2:                                  # both arenas count: neither module's own norm is within the bound of the sum
        for m in modules:
            assert abs(float(eng.train_grad_norm([m])) - n64) > bound * n64


@pytest.mark.parametrize("module", ["idm", "encoder0"])
def test_the_partials_adam_leaves_are_the_first_stage(eng, module):
    """Directly after an apply the norm comes from the partials the Adam kernel left; train_arena(GRADS) marks them stale and changes no
    data, so the next call runs sumsq1_kernel over the same gradients: the same bits.  Then new gradients: the norm is theirs."""
    count = 10
    st, e_old = _case_state(count, "trained", module == "encoder0")
    _write_state(eng, module, st, count, ema=e_old)
    before = eng.train_grad_norm([module]).cpu().numpy()   # first stage run on the written gradients
    eng.train_apply(module, 1e-4)
    fresh = eng.train_grad_norm([module]).cpu().numpy()    # Adam's partials
    g_arena = eng.train_arena(module, eng.TRAIN_GRADS)     # marks the partials stale
    snap = g_arena.clone()
    stale = eng.train_grad_norm([module]).cpu().numpy()    # first stage again
    assert torch.equal(snap, eng.train_arena(module, eng.TRAIN_GRADS))
    assert _bits(fresh) == _bits(stale) == _bits(before), (fresh, stale, before)
    n64, bound, _ = _norm_refs(eng, [module])
    assert abs(float(fresh) - n64) <= bound * n64
    eng.train_apply(module, 1e-4)                          # partials fresh again ...
    _write_grads(eng, module, 310)                         # ... and a write makes them stale
    got = float(eng.train_grad_norm([module]))
    new64, bound, _ = _norm_refs(eng, [module])
    assert abs(new64 - n64) > 10 * bound * n64             # (the new gradients have another norm)
    assert abs(got - new64) <= bound * new64


def test_grad_norm_refuses_three_modules(eng):
    from latent_diffusion_planning_amd._lib import LDPHipError
    _planner(eng)
    with pytest.raises(LDPHipError) as e:
        eng.train_grad_norm(["idm", "encoder0", "planner"])
    assert e.value.code == EINVAL


@pytest.mark.parametrize("module", ["idm", "encoder0", "planner"])
def test_the_norm_of_ones_is_exactly_the_root_of_the_real_element_count(eng, module):
    """Ones in every leaf of a zeroed gradient arena: stripe sums <= 1024 and their double sum are exact, so the norm is exactly
    sqrt(real elements) -- pack_leaf puts nothing into padding and loses nothing."""
    if module == "planner":
        _planner(eng)
    g = eng.train_arena(module, eng.TRAIN_GRADS)
    g.zero_()
    eng.train_write(module, eng.TRAIN_GRADS, {k: np.ones(s, F32) for k, s in SHAPES[module].items()})
    assert int((g != 0).sum()) == N_REAL[module] and float(g.sum(dtype=torch.float64)) == N_REAL[module]
    assert int(g.numel()) > N_REAL[module]                 # the module has padding
    got = eng.train_grad_norm([module]).cpu().numpy()
    assert _bits(got) == _bits(F32(np.sqrt(F64(N_REAL[module])))), (float(got), np.sqrt(N_REAL[module]))


# ---- (e) leaf I/O -----------------------------------------------------------------------------------------------------------------------
def _layout(e, module, which):
    """[(path, off, size_p, real elements)] in arena order, found from the outside: the arena is filled with 1.5, one leaf of 3.0 is
    written, and what changed is the leaf's slot [off, off + size_p) -- 3.0 where it has elements, 0.0 in its padding, one contiguous
    range, nothing else."""
    arena = e.train_arena(module, which)
    n = int(arena.numel())
    out = []
    for k, shape in SHAPES[module].items():
        arena.fill_(1.5)
        e.train_write(module, which, {k: np.full(shape, 3.0, F32)})
        ch = arena != 1.5
        cnt = int(ch.sum())
        lo = int(ch.to(torch.uint8).argmax())
        hi = n - int(ch.flip(0).to(torch.uint8).argmax())
        assert cnt == hi - lo > 0, f"{module}/{k}: a write changed {cnt} floats spread over [{lo}, {hi})"
        real = int((arena[lo:hi] == 3.0).sum())
        assert real == SIZES[module][k] and int((arena[lo:hi] == 0.0).sum()) == cnt - real, f"{module}/{k}"
        out.append((k, lo, cnt, real))
    out.sort(key=lambda r: r[1])
    end = 0
    for k, lo, size_p, _ in out:                           # slots of whole 64 floats, back to back
        assert lo == end and lo % 64 == 0, f"{module}/{k}: slot at {lo}, the previous one ends at {end}"
        end = lo + (size_p + 63) // 64 * 64
    assert end == n == sum((r[2] + 63) // 64 * 64 for r in out)
    return out


def _whiches(e, ema=True):
    return [e.TRAIN_PARAMS, e.TRAIN_GRADS, e.TRAIN_MU, e.TRAIN_NU] + ([e.TRAIN_EMA] if ema else [])


def _roundtrip(e, module, which, paths, seed):
    """Random bit patterns (NaNs, infinities, subnormals, -0 among them) come back as they went in."""
    g = O._rng(seed)
    tree = {k: g.integers(0, 2 ** 32, size=SHAPES[module][k], dtype=np.uint32).view(F32) for k in paths}
    for k in paths:                                        # one leaf at a time, so that a later write cannot repair an earlier one
        e.train_write(module, which, {k: tree[k]})
    back = e.train_read(module, which, {k: SHAPES[module][k] for k in paths})
    for k in paths:
        assert np.array_equal(back[k].view(np.uint32), tree[k].view(np.uint32)), f"{module}/{k}, arena {which}"


def test_leaf_io_on_the_idm(eng_ema):
    e = eng_ema
    for w in _whiches(e):
        lay = _layout(e, "idm", w)
        assert [r[0] for r in lay] == list(SHAPES["idm"])
        padded = {r[0] for r in lay if r[2] > r[3]}
        assert padded == {"MLPResNet_0/Dense_0/kernel", "MLPResNet_0/Dense_1/kernel", "MLPResNet_0/Dense_1/bias"}, padded
        _roundtrip(e, "idm", w, list(SHAPES["idm"]), 400 + w)
    e.train_load("idm", idm_params(D=D, A=A))


def test_leaf_io_on_encoder0(eng):
    for w in _whiches(eng):
        _layout(eng, "encoder0", w)
        _roundtrip(eng, "encoder0", w, list(SHAPES["encoder0"]), 410 + w)
    eng.train_load("encoder0", W.init_resnet_params(seed=5))


def test_leaf_io_on_the_padded_leaves_of_the_planner(eng):
    _planner(eng)
    eng.train_ema("planner", 0.999)
    lay = _layout(eng, "planner", eng.TRAIN_PARAMS)
    padded = [r[0] for r in lay if r[2] > r[3]]
    kinds = {k.split("/", 1)[1] if k.startswith("ConditionalResidualBlock1D") else k for k in padded}
    # cin -> cin_p (the first block's two convolutions), E + G -> CP (every FiLM layer), D -> DP (the output convolution and its bias)
    assert kinds == {"Conv1dBlock_0/Conv_0/kernel", "Conv_0/kernel", "Dense_0/kernel", "Conv_0/bias"}, kinds
    assert sum(k.endswith("/Dense_0/kernel") for k in padded) == sum(k.endswith("/Dense_0/kernel") for k in SHAPES["planner"]) > 0
    for w in _whiches(eng):
        _roundtrip(eng, "planner", w, padded, 420 + w)
    eng.train_load("planner", planner_params(D=D))


def test_leaf_io_return_codes(eng):
    from latent_diffusion_planning_amd._lib import LDPHipError
    k = "MLPResNet_0/Dense_1/kernel"                       # (256, 7) in a (256, 32) slot: neither count is the other
    for bad in (np.zeros((256, 32), F32), np.zeros((256, 6), F32)):
        with pytest.raises(LDPHipError) as e:
            eng.train_write("idm", eng.TRAIN_PARAMS, {k: bad})
        assert e.value.code == EINVAL
        with pytest.raises(LDPHipError) as e:
            eng.train_read("idm", eng.TRAIN_PARAMS, {k: bad.shape})
        assert e.value.code == EINVAL
    for call in (lambda: eng.train_write("idm", eng.TRAIN_MU, {"MLPResNet_0/Dense_9/kernel": np.zeros((256, 7), F32)}),
                 lambda: eng.train_read("idm", eng.TRAIN_MU, {"MLPResNet_0/Dense_9/kernel": (256, 7)})):
        with pytest.raises(LDPHipError) as e:
            call()
        assert e.value.code == EKEY
    for call in (lambda: eng.train_read("idm", eng.TRAIN_EMA, {k: (256, 7)}), lambda: eng.train_write("idm", eng.TRAIN_EMA, {k: np.zeros((256, 7), F32)}),
                 lambda: eng.train_arena("idm", eng.TRAIN_EMA)):
        with pytest.raises(LDPHipError) as e:              # this handle's IDM keeps no EMA
            call()
        assert e.value.code == ESTATE


# ---- (f) a trajectory -------------------------------------------------------------------------------------------------------------------
def test_300_steps_follow_the_float64_optimiser(eng_ema):
    """300 applies at the reference's peak lr (1e-4, above anything the goldens reach), EMA 0.999, the gradients uploaded per step."""
    e, tr = eng_ema, O.trajectory()
    _, flat = _index("idm")
    e.train_load("idm", _tree("idm", tr["p0"]))
    e.train_ema("idm", O.TRAJ_DECAY)
    for t in range(O.TRAJ_STEPS):
        e.train_write("idm", e.TRAIN_GRADS, _tree("idm", tr["stream"](t)))
        e.train_apply("idm", O.TRAJ_LR)
    assert e.train_step_count("idm") == O.TRAJ_STEPS == 300
    r64, r32 = tr["r64"], tr["r32"]
    out = {}
    for name, which in (("p", e.TRAIN_PARAMS), ("ema", e.TRAIN_EMA)):
        got = _read(e, "idm", which).astype(F64)
        d_got, d_32 = np.abs(got - r64[name][flat]), np.abs(r32[name].astype(F64) - r64[name])[flat]
        out[name] = dict(mean=float(f"{d_got.mean():.3e}"), mean32=float(f"{d_32.mean():.3e}"), max=float(f"{d_got.max():.3e}"), max32=float(f"{d_32.max():.3e}"))
    moved = float(np.abs(r64["p"] - tr["p0"])[flat].mean())
    nu = _read(e, "idm", e.TRAIN_NU)
    n32 = O._rel(np.abs(r32["nu"].astype(F64) - r64["nu"]), r64["nu"])
    ng = O._rel(np.abs(nu.astype(F64) - r64["nu"][flat]), r64["nu"][flat])
    print(json.dumps({"case": "idm 300 steps", **out, "mean_move": float(f"{moved:.3e}"),
                      "nu": dict(worst=float(f"{ng[0]:.3e}"), err32=float(f"{n32[0]:.3e}"), bound=float(f"{O.bound('nu', n32[0]):.3e}"))}))
    for name, r in out.items():
        assert r["mean"] <= 3.0 * r["mean32"] and r["max"] <= 3.0 * r["max32"], (name, r)
    assert ng[1] == 0 and ng[0] <= O.bound("nu", n32[0]), (ng, n32)
    _padding_is_zero(e, "idm", True)
