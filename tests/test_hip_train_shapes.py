"""Every kernel and launch shape of the training GEMM family (csrc/train.hip seg_gemm<A_KC, B_KC, MT, KI>, seg_gemm_big, the in-launch split-K
finish and reduce_parts_kernel) against the float64 autograd oracle (oracle/train.py), on every entry of every gradient leaf.  -m gpu.

Which instantiation a gradient call ran is read from the handle's launch counters (`stat_train_gemm_<nn|nt|tn>_<32|64|128>[_ki2]`,
`stat_train_gemm_fused`, `stat_train_gemm_reduce`) before and after the call:

    configuration   options                                    must run                          must not run
    t32             defaults                                   all three _32; fused              any _64, _128, _ki2
    t64             train_small_wg=0                           all three _64                     any _32
    t128            train_big=1                                all three _128 (M, N >= 128)
    t128_64         train_big=1, train_small_wg=0              _128 and _64                      any _32
    ki2_32          train_intra_split=1                        all three _32_ki2 (K split >= 2)
    ki2_64          train_intra_split=1, train_small_wg=0      all three _64_ki2 (K split >= 2)
    nosplit         train_split=0                                                                fused, reduce
    deep / shallow  train_wg_target=1536 / 48                  fused (deep)
    gn_generic      train_gn4=0
    ungrouped       train_group_proj=0
    reduce          train_fuse_reduce=0                        reduce                            fused

Where a batch cannot reach a cell (_128_nn needs 128 rows; a weight gradient over 32 rows has one K step and cannot split), the expectation
is what the `gemm_shape` rule restated in tests/train_cases.py gives for launches the tape is known to make (train_cases.known_launches);
tests/test_train_cpu.py checks that the cases below reach all 15 instantiations, the in-launch finish and the reduce launch.

A. every configuration against float64, per entry: |got - ref64| <= 1e-4 max|ref64 leaf| + 1e-12; loss 1e-5 max(1, |loss|); g_norm 1e-5.
B. the reference's batch (256 plans, 2048 IDM rows) against the weighted sum of its 32-row chunks: 2e-4 max|G leaf| + 1e-12.
C. bit-equality: in-launch finish == reduce launch per tile family; stream placement (train_streams, train_sides) changes no bit.
"""
import json

import numpy as np
import pytest
import torch

from latent_diffusion_planning_amd import weights as W
from tests import train_cases as TC
from tests.train_cases import A, D, T
from tests.util import idm_params, planner_params

pytestmark = pytest.mark.gpu

P_SHAPES = W.planner_shapes(W.PlannerSpec(D, D))
I_SHAPES = W.idm_shapes(W.IDMSpec(D, A))
ALL = list(TC.CONFIGS)
#         case -> (model, plans or rows, seed, configurations)
CASES = dict(p3=("planner", 3, 953, ALL), p33=("planner", 33, 983, ALL), p129=("planner", 129, 1079, ["t32", "t64", "t128", "t128_64"]),
             i24=("idm", 24, 2024, ALL), i320=("idm", 320, 2320, ALL))


@pytest.fixture(scope="module")
def eng():
    from latent_diffusion_planning_amd.engine import HipEngine
    e = HipEngine(obs_dim=D, action_dim=A, global_cond_dim=D, pred_horizon=T, action_horizon=4)
    e.load_params(planner=planner_params(D=D), idm=idm_params(D=D, A=A))
    e.train_init(["planner", "idm"])
    yield e
    torch.cuda.synchronize()
    e.close()


@pytest.fixture(autouse=True)
def _options_restored(eng):
    before = {k: eng.get_option(k) for k in TC.DEFAULTS}
    assert before == TC.DEFAULTS, before
    yield
    for k, v in before.items():
        eng.set_option(k, v)


def _configure(eng, name):
    for k, v in TC.options(name).items():
        eng.set_option(k, v)


@pytest.fixture(scope="module")
def case():
    """case name -> its inputs and the float64 oracle run, computed once per module and never modified."""
    cache = {}

    def get(name):
        if name not in cache:
            model, n, seed, _ = CASES[name]
            torch.set_num_threads(16)
            if model == "planner":
                c = TC.planner_batch(n, seed)
                cache[name] = dict(inputs=c, rows=-(-n // 32) * 32, **TC.oracle_planner(planner_params(D=D), c, alpha=1.3))
            else:
                c, info = TC.idm_rows(idm_params(D=D, A=A), n, seed)
                print(f"IDM rows, case {name}", json.dumps(info))
                assert info["ratio"] >= TC.MARGIN_OVER_ROUNDOFF, info
                cache[name] = dict(inputs=c, rows=-(-n // 32) * 32, **TC.oracle_idm(idm_params(D=D, A=A), c, alpha=0.7))
        return cache[name]
    return get


def _dev(x):
    return torch.tensor(x).cuda()


def _planner_call(eng, c, alpha=1.0):
    return eng.train_planner_grad(_dev(c["obs_emb"][:, 1:].copy()), _dev(c["noise"]), c["t"], _dev(c["obs_emb"][:, 0].copy()), alpha=alpha)


def _idm_call(eng, c, alpha=1.0):
    return eng.train_idm_grad(_dev(c["s"]), _dev(c["a0"]), _dev(c["noise"]), c["t"], alpha=alpha)


def _grad(eng, model, c, alpha=1.0):
    """One gradient call -> (loss, norm, the whole gradient tree)."""
    loss = float(_planner_call(eng, c, alpha) if model == "planner" else _idm_call(eng, c, alpha))
    gn = float(eng.train_grad_norm([model]))
    return loss, gn, eng.train_read(model, eng.TRAIN_GRADS, P_SHAPES if model == "planner" else I_SHAPES)


def _attested(eng, model, rows, cfg, c, alpha=1.0):
    """The gradient call under configuration `cfg`, with the launch counters held against train_cases.expected."""
    _configure(eng, cfg)
    before = TC.read_counters(eng)
    out = _grad(eng, model, c, alpha)
    must, never = TC.expected(model, rows, cfg)
    diff = TC.check_counters(before, TC.read_counters(eng), must, never, f"{model}, {rows} rows, {cfg}")
    return out + ({k: v for k, v in diff.items() if v},)


# ---- A. every configuration against float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cfg", [(n, c) for n, v in CASES.items() for c in v[3]])
def test_every_gradient_entry_matches_float64_in_every_launch_shape(name, cfg, eng, case):
    model = CASES[name][0]
    o = case(name)
    alpha = 1.3 if model == "planner" else 0.7
    loss, gn, got, ran = _attested(eng, model, o["rows"], cfg, o["inputs"], alpha)
    worst, bad = TC.every_entry(got, o["grads"], 1e-4)
    print("train gemm shapes A", json.dumps(dict(case=name, cfg=cfg, rows=o["rows"], **worst, loss_err=abs(loss - o["loss"]),
                                                 g_norm_rel=abs(gn - o["g_norm"]) / o["g_norm"], ran=ran)))
    assert not bad, f"{name} under {cfg}: {len(bad)} leaves over the bound:\n" + "\n".join(bad[:20])
    assert abs(loss - o["loss"]) <= 1e-5 * max(1.0, abs(o["loss"])), (loss, o["loss"])
    assert abs(gn - o["g_norm"]) <= 1e-5 * o["g_norm"], (gn, o["g_norm"])


def test_the_counters_are_read_only(eng):
    for c in TC.COUNTERS:
        assert eng.get_option(c) >= 0
        with pytest.raises(Exception, match="unknown option"):
            eng.set_option(c, 0)
    with pytest.raises(Exception, match="unknown option"):
        eng.get_option("stat_train_gemm_nn_128_ki2")


# ---- B. the reference batch by decomposition ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reference_batch():
    """model -> the reference's batch (train_bc.yaml: 256 samples = 256 plans, 2048 IDM rows) and, once per module, the weighted sum of its
    32-row chunks run under t32 (the shape part A pins): G(batch) = sum_c (|c| / B) G(chunk c), since the loss is a mean over samples and
    neither GroupNorm (per sample) nor LayerNorm (per row) couples them."""
    cache = {}

    def get(eng, model):
        if model not in cache:
            if model == "planner":
                c, n = TC.planner_batch(256, 1256), 256
            else:
                (c, info), n = TC.idm_rows(idm_params(D=D, A=A), 2048, 3048), 2048
                print("IDM rows, reference batch", json.dumps(info))
                assert info["ratio"] >= TC.MARGIN_OVER_ROUNDOFF, info
            chunks, loss = [], 0.0
            for lo in range(0, n, 32):
                part = TC.take_rows(c, slice(lo, lo + 32))
                l, _, g, _ = _attested(eng, model, 32, "t32", part)
                chunks.append((32, g))
                loss += 32 / n * l
            cache[model] = dict(inputs=c, rows=n, comb=TC.combine(chunks), loss=loss)
        return cache[model]
    return get


@pytest.mark.parametrize("cfg", ["t32", "t64", "t128", "deep"])
@pytest.mark.parametrize("model", ["planner", "idm"])
def test_reference_batch_is_the_weighted_sum_of_its_chunks(model, cfg, eng, reference_batch):
    r = reference_batch(eng, model)
    loss, gn, got, ran = _attested(eng, model, r["rows"], cfg, r["inputs"])
    worst, bad = TC.every_entry(got, r["comb"], 2e-4, scale=got)
    print("train gemm shapes B", json.dumps(dict(model=model, cfg=cfg, rows=r["rows"], **worst, ran=ran)))
    assert not bad, f"{model} at {r['rows']} rows under {cfg}: {len(bad)} leaves over the bound:\n" + "\n".join(bad[:20])
    assert np.isfinite(gn) and gn > 0
    assert abs(loss - r["loss"]) <= 1e-5 * max(1.0, abs(r["loss"])), (loss, r["loss"])


# ---- C. bitwise properties --------------------------------------------------------------------------------------------------------------------
def _both_arenas(eng, pc, ic):
    lp, li = _planner_call(eng, pc), _idm_call(eng, ic)
    gn = eng.train_grad_norm(["planner", "idm"])
    return (torch.stack([lp, li, gn]).clone(), eng.train_arena("planner", eng.TRAIN_GRADS).clone(), eng.train_arena("idm", eng.TRAIN_GRADS).clone())


def _bit_equal(ref, got, what):
    for r, g, leaf in zip(ref, got, ("losses / norm", "planner gradient arena", "IDM gradient arena")):
        assert torch.equal(r, g), (what, leaf, int((r != g).sum()))


@pytest.mark.parametrize("cfg", ["t32", "t64", "t128"])
def test_in_launch_finish_equals_the_reduce_launch_in_every_tile_family(cfg, eng):
    """train_fuse_reduce 0 / 1 under each tile family, 64 plans and 512 IDM rows, three repetitions: losses, norm and both gradient arenas
    bit-equal (train_group_proj = 0: the grouped launches have no C-layout workspace and never split K without the in-launch finish)."""
    pc, ic = TC.planner_batch(64, 1064), TC.idm_pool(512, 1512)
    _configure(eng, cfg)
    eng.set_option("train_group_proj", 0)
    eng.set_option("train_fuse_reduce", 0)
    c0 = TC.read_counters(eng)
    ref = _both_arenas(eng, pc, ic)
    c1 = TC.read_counters(eng)
    assert c1["reduce"] > c0["reduce"] and c1["fused"] == c0["fused"], (c0, c1)
    assert torch.isfinite(ref[0]).all() and float(ref[1].abs().max()) > 0 and float(ref[2].abs().max()) > 0
    eng.set_option("train_fuse_reduce", 1)
    for rep in range(3):
        got = _both_arenas(eng, pc, ic)
        _bit_equal(ref, got, f"{cfg}, repetition {rep}")
    c2 = TC.read_counters(eng)
    assert c2["reduce"] == c1["reduce"] and c2["fused"] > c1["fused"], (c1, c2)


@pytest.mark.parametrize("B", [64, 256])
def test_stream_placement_changes_no_bit(B, eng):
    """train_streams = 0 (everything on the caller's stream) and train_sides = 2, 3 (the weight-gradient work dealt to more side streams) only
    change where launches are enqueued: the arenas equal the default's bit for bit (a missing cross-stream dependency would show here)."""
    pc, ic = TC.planner_batch(B, 1300 + B), TC.idm_pool(8 * B, 1400 + B)
    ref = _both_arenas(eng, pc, ic)
    assert torch.isfinite(ref[0]).all() and float(ref[1].abs().max()) > 0 and float(ref[2].abs().max()) > 0
    for opt, v in (("train_streams", 0), ("train_sides", 2), ("train_sides", 3)):
        eng.set_option(opt, v)
        for rep in range(2):
            _bit_equal(ref, _both_arenas(eng, pc, ic), f"{opt} = {v}, repetition {rep}")
        eng.set_option(opt, TC.DEFAULTS[opt])
