"""The planner and IDM training tapes (csrc/train.hip: seg_gemm*, gn_fwd / gn_bwd, gn_fwd4 / gn_bwd4, ln_fwd / ln_bwd, act_fwd / act_bwd,
mse_grad, the column sums) on TRAINED-LIKE parameters, against the float64 autograd oracle on every entry of every gradient leaf.  -m gpu.

Every other gradient test of the two modules loads a seeded initialisation and draws inputs from uniform(-1, 1): no Mish input leaves +-6,
no ReLU input exceeds 7.  On tests.util.planner_params_heavy / idm_params_heavy (norm scales over four decades, biases O(10), one output
channel of every kernel x 100: tests.util.trained_like) the same batches put 1 % of the Mish inputs above 20 -- the clamp of mish_x /
mish_dx, without which e (e + 2) overflows from x = 44 and every gradient is NaN -- another 1 % below -20 and some below -88, where expf
underflows; FiLM and GroupNorm scales reach 100; a LayerNorm row is dominated by one unit; half of the IDM's hidden units are dead.
tests/test_train_heavy_cpu.py asserts that census, and the conditions below, without a GPU; tests/train_heavy_cases.py holds the fixtures.

The rule, per entry:  |got - ref64| <= max(1e-4 max|ref64 leaf|, 3 err32_leaf) + 1e-12,  err32_leaf = max|g32 - g64| of the
float32 restatement of the same gradients with the norms' statistics as flax and the kernels compute them (train_heavy_cases.grads32);
err32_leaf <= 1e-4 max|ref64 leaf| in every case (CPU file), so no bound exceeds 3e-4 of its leaf.  Loss 1e-5 max(1, |loss|); g_norm 1e-5.

A. the trained-like sets against float64: the planner (T = 8: 3, 33, 129 plans, the in-range and the "wide" set, the 256-value GroupNorm fast
   paths and the generic kernels alike; T = 16, where only the generic ones run), the IDM (24 and 320 rows), the hierarchical agent's
   U-Net IDM (3 and 40 chunks of 4 actions), the DP policy with the gradient of its 2066-wide condition (3 and 33 samples) -- and one
   constructed edge, a GroupNorm group whose input is exactly constant (var = 0, rstd = 1000).  Planner and IDM cases read the launch
   counters as tests/test_hip_train_shapes.py does, so each runs on the kernels its configuration names.
B. the IDM rows are chosen by a per-unit gate rule (train_heavy_cases.idm_rows_per_unit): each ReLU input against its own round-off.
C. no IDM row exempt: the 8 rows of each pool (init-like, trained-like) closest to a gate, each as a batch of its own, must meet float64
   under ONE assignment of the row's ambiguous gates (|u64| <= 3 roundoff_j; at most 4 of them) on all leaves at once.
"""
import json

import numpy as np
import pytest
import torch

from latent_diffusion_planning_amd import weights as W
from tests import train_cases as TC
from tests import train_heavy_cases as H
from tests.cases import HIER_IDM_DOWN
from tests.train_cases import A, D

pytestmark = pytest.mark.gpu

PLANNER_CFGS = ["t32", "t64", "gn_generic", "reduce", "deep"]
IDM_CFGS = ["t32", "t64", "t128", "reduce"]


def _policy_spec():
    from tests import dp_resnet_oracle as RO
    return RO.planner_spec(RO.RM_IMG, H.POLICY_OH)


class _Engines:
    """One engine handle per module family, built on first use; `use` uploads a parameter set and re-creates the module's training state when
    the module holds another one."""
    BUILD = dict(tape=lambda: dict(obs_dim=D, action_dim=A, global_cond_dim=D, pred_horizon=TC.T, action_horizon=4),
                 t16=lambda: dict(obs_dim=D, action_dim=A, global_cond_dim=D, pred_horizon=16, action_horizon=4),
                 hier=lambda: dict(obs_dim=A, action_dim=A, global_cond_dim=2 * D, pred_horizon=H.IH, action_horizon=H.IH, down_dims=HIER_IDM_DOWN),
                 policy=lambda: dict(obs_dim=A, action_dim=A, global_cond_dim=_policy_spec().global_cond_dim, pred_horizon=H.POLICY_T,
                                     action_horizon=8, image_size=0))
    SHAPES = dict(tape=lambda: W.planner_shapes(W.PlannerSpec(D, D)), t16=lambda: W.planner_shapes(W.PlannerSpec(D, D)),
                  hier=lambda: W.planner_shapes(W.PlannerSpec(A, 2 * D, down_dims=HIER_IDM_DOWN)), policy=lambda: W.planner_shapes(_policy_spec()))

    def __init__(self):
        self.engines, self.loaded = {}, {}

    def use(self, family, pset, module="planner"):
        from latent_diffusion_planning_amd.engine import HipEngine
        if family not in self.engines:
            self.engines[family] = HipEngine(**self.BUILD[family]())
        e = self.engines[family]
        if self.loaded.get((family, module)) != pset:
            e.load_params(**{module: H.params_of(pset)})
            e.train_init([module])
            self.loaded[(family, module)] = pset
        return e

    def shapes(self, family, module="planner"):
        return W.idm_shapes(W.IDMSpec(D, A)) if module == "idm" else self.SHAPES[family]()

    def close(self):
        torch.cuda.synchronize()
        for e in self.engines.values():
            e.close()


@pytest.fixture(scope="module")
def engines():
    es = _Engines()
    yield es
    es.close()


@pytest.fixture(autouse=True)
def _options_restored(engines):
    yield
    for e in engines.engines.values():
        for k, v in TC.DEFAULTS.items():
            e.set_option(k, v)


def _configure(eng, name):
    assert {k: eng.get_option(k) for k in TC.DEFAULTS} == TC.DEFAULTS
    for k, v in TC.options(name).items():
        eng.set_option(k, v)


def _dev(x):
    return torch.tensor(np.ascontiguousarray(x)).cuda()


def _unet_inputs(model, c):
    """-> (x0, noise, t, cond) of train_planner_grad for a case of train_heavy_cases"""
    if model == "planner":
        return _dev(c["obs_emb"][:, 1:]), _dev(c["noise"]), c["t"], _dev(c["obs_emb"][:, 0])
    if model == "hier":                   # LDPHierAgent._nets: the IDM handle's train_planner_grad(a, eps, t, s, w), s = (state, state + idm_horizon)
        return _dev(c["actions"][:, :H.IH]), _dev(c["noise"]), c["t"], _dev(np.concatenate([c["obs_emb"][:, 0], c["obs_emb"][:, H.IH]], axis=-1))
    return _dev(c["x0"]), _dev(c["noise"]), c["t"], _dev(c["cond"])


def _idm_call(eng, c, alpha):
    return eng.train_idm_grad(_dev(c["s"]), _dev(c["a0"]), _dev(c["noise"]), c["t"], alpha=alpha)


def _held_to_the_rule(name, cfg, ref, loss, gn, got, ran=None):
    want = dict(ref["grads"], **({"dcond": ref["dcond"]} if "dcond" in ref else {}))
    worst, bad = TC.every_entry(got, want, 1e-4, floor=H.floors(ref))
    leaf = worst["leaf"]
    print("train heavy A", json.dumps(dict(case=name, cfg=cfg, **worst, err32_over_leafmax=ref["err32"][leaf] / float(np.abs(want[leaf]).max()),
                                           loss_err=abs(loss - ref["loss"]), g_norm_rel=abs(gn - ref["g_norm"]) / ref["g_norm"], ran=ran)))
    assert not bad, f"{name} under {cfg}: {len(bad)} leaves over the bound:\n" + "\n".join(bad[:20])
    assert abs(loss - ref["loss"]) <= 1e-5 * max(1.0, abs(ref["loss"])), (loss, ref["loss"])
    assert abs(gn - ref["g_norm"]) <= 1e-5 * ref["g_norm"], (gn, ref["g_norm"])


def _unet_case(engines, family, name, cfg, counters):
    ref = H.reference(name)
    eng = engines.use(family, ref["params"])
    _configure(eng, cfg)
    before = TC.read_counters(eng)
    loss = float(eng.train_planner_grad(*_unet_inputs(ref["model"], ref["inputs"]), alpha=ref["alpha"]))
    gn = float(eng.train_grad_norm(["planner"]))
    got = eng.train_read("planner", eng.TRAIN_GRADS, engines.shapes(family))
    diff = {k: v - before[k] for k, v in TC.read_counters(eng).items() if v != before[k]}
    if counters:
        TC.check_counters(before, TC.read_counters(eng), *TC.expected("planner", ref["rows"], cfg), f"{name}, {ref['rows']} rows, {cfg}")
    _held_to_the_rule(name, cfg, ref, loss, gn, got, diff)


# ---- A. the trained-like sets against float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cfg", [(n, c) for n in ("ph3", "ph33", "pw3", "pw33") for c in PLANNER_CFGS] + [("ph129", "t128"), ("pw129", "t128")])
def test_planner_tape_on_trained_like_parameters(name, cfg, engines):
    _unet_case(engines, "tape", name, cfg, counters=True)


def test_planner_tape_on_trained_like_parameters_at_16_positions(engines):
    """pred_horizon 16: (sample, group) blocks of 512 values, so gn_fwd / gn_bwd (the generic kernels) run under the defaults."""
    _unet_case(engines, "t16", "p16h3", "t32", counters=False)


@pytest.mark.parametrize("cfg", ["t32", "gn_generic"])
def test_a_constant_group_is_normalised_at_the_ceiling_of_rstd(cfg, engines):
    """Group 0 of ConditionalResidualBlock1D_2/Conv1dBlock_0 sees 8.0 at every one of its 256 values: mean = 8, var = 0 exactly, rstd =
    1 / sqrt(1e-6f) and the gradient of the convolution's output carries the factor 1000 -- in the fast path and in the generic kernel."""
    _unet_case(engines, "tape", "pc3", cfg, counters=True)


@pytest.mark.parametrize("name,cfg", [(n, c) for n in ("ih24", "ih320") for c in IDM_CFGS])
def test_idm_tape_on_trained_like_parameters(name, cfg, engines):
    ref = H.reference(name)
    print(f"IDM rows, case {name}", json.dumps(ref["rows_info"]))
    assert ref["rows_info"]["kept_min"] >= TC.MARGIN_OVER_ROUNDOFF, ref["rows_info"]
    eng = engines.use("tape", ref["params"], "idm")
    _configure(eng, cfg)
    before = TC.read_counters(eng)
    loss = float(_idm_call(eng, ref["inputs"], ref["alpha"]))
    gn = float(eng.train_grad_norm(["idm"]))
    got = eng.train_read("idm", eng.TRAIN_GRADS, engines.shapes("tape", "idm"))
    diff = TC.check_counters(before, TC.read_counters(eng), *TC.expected("idm", ref["rows"], cfg), f"{name}, {ref['rows']} rows, {cfg}")
    _held_to_the_rule(name, cfg, ref, loss, gn, got, {k: v for k, v in diff.items() if v})


@pytest.mark.parametrize("name", ["hh3", "hh40"])
def test_hierarchical_idm_tape_on_trained_like_parameters(name, engines):
    """The two-level U-Net over chunks of 4 actions, through the entry point LDPHierAgent.update trains it with (its IDM handle's
    train_planner_grad), against oracle.train.hier_idm_loss."""
    _unet_case(engines, "hier", name, "t32", counters=False)


@pytest.mark.parametrize("name", ["dh3", "dh33"])
def test_policy_tape_and_condition_gradient_on_trained_like_parameters(name, engines):
    """train_planner_grad_cond on a trained-like DP policy at the condition width of tests/test_hip_dp_train.py: every parameter leaf and
    dcond under the rule (err32 of dcond: float32 autograd with the condition a leaf); loss and gradient arena bitwise train_planner_grad's."""
    ref = H.reference(name)
    eng = engines.use("policy", ref["params"])
    args = _unet_inputs("policy", ref["inputs"])
    assert args[3].shape == (ref["n"], 2066)
    l0 = eng.train_planner_grad(*args, alpha=ref["alpha"])
    g0 = eng.train_arena("planner", eng.TRAIN_GRADS).clone()
    eng.train_arena("planner", eng.TRAIN_GRADS).zero_()
    l1, dcond = eng.train_planner_grad_cond(*args, alpha=ref["alpha"])
    assert torch.equal(l0, l1) and torch.equal(eng.train_arena("planner", eng.TRAIN_GRADS), g0)
    gn = float(eng.train_grad_norm(["planner"]))
    got = eng.train_read("planner", eng.TRAIN_GRADS, engines.shapes("policy"))
    got["dcond"] = dcond.cpu().numpy()
    _held_to_the_rule(name, "t32", ref, float(l1), gn, got)


# ---- C. no IDM row exempt -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pset,i", [(p, i) for p in ("idm", "idm_heavy") for i in range(H.GATE_ROWS)])
def test_no_idm_row_is_exempt(pset, i, engines):
    """A row the selection of part B (or train_cases.idm_rows) drops, alone in a batch of one (32 padded rows): float32 may gate its ambiguous
    ReLU inputs either way, and which way moves the row's whole gradient -- but it must BE the float64 gradient of one of those assignments,
    on every entry of every leaf under the rule."""
    row = H.gate_rows(pset)[i]
    eng = engines.use("tape", pset, "idm")
    loss = float(_idm_call(eng, row["inputs"], 0.7))
    got = eng.train_read("idm", eng.TRAIN_GRADS, engines.shapes("tape", "idm"))
    met, ratios = H.assignment_met(got, loss, row)
    print("train heavy C", json.dumps(dict(params=pset, row=row["row"], margin=row["margin"], gates=row["gates"],
                                           met=None if met is None else {str(k): bool(v) for k, v in row["refs"][met]["gates"].items()},
                                           err_over_bound=ratios)))
    assert all(np.isfinite(g).all() for g in got.values())
    assert met is not None, f"row {row['row']} of the {pset} pool meets no assignment of its gates {row['gates']}: |err| / bound = {ratios}"
