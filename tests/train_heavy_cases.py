"""Fixtures of the trained-like training-tape tests (tests/test_hip_train_heavy.py on the GPU, the premises they rest on in
tests/test_train_heavy_cpu.py): the cases, their float64 oracle runs, the float32 restatement of the same gradients that prices the number
format per leaf, the census of the activation tails, the per-unit IDM gate rule and the gate assignments of the rows no rule keeps.
Test infrastructure, NOT a product path.

The oracle's forward (oracle/torch32.py) is written against `torch.nn.functional` under the module-level name `F`.  `FlaxF` stands in for
that name while a loss is evaluated (`functional`): every function is torch's own, except
  * group_norm / layer_norm, restated as flax computes them under use_fast_variance -- var = max(E[x^2] - E[x]^2, 0) -- because
    F.group_norm / F.layer_norm centre first, and a float32 run of THAT form would understate what float32 costs a norm at a large mean;
  * mish, which also records its input (the census);  relu, which can take the gate of listed units as given (part C).
"""
import contextlib
import functools
import itertools
import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import torch32
from oracle import train as OT
from tests import train_cases as TC
from tests.cases import HIER_IDM_DOWN, hier_idm_params_heavy
from tests.train_cases import A, D
from tests.util import PLANNER_STREAM, idm_params, idm_params_heavy, planner_params, planner_params_heavy, rng, trained_like

IH = 4                                     # the hierarchical agent's idm_horizon: action positions of its U-Net IDM
POLICY_T, POLICY_OH = 16, 2                # tests/test_hip_dp_train.py: DPTrainAgent's policy U-Net on rm_img (one camera)
POLICY_SEED = 801                          # the parameter seed of its golden dp_train_update_rm_img_b3
CONST_BLOCK = "ConditionalResidualBlock1D_2/Conv1dBlock_0"       # 256 -> 512 channels at 4 positions: (sample, group) = 4 x 64 values
CONST_GN_CALL = 4                          # its GroupNorm is the fifth of unet_forward (two per residual block)
CONST_VALUE = 8.0


# ---- the oracle's functional namespace, restated where flax differs -------------------------------------------------------------------------
class FlaxF:
    def __init__(self, fast_variance=True, gates=None):
        self.fast_variance, self.gates = fast_variance, gates
        self.mish_inputs, self.gn_stats, self.relu_offset = [], [], 0

    def __getattr__(self, name):
        return getattr(F, name)

    @staticmethod
    def _normalise(x, eps):
        """Over the last axis, as flax's _compute_stats / _normalize with use_fast_variance -> (x hat, mean, var)."""
        mean = x.mean(-1, keepdim=True)
        var = ((x * x).mean(-1, keepdim=True) - mean * mean).clamp_min(0.0)
        return (x - mean) * torch.rsqrt(var + eps), mean, var

    def group_norm(self, x, groups, weight, bias, eps):
        if not self.fast_variance:
            return F.group_norm(x, groups, weight, bias, eps=eps)
        xh, mean, var = self._normalise(x.reshape(x.shape[0], groups, -1), eps)
        self.gn_stats.append((mean.detach()[..., 0], var.detach()[..., 0]))
        return xh.reshape(x.shape) * weight[None, :, None] + bias[None, :, None]

    def layer_norm(self, x, shape, weight, bias, eps):
        if not self.fast_variance:
            return F.layer_norm(x, shape, weight, bias, eps=eps)
        return self._normalise(x, eps)[0] * weight + bias

    def mish(self, x):
        self.mish_inputs.append(x.detach().double().reshape(-1))
        return F.mish(x)

    def relu(self, x):
        """The gate of unit j (counted over the ReLU calls in order, as train_cases.idm_preacts lays them out) is gates[j] where listed, x > 0
        elsewhere."""
        lo, self.relu_offset = self.relu_offset, self.relu_offset + x.shape[-1]
        if not self.gates:
            return F.relu(x)
        mask = x.detach() > 0
        for j, open_ in self.gates.items():
            if lo <= j < lo + x.shape[-1]:
                mask[..., j - lo] = bool(open_)
        return x * mask.to(x.dtype)

    def census(self):
        """Mish inputs of the run: how many, how many above 20, below -20 and below -88, the largest and the smallest."""
        x = torch.cat(self.mish_inputs)
        return dict(n=int(x.numel()), above20=int((x > 20).sum()), below20=int((x < -20).sum()), below88=int((x < -88).sum()),
                    max=float(x.max()), min=float(x.min()))


@contextlib.contextmanager
def functional(f):
    old, torch32.F = torch32.F, f
    try:
        yield f
    finally:
        torch32.F = old


class LeafParams(torch32.TorchParams):
    """TorchParams whose leaves are autograd leaves of `dtype` in the Flax layout: oracle.train.GradParams at either precision."""

    def __init__(self, params, dtype):
        super().__init__(params, dtype=dtype)
        self.leaves = OrderedDict((k, torch.tensor(np.asarray(v, np.float64)).to(dtype).requires_grad_()) for k, v in params.items())

    def t(self, key):
        return self.leaves[key]

    def grads(self):
        return OrderedDict((k, (v.grad if v.grad is not None else torch.zeros_like(v)).double().numpy().copy()) for k, v in self.leaves.items())


def _t64(a):
    return torch.as_tensor(np.asarray(a, np.float64))


def _loss(model, P, c, cond=None):
    """The loss of oracle/train.py for the module family; every input enters in float64 and the forward rounds the noisy sample once
    (unet_forward / idm_forward cast it to P.dtype).  "policy": plan_loss with the condition given as a tensor of its own."""
    if model == "idm":
        emb, act = TC.idm_as_samples(c)
        return OT.idm_loss(P, _t64(emb), _t64(act), c["t"], c["noise"], 1, 100)
    if model == "hier":
        return OT.hier_idm_loss(P, _t64(c["obs_emb"]), _t64(c["actions"]), c["t"], c["noise"], 1, IH, 100, down_dims=HIER_IDM_DOWN)
    if model == "planner":
        return OT.plan_loss(P, _t64(c["obs_emb"]), c["t"], c["noise"], 1, 100)
    assert model == "policy", model
    noise = _t64(c["noise"])
    pred = torch32.unet_forward(P, OT._add_noise(_t64(c["x0"]), noise, c["t"], 100), torch.as_tensor(np.asarray(c["t"]).reshape(-1)), cond)
    return ((pred - noise) ** 2).mean()


def grads32(model, params, case, alpha=1.0, dtype=torch.float32, f=None):
    """alpha * the loss of oracle.train.plan_loss / idm_loss / hier_idm_loss (model "planner" / "idm" / "hier"; "policy": plan_loss with the
    condition a leaf) and its gradients by autograd in `dtype`, float32 unless asked: what the tape's arithmetic costs when nothing but the
    number format differs from the float64 oracle.  The noisy input is computed in float64 and rounded once, as train_cases.idm_preacts
    does.  oracle/torch32.py calls F.group_norm / F.layer_norm, which centre before they square; here both are restated as flax computes
    them under use_fast_variance, max(E[x^2] - E[x]^2, 0) (FlaxF), unless `f` says otherwise.
    -> dict(loss, grads {leaf: float64 array}, f [, dcond])."""
    P = LeafParams(params, dtype)
    cond = torch.tensor(np.asarray(case["cond"], np.float64)).to(dtype).requires_grad_() if model == "policy" else None
    with functional(f or FlaxF()) as f:
        loss = alpha * _loss(model, P, case, cond)
    loss.backward()
    out = dict(loss=float(loss.detach()), grads=P.grads(), f=f)
    if cond is not None:
        out["dcond"] = cond.grad.double().numpy().copy()
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
def planner_case(B, seed, T=TC.T):
    g = rng(seed)
    obs_emb = g.uniform(-1, 1, (B, T + 1, D)).astype(np.float32)
    return dict(obs_emb=obs_emb, t=g.integers(0, 100, B), noise=g.standard_normal((B, T, D)).astype(np.float32))


def hier_case(n, seed):
    """n action chunks as one-chunk samples of hier_idm_loss: obs_emb (n, 1 + IH, D) (the chunk's first and last state are its condition),
    actions (n, 1 + IH, A) (the last one is never read)."""
    g = rng(seed)
    return dict(obs_emb=g.uniform(-1, 1, (n, 1 + IH, D)).astype(np.float32), actions=g.uniform(-1, 1, (n, 1 + IH, A)).astype(np.float32),
                t=g.integers(0, 100, n), noise=g.standard_normal((n, IH, A)).astype(np.float32))


def policy_case(B, seed):
    from tests import dp_resnet_oracle as RO
    g = rng(seed)
    G = RO.cond_dim(RO.RM_IMG, POLICY_OH)
    return dict(x0=g.uniform(-1, 1, (B, POLICY_T, A)).astype(np.float32), cond=g.uniform(-1, 1, (B, G)).astype(np.float32),
                t=g.integers(0, 100, B), noise=g.standard_normal((B, POLICY_T, A)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def params_of(name):
    if name == "planner":
        return planner_params(D=D)
    if name == "planner_heavy":
        return planner_params_heavy(D=D)
    if name == "planner_wide":
        return planner_params_heavy(D=D, wide=True)
    if name == "planner_const":
        return constant_group_params()
    if name == "idm":
        return idm_params(D=D, A=A)
    if name == "idm_heavy":
        return idm_params_heavy(D=D, A=A)
    if name == "hier_heavy":
        return hier_idm_params_heavy(A, D)
    if name in ("policy", "policy_heavy"):
        from tests import dp_resnet_oracle as RO
        p = RO.planner_params(RO.RM_IMG, POLICY_SEED, POLICY_OH)
        return p if name == "policy" else trained_like(p, 1000 + POLICY_SEED, heads=("Conv_0",), out_scale=1.0 / 300.0, keep=PLANNER_STREAM)
    raise KeyError(name)


def constant_group_params():
    """The init-like planner with one GroupNorm group fed a constant: the output channels of group 0 of CONST_BLOCK's convolution have a zero
    kernel and bias 8, so every sum of the group's statistics is exact in float32: mean = 8, var = 0, rstd = 1 / sqrt(1e-6f)."""
    p = {k: np.array(v, np.float32) for k, v in planner_params(D=D).items()}
    cg = p[f"{CONST_BLOCK}/Conv_0/kernel"].shape[-1] // 8
    p[f"{CONST_BLOCK}/Conv_0/kernel"][..., :cg] = 0.0
    p[f"{CONST_BLOCK}/Conv_0/bias"][:cg] = CONST_VALUE
    return p


#   case -> (model, parameter set, plans / rows / chunks / samples, seed, alpha)
CASES = OrderedDict(
    ph3=("planner", "planner_heavy", 3, 953, 1.3), ph33=("planner", "planner_heavy", 33, 983, 1.3), ph129=("planner", "planner_heavy", 129, 1079, 1.3),
    pw3=("planner", "planner_wide", 3, 953, 1.3), pw33=("planner", "planner_wide", 33, 983, 1.3), pw129=("planner", "planner_wide", 129, 1081, 1.3),
    p16h3=("planner", "planner_heavy", 3, 316, 1.3),                       # T = 16: see planner_T
    pc3=("planner", "planner_const", 3, 953, 1.3),
    ih24=("idm", "idm_heavy", 24, 2024, 0.7), ih320=("idm", "idm_heavy", 320, 2320, 0.7),
    hh3=("hier", "hier_heavy", 3, 4005, 1.0), hh40=("hier", "hier_heavy", 40, 4040, 1.0),
    dh3=("policy", "policy_heavy", 3, 5003, 1.0), dh33=("policy", "policy_heavy", 33, 5033, 1.0),
)
# the init-like counterparts of the census: the inputs of the same seeds on the parameters every earlier test of the tape loads
INIT_LIKE = OrderedDict(ph33=("planner", "planner"), hh40=("hier", None), dh33=("policy", "policy"))


def planner_T(name):
    return 16 if name == "p16h3" else TC.T


def inputs_of(name):
    """-> (inputs, dict of the row selection or None)"""
    model, pset, n, seed, _ = CASES[name]
    if model == "planner":
        return planner_case(n, seed, planner_T(name)), None
    if model == "idm":
        return idm_rows_per_unit(params_of(pset), n, seed)
    return (hier_case if model == "hier" else policy_case)(n, seed), None


def oracle64(model, params, c, alpha=1.0, f=None):
    """The float64 reference of a case: oracle.train.loss_and_grads as every other test of the tape calls it (F.group_norm / F.layer_norm in
    float64), run under a FlaxF that only records; the policy, which loss_and_grads does not state, through grads32 in float64 with the
    same F.group_norm.  -> dict(loss, grads, g_norm, f [, dcond])."""
    f = f or FlaxF(fast_variance=False)
    if model == "policy":
        r = grads32(model, params, c, alpha, torch.float64, f)
        r["g_norm"] = math.sqrt(sum(float((g ** 2).sum()) for g in r["grads"].values()))
        return r
    with functional(f):
        if model == "planner":
            T = c["noise"].shape[1]
            r = OT.loss_and_grads(params, None, c["obs_emb"], np.zeros((len(c["t"]), T + 1, A)), t_plan=c["t"], noise_plan=c["noise"], alpha_planner=alpha)
            return dict(loss=r["plan_loss"], grads=r["grads_planner"], g_norm=r["g_norm"], f=f)
        if model == "idm":
            emb, act = TC.idm_as_samples(c)
            r = OT.loss_and_grads(None, params, emb, act, t_idm=c["t"], noise_idm=c["noise"], alpha_idm=alpha)
        else:
            r = OT.loss_and_grads(None, params, c["obs_emb"], c["actions"], t_idm=c["t"], noise_idm=c["noise"], alpha_idm=alpha, idm_horizon=IH,
                                  idm_unet_kw=dict(down_dims=HIER_IDM_DOWN))
        return dict(loss=r["idm_loss"], grads=r["grads_idm"], g_norm=r["g_norm"], f=f)


def err32_of(r32, r64):
    """leaf -> max |g32 - g64| ("dcond" among the leaves where the case has one)"""
    out = OrderedDict((k, float(np.abs(r32["grads"][k] - g).max())) for k, g in r64["grads"].items())
    if "dcond" in r64:
        out["dcond"] = float(np.abs(r32["dcond"] - r64["dcond"]).max())
    return out


@functools.lru_cache(maxsize=2)
def reference(name):
    """case -> its inputs, the float64 oracle run, err32 per leaf and the census; shared by the tests of the case, which run one after
    the other (a planner gradient tree in float64 is a third of a gigabyte: two are kept), and never modified."""
    model, pset, n, seed, alpha = CASES[name]
    torch.set_num_threads(min(16, torch.get_num_threads()))
    params = params_of(pset)
    c, rows_info = inputs_of(name)
    r64 = oracle64(model, params, c, alpha)
    r32 = grads32(model, params, c, alpha)
    out = dict(model=model, params=pset, inputs=c, n=n, rows=-(-n // 32) * 32, alpha=alpha, loss=r64["loss"], grads=r64["grads"], g_norm=r64["g_norm"],
               err32=err32_of(r32, r64), loss32=r32["loss"], rows_info=rows_info, gn_stats32=r32["f"].gn_stats)
    if "dcond" in r64:
        out["dcond"] = r64["dcond"]
    if model != "idm":
        out["census"] = r64["f"].census()
    return out


def floors(ref):
    """leaf -> 3 err32_leaf: the floor the rule of DESIGN 4.11 gives the number format under the 1e-4 of the leaf's largest entry."""
    return {k: 3.0 * v for k, v in ref["err32"].items()}


def worst_err32_over_leafmax(ref):
    """-> (the largest err32_leaf / max|ref64 leaf| of the case, its leaf): the rule's bound is max(1e-4, 3 x this) of the leaf's maximum."""
    leaves = dict(ref["grads"], **({"dcond": ref["dcond"]} if "dcond" in ref else {}))
    worst = max(((ref["err32"][k] / float(np.abs(g).max()), k) for k, g in leaves.items() if np.abs(g).max() > 0), key=lambda x: x[0])
    return worst


def init_like_census(name):
    """The Mish inputs of case `name`'s batch on the init-like parameters of its family."""
    model, pset = INIT_LIKE[name]
    if pset is None:
        from tests.cases import hier_idm_params
        params = hier_idm_params(A, D)
    else:
        params = params_of(pset)
    f = FlaxF(fast_variance=False)
    P = torch32.TorchParams(params, dtype=torch.float64)
    c = inputs_of(name)[0]
    with torch.no_grad(), functional(f):
        _loss(model, P, c, _t64(c["cond"]) if model == "policy" else None)
    return f.census()


# ---- part B: the IDM rows, by a per-unit gate rule ---------------------------------------------------------------------------------------------
def idm_margins(ip, pool):
    """-> (margin (rows,), u64 (rows, units), roundoff (units,)): roundoff_j = the largest |float32 - float64| ReLU input j over the pool's
    rows; a row's margin = min_j |u64_rj| / roundoff_j -- how many times its own round-off the row's closest gate is from zero."""
    u64, u32 = TC.idm_preacts(ip, pool, torch.float64), TC.idm_preacts(ip, pool, torch.float32)
    roundoff = np.maximum(np.abs(u32 - u64).max(axis=0), 1e-300)
    return (np.abs(u64) / roundoff[None, :]).min(axis=1), u64, roundoff


def idm_rows_per_unit(ip, rows, seed):
    """train_cases.idm_rows with each ReLU input held against ITS OWN round-off: on a trained-like set the one global figure is set by the
    x 100 units and rejects rows for the wrong reason.  A pool of 1.5 x rows, the `rows` with the largest margin kept.
    -> (the rows, dict(kept_min: the smallest kept margin, pool_clear: pool rows with a margin >= MARGIN_OVER_ROUNDOFF, gates_differ: float32
    gates of the kept rows that differ from float64's, dead: units that are <= 0 on every kept row, max_abs: the largest |ReLU input|))."""
    assert rows % 2 == 0
    pool = TC.idm_pool(rows * 3 // 2, seed)
    margin, u64, roundoff = idm_margins(ip, pool)
    keep = np.sort(np.argsort(-margin, kind="stable")[:rows])
    u32 = TC.idm_preacts(ip, TC.take_rows(pool, keep), torch.float32)
    info = dict(kept_min=float(margin[keep].min()), pool_clear=int((margin >= TC.MARGIN_OVER_ROUNDOFF).sum()), pool=len(margin),
                gates_differ=int(((u32 > 0) != (u64[keep] > 0)).sum()), dead=int((u64[keep] <= 0).all(axis=0).sum()),
                max_abs=float(np.abs(u64[keep]).max()))
    return TC.take_rows(pool, keep), info


# ---- part C: the rows no rule keeps, one at a time, under every assignment of their ambiguous gates ------------------------------------------------
GATE_ROWS, GATE_POOL, GATE_SEED, MAX_GATES = 8, 480, 2320, 4


@functools.lru_cache(maxsize=None)
def gate_rows(pset):
    """The GATE_ROWS rows of the pool of case i320 / ih320 with the smallest margin, each as a batch of its own.  A row's ambiguous gates are
    the ReLU inputs with |u64| <= 3 roundoff_j; for every assignment of them (open / shut, every other gate computed) the float64 gradient and
    the float32 one under the SAME gates, whose difference is err32 of that assignment.
    -> [dict(row, inputs, margin, gates [(unit, u64, roundoff)], refs [dict(gates, loss, grads, err32)], run32: float32 with its own gates)]"""
    ip = params_of(pset)
    pool = TC.idm_pool(GATE_POOL, GATE_SEED)
    margin, u64, roundoff = idm_margins(ip, pool)
    out = []
    for r in np.argsort(margin, kind="stable")[:GATE_ROWS]:
        c = TC.take_rows(pool, slice(int(r), int(r) + 1))
        units = [int(j) for j in np.nonzero(np.abs(u64[r]) <= 3.0 * roundoff)[0]]
        refs = []
        for bits in itertools.product((False, True), repeat=min(len(units), MAX_GATES)):
            gates = dict(zip(units, bits))
            r64 = grads32("idm", ip, c, 0.7, torch.float64, FlaxF(gates=gates))
            r32 = grads32("idm", ip, c, 0.7, torch.float32, FlaxF(gates=gates))
            refs.append(dict(gates=gates, loss=r64["loss"], grads=r64["grads"], err32=err32_of(r32, r64)))
        out.append(dict(row=int(r), inputs=c, margin=float(margin[r]), gates=[(j, float(u64[r, j]), float(roundoff[j])) for j in units], refs=refs,
                        run32=grads32("idm", ip, c, 0.7)))
    return out


def assignment_met(got, loss, row):
    """The first assignment of the row's ambiguous gates whose float64 gradient `got` meets on every entry of every leaf under the rule
    (and whose loss it meets) -> (its index or None, per assignment the worst |got - ref| / bound)."""
    met, ratios = None, []
    for i, ref in enumerate(row["refs"]):
        worst, bad = TC.every_entry(got, ref["grads"], 1e-4, floor={k: 3.0 * v for k, v in ref["err32"].items()})
        ratios.append(worst["err_over_bound"])
        if met is None and not bad and abs(loss - ref["loss"]) <= 1e-5 * max(1.0, abs(ref["loss"])):
            met = i
    return met, ratios
