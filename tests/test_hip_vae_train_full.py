"""ldp_train_vae_grad (csrc/vae_train.hpp) checked on EVERY entry of every gradient leaf, in every launch shape of its GEMMs.  -m gpu.

A. Whole leaves against the float64 autograd oracle (tests/vae_train_oracle.py) run inside the test, at the smallest batches that reach an
   edge (tests/vae_train_cases.CASES): one live row of 32, the KL backward dominant (beta = 1), use_kl = 0 with a beta it must ignore, and
   log-variances beyond both ends of the clamp.  The rule is the project's (tests/test_hip_vae_train.py), applied to all 41 672 679 entries:
   |got - ref64| <= max(1e-4 leafmax64, 3 err32_leaf) + 1e-12, err32 = the leaf's max |float32 autograd - float64| of the same chain.
B. Batches no oracle can afford (rows = rup(B, 32): 64, 96 and 160): the loss is a mean over frames and nothing couples frames, so
   G(batch) = sum_c (|c| / B) G(chunk c); the chunks have 32 rows, the shape part A pins.  With the default options every one of these
   launches runs the 32-row tile (csrc/train.hip gemm_shape: train_small_wg = 1 << 20, train_big = 0), two, three and five row tiles
   deep; at 96 and 160 rows the same batch is run again on the 64-row tiles (train_small_wg = 0: a half-empty last row tile) and on
   seg_gemm_big (train_big = 1: the weight gradients at 96 rows, all three forms at 160 = 128 + 32 rows), each held per entry against the
   default-option gradient and attested by the handle's launch counters (stat_train_gemm_*).
C. The backward's own Philox draw (eps == NULL) is the forward's, keyed by (seed, row_offset).
D. The global norm and the zero padding of the gradient arena.
"""
import json

import numpy as np
import pytest
import torch

from latent_diffusion_planning_amd import _lib, weights as W
from tests import train_cases as TC
from tests import vae_model_oracle as VO
from tests import vae_train_cases as VC
from tests.golden.make_golden_vae_update import golden_path
from tests.test_hip_vae_train import K, _check_metrics, _f32, _grads, _model

pytestmark = pytest.mark.gpu
NAMES = list(W.vae_shapes(W.VAESpec()))
LOSSES = ("loss", "loss_mse", "loss_kl")


@pytest.fixture(scope="module")
def base_model():
    """One engine for the module: every test loads its parameters into the same arenas.  Closed at the end (the B = 129 tape keeps ~28 GB)."""
    m = _model(W.init_vae_params(seed=5))
    yield m
    torch.cuda.synchronize()
    m._engine.close()


@pytest.fixture(scope="module")
def oracle():
    """case name -> its inputs and the float64 / float32 oracle runs, computed once per module and never modified."""
    cache = {}

    def get(name):
        if name not in cache:
            p, frames, eps, use_kl, beta = VC.case_inputs(name)
            cache[name] = dict(VC.oracle_run(p, frames, eps, use_kl, beta), params=p, frames=frames, eps=eps, use_kl=use_kl, beta=beta)
        return cache[name]
    return get


def _load(base, params):
    m = base.replace(vae_state=base.vae_state.replace(params=params, ema_params=params))
    m._train_sync(m.vae_state)
    return m


def _run(model, frames, use_kl, beta, **eps_args):
    """One gradient call -> (the eleven metrics, the whole gradient tree)."""
    m = model._engine.train_vae_grad(_f32(frames).cuda(), use_kl, beta, **eps_args)
    return m.cpu().numpy().astype(np.float64), _grads(model)


def _where(path, flat):
    """A flat index of a leaf as its coordinates: (tap row, tap column, cin, cout) for a conv kernel, (in, out) for a Dense one."""
    return tuple(int(i) for i in np.unravel_index(int(flat), tuple(W.vae_shapes(W.VAESpec())[path])))


def _assert_every_entry(got, ref, bounds, what):
    """|got - ref| <= bound_leaf on every entry of every leaf; the report names leaf, coordinates and the number of entries over the bound."""
    bad, worst, worst_leaf, rel = [], 0.0, NAMES[0], []
    for k in NAMES:
        g, r = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)
        assert g.shape == r.shape, (k, g.shape, r.shape)
        err = np.abs(g - r)
        ratio = float(err.max()) / bounds[k]
        rel.append(float(err.max()) / max(float(np.abs(r).max()), 1e-300))
        if not ratio <= worst:                                   # (a NaN is the worst)
            worst, worst_leaf = ratio, k
        if not ratio <= 1.0:
            i = int(np.nanargmax(np.where(np.isnan(err), np.inf, err)))
            bad.append(f"{k}{_where(k, i)}: got {g.flat[i]:.9e}, want {r.flat[i]:.9e}, |diff| / bound = {ratio:.3g}; "
                       f"{int((~(err <= bounds[k])).sum())} of {err.size} entries over the bound")
    line = dict(worst_err_over_bound=worst, leaf=worst_leaf, median_err_over_leafmax=float(np.median(rel)))
    print(f"vae_update whole-leaf gradients {what}", json.dumps(line))
    assert not bad, f"{what}: {len(bad)} of {len(NAMES)} leaves over the bound:\n" + "\n".join(bad[:20])
    return line


def _bounds(o):
    return {k: VC.leaf_bound(o["grads"][k], o["err32"][k]) for k in NAMES}


def _as_golden(o):
    """The oracle run in the layout _check_metrics reads from a golden file."""
    return dict(out_metrics=np.asarray([[o["metrics"][k] for k in VO.METRIC_KEYS]]), out_moments=o["moments"], out_eps=o["eps"][None],
                seed_use_kl=int(o["use_kl"]), seed_trained_like=0)


# ---- A. every entry of every leaf against float64 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(VC.CASES))
def test_every_gradient_entry_matches_float64(name, base_model, oracle):
    o = oracle(name)
    model = _load(base_model, o["params"])
    metrics, got = _run(model, o["frames"], o["use_kl"], o["beta"], noise=_f32(o["eps"]).cuda())
    _assert_every_entry(got, o["grads"], _bounds(o), f"case {name} B={len(o['frames'])} use_kl={int(o['use_kl'])} beta={o['beta']:g}")
    if name != "d":
        _check_metrics(metrics, _as_golden(o), beta=o["beta"])
        return
    # the clamp: channels 0 / 1 of the log-variance are outside it, where neither z nor KL depends on them -- the oracle's gradients of
    # their quant_conv column and bias are exact zeros, and so must these be
    lc = VO.latent_channels(o["params"])
    lv = o["moments"][..., lc:]
    assert lv[..., 0].min() > 30 and lv[..., 1].max() < -40 and lv[..., 2:].min() > -29 and lv[..., 2:].max() < 19
    for path, cols in (("quant_conv/bias", got["quant_conv/bias"][lc:lc + 2]), ("quant_conv/kernel", got["quant_conv/kernel"][..., lc:lc + 2])):
        assert not np.any(o["grads"][path][..., lc:lc + 2]) and not np.any(cols), (path, cols)
    # loss_kl ~ 9.7e8 (exp(20) per saturated entry): _kl_bound's first-order form does not apply beyond the clamp; 1e-5 relative instead
    ref_kl = o["metrics"]["loss_kl"]
    assert ref_kl > 1e8 and abs(metrics[K["loss_kl"]] - ref_kl) <= 1e-5 * ref_kl, (metrics[K["loss_kl"]], ref_kl)
    _check_metrics(metrics, _as_golden(o), beta=o["beta"], klb=9e-6 * ref_kl)                # (+ its own 1e-6 ref_kl: 1e-5 relative)


# ---- C. the Philox branch of the backward ------------------------------------------------------------------------------------------------
def test_backward_draws_the_eps_of_the_forward(base_model, oracle):
    """eps == NULL: vae_post_bwd_kernel re-draws eps from (seed, row_offset).  The header promises the bits of ldp_philox_normal at the
    global elements (row_offset + n) * 16 + e, so the whole arena equals the one of the same eps passed explicitly; another row offset
    gives other encoder gradients (at beta = 1 and B = 3 they depend on eps through dz eps std / 2)."""
    from latent_diffusion_planning_amd.engine import philox_normal
    o = oracle("b")
    model = _load(base_model, o["params"])
    eng, img = model._engine, _f32(o["frames"]).cuda()
    B, seed, row = len(o["frames"]), 17, 5

    def call(**kw):
        m = eng.train_vae_grad(img, True, 1.0, **kw).clone()
        return m, eng.train_arena("vae", eng.TRAIN_GRADS).clone()
    m_phil, a_phil = call(seed=seed, row_offset=row)
    tree_phil = _grads(model)
    eps = philox_normal(seed, row * 16, 0, _lib.PHILOX_STREAM_VAE_EPS, B * 16).reshape(B, 2, 2, 4)
    m_expl, a_expl = call(noise=eps)
    assert torch.equal(m_phil, m_expl), (m_phil, m_expl)
    assert torch.equal(a_phil, a_expl), f"{int((a_phil != a_expl).sum())} of {a_phil.numel()} arena entries differ"
    call(seed=seed, row_offset=0)
    tree_zero, bounds = _grads(model), _bounds(o)
    moved = [k for k in NAMES if k.startswith("encoder/") and float(np.abs(tree_phil[k] - tree_zero[k]).max()) > bounds[k]]
    assert moved, "row_offset = 0 and 5 give the same encoder gradients"


# ---- D. global norm, arena padding ---------------------------------------------------------------------------------------------------------
def test_grad_norm_and_arena_padding(base_model):
    p, frames, eps, use_kl, beta = VC.case_inputs("b")
    model = _load(base_model, p)
    eng = model._engine
    _, got = _run(model, frames, use_kl, beta, noise=_f32(eps).cuda())
    gn = float(eng.train_grad_norm(["vae"]))
    sumsq = float(sum(np.sum(np.square(v.astype(np.float64))) for v in got.values()))
    assert abs(gn - np.sqrt(sumsq)) <= 1e-5 * np.sqrt(sumsq), (gn, np.sqrt(sumsq))
    # "padding of the gradient arena is written as zeros": the arena holds the leaves and nothing else
    arena = eng.train_arena("vae", eng.TRAIN_GRADS).clone()
    assert arena.numel() > sum(v.size for v in got.values())                   # (conv_in / conv_out / the latent-side convs are padded to 32)
    assert int(torch.count_nonzero(arena)) == sum(int(np.count_nonzero(v)) for v in got.values())
    a2 = float(arena.double().square().sum())
    assert abs(a2 - sumsq) <= 1e-12 * sumsq, (a2, sumsq)


# ---- B. batch decomposition at the other tile shapes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (33, 70, 129))
def test_batch_gradient_is_the_weighted_sum_of_its_chunks(B, base_model):
    """Rows = rup(B, 32) = 64 (the golden's own batch), 96 and 160 (31 padding rows), all on the 32-row tile, against chunks of at most 32
    frames, per entry:  |G - sum_c w_c G_c| <= 2 max(1e-4, 3 rel32_leaf) leafmax(G) + 1e-12,
    rel32_leaf = err32 / leafmax64 of the committed B = 33 golden (capped at 1 on the two key/bias leaves, whose true gradient is 0: both sides
    are the exact zero there); the factor 2 because each side carries one allowance of the project's rule.
    That rel32 carries over from B = 33 to the other sizes was checked once with the float32 CPU chain (seeded parameters 6, beta = 1,
    B = 65 in chunks 32 + 32 + 1): its residual |G32 - sum w_c G32_c| is at most 0.197 of this bound (on encoder/.../key/bias, whose float32
    autograd value is round-off; median over the leaves 0.0056).  In float64 the identity holds to 2e-14 of the leaf maximum.
    At 96 and 160 rows the batch then runs on the 64-row tiles and on seg_gemm_big, against the default-option gradient under the same bound."""
    z = np.load(golden_path("vae_update_seeded_b33"))
    assert int(z["seed_params"]) == 6 and int(z["seed_B"]) == 33
    rel32 = np.minimum(z["out_err32"] / np.maximum(z["out_gdig"][:, 1].astype(np.float64), 1e-300), 1.0)
    model = _load(base_model, W.init_vae_params(seed=6))
    frames, eps = VC.frames_and_eps(B)
    if B == 33:
        assert np.array_equal(eps, z["out_eps"][0].astype(np.float32))         # the golden's own batch
    eng = model._engine
    c0 = TC.read_counters(eng)
    m_full, g_full = _run(model, frames, True, 1.0, noise=_f32(eps).cuda())
    TC.check_counters(c0, TC.read_counters(eng), {"nn_32", "nt_32", "tn_32"}, {k for k in TC.KERNELS if k not in ("nn_32", "nt_32", "tn_32")},
                      f"batch {B}, default options")
    chunks, m_comb = [], np.zeros(11)
    for lo in range(0, B, 32):
        hi = min(lo + 32, B)
        m_c, g_c = _run(model, frames[lo:hi], True, 1.0, noise=_f32(eps[lo:hi]).cuda())
        chunks.append((hi - lo, g_c))
        m_comb += (hi - lo) / B * m_c
    comb = VC.combine(chunks)
    bounds = {k: 2 * max(1e-4, 3 * float(rel32[i])) * float(np.abs(g_full[k]).max()) + 1e-12 for i, k in enumerate(NAMES)}
    _assert_every_entry(g_full, comb, bounds, f"batch {B} (rows {-(-B // 32) * 32}) against its chunks of 32")
    for k in NAMES:
        if k.endswith("attentions_0/key/bias"):
            assert not np.any(g_full[k]) and not np.any(comb[k]), k
    assert np.isfinite(m_full).all() and float(sum(np.abs(v).max() for v in g_full.values())) > 0
    for k in LOSSES:
        assert abs(m_full[K[k]] - m_comb[K[k]]) <= 1e-5 * abs(m_comb[K[k]]), (k, m_full[K[k]], m_comb[K[k]])
    if B == 33:
        return
    # the same batch on the other tile families: convolutions have M = the rows (forward, data gradient) or M = cin (weight gradient); 128- and
    # 256-channel layers on both sides, so the 128-row tile needs 128 rows for NN / NT and runs for TN at any batch
    rows = -(-B // 32) * 32
    for cfg in ("t64", "t128"):
        opt = TC.options(cfg)
        big = {f"{f}_128" for f, M in (("nn", rows), ("nt", rows), ("tn", 128)) if TC.gemm_shape(M, 128, 1, 8, opt)[0] == 128}
        must = {"nn_64", "nt_64", "tn_64"} if cfg == "t64" else big | {f"{f}_32" for f in TC.FORMS if f"{f}_128" not in big}
        never = {k for k in TC.KERNELS if "_32" in k} if cfg == "t64" else {k for k in TC.KERNELS if "_64" in k}
        before = {k: eng.get_option(k) for k in TC.CONFIGS[cfg]}
        try:
            for k, v in TC.CONFIGS[cfg].items():
                eng.set_option(k, v)
            c0 = TC.read_counters(eng)
            m_cfg, g_cfg = _run(model, frames, True, 1.0, noise=_f32(eps).cuda())
            TC.check_counters(c0, TC.read_counters(eng), must, never, f"batch {B}, {cfg}")
        finally:
            for k, v in before.items():
                eng.set_option(k, v)
        _assert_every_entry(g_cfg, g_full, bounds, f"batch {B} (rows {rows}) under {cfg} against the default options")
        for k in LOSSES:
            assert abs(m_cfg[K[k]] - m_full[K[k]]) <= 1e-5 * abs(m_full[K[k]]), (cfg, k, m_cfg[K[k]], m_full[K[k]])
