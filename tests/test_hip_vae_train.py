"""StableVAEModel.update on the GPU (ldp_train_vae_grad, module bit 4 of the training calls): gradients against the float64 autograd goldens,
the loss metrics, Adam + EMA over several steps, determinism, publishing the trained weights, the eps keying, snapshots and the ABI.  -m gpu.

Gradient rule (tests/test_hip_stress.py, DESIGN 2, per leaf, with the 1e-12 floor of tests/test_hip_dp_vae.py): every sampled entry of every
leaf satisfies |got - ref64| <= max(1e-4 leafmax64, 3 err32_leaf) + 1e-12, err32 = the leaf's max |float32 autograd - float64| of the same chain.
"""
import json

import numpy as np
import pytest
import torch

from latent_diffusion_planning_amd import _lib, weights as W
from tests import vae_model_oracle as VO
from tests import vae_train_oracle as VT
from tests.golden.make_golden_vae_update import DIGEST_SEED, KEY, golden_path, normalised, params_of, raw_frames
from tests.util import tree_digest

pytestmark = pytest.mark.gpu
K = {k: i for i, k in enumerate(VO.METRIC_KEYS)}
CASES = ("vae_update_seeded_b2", "vae_update_seeded_b33", "vae_update_trained_like_b2", "vae_update_nokl_b2")


def _f32(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32)


def _model(params, ema=None, use_kl=True):
    from latent_diffusion_planning_amd.vae_model import StableVAEModel
    m = StableVAEModel.create(0, None, dict(all_shapes={KEY: [64, 64, 3]}), name="stable_vae_model",
                              vae=dict(latent_channels=4, block_out_channels=[128, 256, 256, 256, 256, 256], layers_per_block=2,
                                       norm_num_groups=32, down_block_types=["DownEncoderBlock2D"] * 6),
                              rgb_obs=[KEY], obs_normalization={"obs": {KEY: dict(min=0, max=255)}}, lr=VT.LR, end_lr=VT.END_LR,
                              warmup_steps=VT.WARMUP, decay_steps=300000, ema_decay=VT.EMA_DECAY, use_kl=use_kl, beta=VT.BETA,
                              data_name="rm_lift")
    return m.replace(vae_state=m.vae_state.replace(params=params, ema_params=params if ema is None else ema))


def _golden(name):
    z = np.load(golden_path(name))
    return z, params_of("trained_like" if int(z["seed_trained_like"]) else "seeded", int(z["seed_params"]))


def _kl_bound(mom_ref, tol):
    """tests/test_hip_vae_model.py: first-order propagation of a moment error `tol` through kl, averaged over the images."""
    lc = mom_ref.shape[-1] // 2
    mean, lv = mom_ref[..., :lc], np.clip(mom_ref[..., lc:], -30, 20)
    return float(np.mean(0.5 * np.sum(2 * np.abs(mean) + np.abs(np.exp(lv) - 1), axis=(1, 2, 3))) * tol)


def _check_metrics(got, z, step=0, beta=VT.BETA, klb=None):
    """The bounds tests/test_hip_vae_model.py applies to get_metrics against the same oracle: reconstruction within 1e-4 and moments within
    5e-5 (the seeded sets), max(1e-4, 3 x the float32 chain's own error) on the trained-like set; the scalars by propagation.  `klb`: the
    bound on loss_kl where the first-order form of _kl_bound does not apply (log-variances outside the clamp)."""
    ref = {k: float(v) for k, v in zip(VO.METRIC_KEYS, z["out_metrics"][step])}
    mom, eps = z["out_moments"], z["out_eps"][step]
    use_kl = bool(int(z["seed_use_kl"]))
    if int(z["seed_trained_like"]):
        tol, tm = max(1e-4, 3 * float(z["out_rec_err32"])), max(1e-4, 3 * float(z["out_mom_err32"])) * max(1.0, float(np.abs(mom).max()))
    else:
        tol, tm = 1e-4, 5e-5
    _, _, std_ref = VO.posterior(mom, eps)
    zb = tm * (1 + 0.5 * float(np.abs(std_ref * eps).max()))
    if klb is None:
        klb = _kl_bound(mom, tm) if use_kl else 0.0
    g = {k: float(got[K[k]]) for k in VO.METRIC_KEYS}
    mb = 2 * np.sqrt(ref["loss_mse"]) * tol + tol * tol
    assert abs(g["loss_mse"] - ref["loss_mse"]) <= mb, (step, g, ref)
    assert abs(g["loss_kl"] - ref["loss_kl"]) <= klb + 1e-6 * ref["loss_kl"], (step, g["loss_kl"], ref["loss_kl"], klb)
    assert abs(g["loss"] - ref["loss"]) <= mb + beta * klb + 1e-6 * ref["loss"], (step, g["loss"], ref["loss"])
    for k in ("img_min", "img_max", "img_mean", "img_std"):
        assert abs(g[k] - ref[k]) <= 1e-6, (k, g[k], ref[k])
    for k in ("z_min", "z_max", "z_mean", "z_std"):
        assert abs(g[k] - ref[k]) <= zb + 1e-6 * abs(ref[k]), (k, g[k], ref[k])
    if not use_kl:
        assert g["loss_kl"] == 0.0 and g["loss"] == g["loss_mse"]


def _assert_digest(got_tree, want, seed, tol, what):
    """tests/test_hip_dp_vae.py: L2 norm, max |x| and the projection 1e-4 relative; the sampled elements absolute."""
    got = tree_digest(got_tree, seed)
    rel = np.abs(got[:, :3] - want[:, :3]) / np.maximum(np.abs(want[:, :3]), 1e-30)
    assert float(rel.max()) < 1e-4, f"{what}: digest statistics off by {float(rel.max()):.3e} relative"
    err = float(np.abs(got[:, 3:] - want[:, 3:]).max())
    assert err < tol, f"{what}: max |diff| {err:.3e}"


def _grads(model):
    eng = model._engine
    return eng.train_read("vae", eng.TRAIN_GRADS, W.vae_shapes(model._vae_spec))


# ---- 1. gradients and the step-0 metrics against the goldens --------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_gradients_and_metrics_match_the_golden(name):
    z, p = _golden(name)
    B, use_kl = int(z["seed_B"]), bool(int(z["seed_use_kl"]))
    model = _model(p, use_kl=use_kl)
    model._train_sync(model.vae_state)
    img = _f32(normalised(raw_frames(int(z["seed_frames"][0]), B))).cuda()
    m = model._engine.train_vae_grad(img, use_kl, VT.BETA, noise=_f32(z["out_eps"][0]).cuda())
    got = tree_digest(_grads(model), DIGEST_SEED)
    ref = z["out_gdig"].astype(np.float64)
    bound = np.maximum(1e-4 * ref[:, 1], 3 * z["out_err32"])[:, None] + 1e-12
    ratio = np.abs(got[:, 3:] - ref[:, 3:]) / bound
    names = list(W.vae_shapes(W.VAESpec()))
    worst = int(ratio.max(axis=1).argmax())
    rel = np.abs(got[:, 3:] - ref[:, 3:]).max(axis=1) / np.maximum(ref[:, 1], 1e-300)
    print(f"vae_update gradients {name}", json.dumps(dict(worst_err_over_bound=float(ratio.max()), leaf=names[worst],
                                                          median_err_over_leafmax=float(np.median(rel)))))
    assert float(ratio.max()) <= 1.0, (name, names[worst], float(ratio.max()))
    _check_metrics(m.cpu().numpy(), z)


# ---- 2. several steps: metrics of every step, Adam + EMA after 1 and 3 steps --------------------------------------------------------------
def test_three_updates_match_adam_and_the_ema():
    z, p = _golden("vae_update_seeded_b2")
    B = int(z["seed_B"])
    model = _model(p)
    for i in range(3):
        batch = {"obs": {KEY: raw_frames(int(z["seed_frames"][i]), B)}}
        model, m = model.update(batch, 0, i, noise=z["out_eps"][i])
        assert list(m) == list(VO.METRIC_KEYS) + ["vae_lr", "vae_step"]
        _check_metrics(np.asarray([float(m[k]) for k in VO.METRIC_KEYS]), z, step=i)
        assert abs(float(m["vae_lr"]) - z["out_lr"][i]) <= 1e-6 * z["out_lr"][i] and m["vae_step"] == i
        assert model.vae_state.step == i + 1
        if i + 1 in (1, 3):
            _assert_digest(model.vae_state.params, z[f"out_pdig{i + 1}"].astype(np.float64), DIGEST_SEED, 1e-5, f"params after {i + 1}")
            _assert_digest(model.vae_state.ema_params, z[f"out_edig{i + 1}"].astype(np.float64), DIGEST_SEED, 1e-5, f"EMA after {i + 1}")


# ---- 3. determinism ------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits():
    z, p = _golden("vae_update_seeded_b33")
    B = int(z["seed_B"])
    model = _model(p)
    model._train_sync(model.vae_state)
    eng = model._engine
    img = _f32(normalised(raw_frames(int(z["seed_frames"][0]), B))).cuda()
    runs = []
    for _ in range(2):
        m = eng.train_vae_grad(img, True, VT.BETA, seed=3)
        runs.append((m.clone(), eng.train_arena("vae", eng.TRAIN_GRADS).clone()))
    torch.cuda.synchronize()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert bool(torch.isfinite(runs[0][1]).all()) and float(runs[0][1].abs().max()) > 0


# ---- 4. the trained weights reach the sampling path ----------------------------------------------------------------------------------
def test_publish_equals_a_fresh_model_with_the_fetched_weights():
    z, p = _golden("vae_update_seeded_b2")
    B = int(z["seed_B"])
    batch = {"obs": {KEY: raw_frames(int(z["seed_frames"][0]), B)}}
    model = _model(p)
    model, _ = model.update(batch, 0, 0, noise=z["out_eps"][0])
    model, _ = model.update(batch, 1, 1)
    gm = model.get_metrics(batch, 5)
    rec = model.reconstruct(batch, 0, KEY)
    a = np.asarray([float(gm[k]) for k in VO.METRIC_KEYS])
    rec_a = np.array(rec)
    fresh = _model({k: np.array(v) for k, v in model.vae_state.params.items()}, {k: np.array(v) for k, v in model.vae_state.ema_params.items()})
    gm2 = fresh.get_metrics(batch, 5)
    b = np.asarray([float(gm2[k]) for k in VO.METRIC_KEYS])
    assert np.array_equal(a, b)
    assert np.array_equal(rec_a, np.array(fresh.reconstruct(batch, 0, KEY)))
    assert not np.array_equal(model.vae_state.params["decoder/conv_out/bias"], p["decoder/conv_out/bias"])


# ---- 5. eps keying: the Philox draw of update is get_metrics' --------------------------------------------------------------------------
def test_row_offset_draws_the_global_frames():
    z, p = _golden("vae_update_seeded_b2")
    B, seed, k = int(z["seed_B"]), 17, 5
    batch = {"obs": {KEY: raw_frames(int(z["seed_frames"][0]), B)}}
    _, m_phil = _model(p).update(batch, seed, 0, row_offset=k)
    eps = VO.philox_eps(seed, B, 16, row_offset=k).reshape(B, 2, 2, 4).astype(np.float32)
    _, m_expl = _model(p).update(batch, 0, 0, noise=eps)
    _, m_zero = _model(p).update(batch, seed, 0, row_offset=0)
    a, b, c = ({q: float(m[q]) for q in VO.METRIC_KEYS} for m in (m_phil, m_expl, m_zero))
    # the device draw is the float32 evaluation of oracle.philox.normal (within 5e-6, tests/test_hip_vae_model.py): z moves by at most std * 5e-6
    for q in ("z_min", "z_max", "z_mean", "z_std"):
        assert abs(a[q] - b[q]) <= 1e-5, (q, a[q], b[q])
    assert abs(a["loss"] - b["loss"]) <= 1e-5 * b["loss"]
    assert max(abs(a[q] - c[q]) for q in ("z_min", "z_max", "z_mean", "z_std")) > 1e-3      # another offset draws other eps


# ---- 6. snapshots ---------------------------------------------------------------------------------------------------------------------
def test_snapshot_of_a_trained_model_round_trips_and_trains_on(tmp_path):
    from latent_diffusion_planning_amd import checkpoint
    z, p = _golden("vae_update_seeded_b2")
    B = int(z["seed_B"])
    batch = {"obs": {KEY: raw_frames(int(z["seed_frames"][0]), B)}}
    model = _model(p)
    for i in range(2):
        model, _ = model.update(batch, i, i)
    path = str(tmp_path / "2.ckpt")
    checkpoint.save_snapshot(model, path)
    back = checkpoint.load_snapshot(_model(p), path)
    for key in p:
        assert np.array_equal(np.asarray(back.vae_state.params[key]), np.asarray(model.vae_state.params[key])), key
        assert np.array_equal(np.asarray(back.vae_state.ema_params[key]), np.asarray(model.vae_state.ema_params[key])), key
    nxt, m = back.update(batch, 2, 2)
    assert np.isfinite(float(m["loss"])) and m["vae_step"] == back.vae_state.step and nxt.vae_state.step == back.vae_state.step + 1


# ---- 7. ABI -----------------------------------------------------------------------------------------------------------------------------
def test_bit4_refusals():
    from latent_diffusion_planning_amd.engine import HipEngine
    e = HipEngine(obs_dim=25, action_dim=7, global_cond_dim=25, pred_horizon=8, action_horizon=4, image_size=0)
    try:
        assert e.lib.ldp_train_init(e._h, 4, e._stream()) == -1                   # LDP_EINVAL: no StableVAE on this handle
        assert b"image_size = 0" in e.lib.ldp_last_error()
    finally:
        e.close()
    model = _model(W.init_vae_params(seed=5))
    model._train_sync(model.vae_state)
    with pytest.raises(_lib.LDPHipError, match="at most 256"):
        model._engine.train_vae_grad(torch.zeros((257, 64, 64, 3), device="cuda"), True, VT.BETA)
    # N = 0 is refused as well (LDP_EINVAL), with valid pointers: it is the count that is refused
    import ctypes as C
    eng = model._engine
    img, out = torch.zeros((1, 64, 64, 3), device="cuda"), torch.zeros((11,), device="cuda")
    code = eng.lib.ldp_train_vae_grad(eng._h, C.c_void_p(img.data_ptr()), 0, 1, C.c_float(VT.BETA), None, C.c_uint64(0), C.c_int64(0),
                                      C.c_void_p(out.data_ptr()), eng._stream())
    assert code == -1 and b"bad argument" in eng.lib.ldp_last_error()
    with pytest.raises(_lib.LDPHipError) as refused:
        eng.train_vae_grad(torch.zeros((0, 64, 64, 3), device="cuda"), True, VT.BETA)
    assert refused.value.code == -1
