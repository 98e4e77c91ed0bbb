"""StableVAEModel on the GPU: moments, the posterior kernel, the loss / statistics reductions, ldp_vae_metrics end to end against the
float64 goldens, the model class (params vs ema_params, cameras on the batch axis, snapshots) and harness.eval_vae_metrics.  -m gpu."""
import json

import numpy as np
import pytest
import torch

from latent_diffusion_planning_amd import _lib, weights as W
from oracle import philox
from tests import vae_model_oracle as VO
from tests.golden.make_golden_vae_model import (BETA, EMA_SEED, KEY, KEY2, PARAMS_SEED, eps_of, golden_path, normalised, raw_frames,
                                                sample_latents)
from tests.util import assert_close, rng

pytestmark = pytest.mark.gpu
K = {k: i for i, k in enumerate(VO.METRIC_KEYS)}


def _f32(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32)


@pytest.fixture(scope="module")
def vae_params():
    return W.init_vae_params(seed=PARAMS_SEED)


@pytest.fixture(scope="module")
def eng(vae_params):
    from latent_diffusion_planning_amd.engine import HipEngine
    e = HipEngine(obs_dim=25, action_dim=7, global_cond_dim=25, pred_horizon=8, action_horizon=4)
    e.load_params(vae=vae_params)
    yield e
    e.close()


def _model(params=None, ema=None, rgb_obs=(KEY,), use_kl=True, beta=BETA):
    from latent_diffusion_planning_amd.vae_model import StableVAEModel
    norm = {"obs": {KEY: dict(min=0, max=255), KEY2: dict(min=0, max=255)}}
    m = StableVAEModel.create(0, None, dict(all_shapes={KEY: [64, 64, 3], KEY2: [64, 64, 3]}), name="stable_vae_model",
                              vae=dict(latent_channels=4, block_out_channels=[128, 256, 256, 256, 256, 256], layers_per_block=2,
                                       norm_num_groups=32, down_block_types=["DownEncoderBlock2D"] * 6),
                              rgb_obs=list(rgb_obs), obs_normalization=norm, lr=1e-4, end_lr=1e-6, warmup_steps=10, decay_steps=100,
                              ema_decay=0.99, use_kl=use_kl, beta=beta, data_name="rm_lift")
    if params is not None:
        m = m.replace(vae_state=m.vae_state.replace(params=params, ema_params=params if ema is None else ema))
    return m


# ---- 1. moments ------------------------------------------------------------------------------------------------------------------
def test_moments_mean_channels_are_vae_encode_bitwise_and_match_oracle(eng, vae_params):
    img = rng(11).uniform(-1, 1, (3, 64, 64, 3))
    x = _f32(img).cuda()
    mom, mean = eng.vae_moments(x), eng.vae_encode(x)
    torch.cuda.synchronize()
    assert mom.shape == (3, 2, 2, 8)
    assert torch.equal(mom[..., :4], mean)
    ref = VO.moments(vae_params, img)
    assert_close(mom.cpu().numpy(), ref, 5e-5, "moments vs float64 oracle (the encode bound of tests/test_hip_vae.py:139)")


# ---- 2. posterior kernel on hand-made moments -----------------------------------------------------------------------------------------
def _hand_moments(N, seed):
    g = rng(seed)
    mom = np.concatenate([g.normal(0, 2, (N, 2, 2, 4)), g.uniform(-8, 4, (N, 2, 2, 4))], axis=-1)
    mom[0, 0, 0, 4:] = [-40.0, -30.0, 0.0, 20.0]                    # the clamp cases of the issue: below, at, inside, at, above
    mom[0, 0, 1, 4] = 25.0
    return mom.astype(np.float32)


def test_posterior_matches_float64_including_the_clamp(eng):
    N = 70                                                              # 16 images per block: five blocks, the last one ragged
    mom, eps = _hand_moments(N, 21), rng(22).standard_normal((N, 2, 2, 4)).astype(np.float32)
    z, std, kl, stats = eng.vae_posterior(_f32(mom).cuda(), noise=_f32(eps).cuda())
    zr, klr, stdr = VO.posterior(mom, eps)
    z, std, kl, stats = z.cpu().numpy(), std.cpu().numpy(), kl.cpu().numpy(), stats.cpu().numpy()
    # fp32: expf within 2 ulp, one product and one sum -> a few ulp (6e-8 each) of the largest term; 1e-6 leaves ~4x
    mean, lv = mom[..., :4].astype(np.float64), np.clip(mom[..., 4:].astype(np.float64), -30, 20)
    assert (np.abs(std - stdr) <= 1e-6 * stdr).all()
    assert (np.abs(z - zr) <= 1e-6 * (np.abs(mean) + np.abs(stdr * eps) + 1)).all()
    scale = 0.5 * np.sum(mean ** 2 + np.exp(lv) + 1 + np.abs(lv), axis=(1, 2, 3))
    assert (np.abs(kl - klr) <= 1e-6 * scale).all(), float((np.abs(kl - klr) / scale).max())
    assert std[0, 0, 0, 0] == np.float32(np.exp(-15.0)) or abs(std[0, 0, 0, 0] / np.exp(-15.0) - 1) < 1e-6   # logvar -40 -> -30
    assert abs(std[0, 0, 1, 0] / np.exp(10.0) - 1) < 1e-6                                                    # logvar 25 -> 20
    z64 = z.astype(np.float64)
    for got, want in zip(stats, (z64.min(), z64.max(), z64.mean(), z64.std())):
        assert abs(got - want) <= 1e-5 * abs(want), (stats, want)


def test_posterior_philox_equals_explicit_noise_and_shards_equal_the_whole(eng):
    N, seed = 70, 1234567
    mom = _f32(_hand_moments(N, 23)).cuda()
    from latent_diffusion_planning_amd.engine import philox_normal
    zp, _, klp, sp = eng.vae_posterior(mom, seed=seed)
    eps = philox_normal(seed, 0, 0, _lib.PHILOX_STREAM_VAE_EPS, N * 16).reshape(N, 2, 2, 4)
    ze, _, kle, se = eng.vae_posterior(mom, noise=eps)
    torch.cuda.synchronize()
    assert torch.equal(zp, ze) and torch.equal(klp, kle) and torch.equal(sp, se)
    # the device eps is the float32 evaluation of oracle.philox.normal at (seed, element, step 0, stream 9)
    assert np.abs(eps.cpu().numpy().reshape(-1) - philox.normal(seed, 0, 0, VO.STREAM_VAE_EPS, N * 16)).max() < 5e-6
    a = eng.vae_posterior(mom[:33].contiguous(), seed=seed, row_offset=0)
    b = eng.vae_posterior(mom[33:].contiguous(), seed=seed, row_offset=33)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([a[0], b[0]]), zp) and torch.equal(torch.cat([a[2], b[2]]), klp)
    # a shifted batch draws the global rows: rows 5.. of the whole == a batch that starts at row_offset 5
    c = eng.vae_posterior(mom[5:25].contiguous(), seed=seed, row_offset=5)
    assert torch.equal(c[0], zp[5:25])


# ---- 3. the reductions in isolation -------------------------------------------------------------------------------------------------
def _scalars_from_device_tensors(img, z, rec, mom, use_kl, beta):
    _, kl, _ = VO.posterior(mom, np.zeros(z.shape))
    return VO.metrics_from(img, z, kl, rec, use_kl, beta)


def _check_scalars(got, want, rel, what, std_rel=None):
    print(what, json.dumps({k: [float(got[K[k]]), want[k]] for k in VO.METRIC_KEYS}))
    for k in VO.METRIC_KEYS:
        tol = std_rel if (std_rel is not None and k == "img_std") else rel
        assert abs(float(got[K[k]]) - want[k]) <= tol * abs(want[k]), f"{what}: {k} got {float(got[K[k]])!r} want {want[k]!r} (rel {tol})"


@pytest.mark.parametrize("N", [3, 300])
def test_metric_scalars_match_float64_of_the_device_tensors(eng, N):
    """Every scalar against its float64 value computed FROM THE DEVICE's z and reconstruction, relative 1e-5: blocked summation of
    n = 256 * 12288 = 3.1 M terms has a relative error of order log2(n) * 2^-24 = 1.3e-6 (the kernels accumulate in float64, so only the
    final rounding to float32 is left); 1e-5 is ~8x that.  N = 300 crosses the 256-image chunk."""
    img = rng(31 + N).uniform(-1, 1, (N, 64, 64, 3)).astype(np.float32)
    eps = rng(32 + N).standard_normal((N, 2, 2, 4)).astype(np.float32)
    x = _f32(img).cuda()
    m1, ex = eng.vae_metrics(x, True, 0.5, noise=_f32(eps).cuda(), want=("z", "rec"))
    m2, ex2 = eng.vae_metrics(x, True, 0.5, noise=_f32(eps).cuda(), want=("z", "rec"))
    m3, _ = eng.vae_metrics(x, True, 0.5, noise=_f32(eps).cuda())            # without the optional outputs: internal buffers
    mom = eng.vae_moments(x)
    torch.cuda.synchronize()
    assert torch.equal(m1, m2) and torch.equal(ex["z"], ex2["z"]) and torch.equal(ex["rec"], ex2["rec"]), "run-to-run bits differ"
    assert torch.equal(m1, m3)
    assert ex["z"].shape == (N, 2, 2, 4) and ex["rec"].shape == (N, 3, 64, 64)
    # z is the posterior kernel's draw from these moments
    zr, _, _ = VO.posterior(mom.cpu().numpy(), eps)
    assert np.abs(ex["z"].cpu().numpy() - zr).max() < 1e-5
    want = _scalars_from_device_tensors(img, ex["z"].cpu().numpy(), ex["rec"].cpu().numpy(), mom.cpu().numpy(), True, 0.5)
    _check_scalars(m1.cpu().numpy(), want, 1e-5, f"N={N}")


def test_nearly_constant_frame_keeps_its_standard_deviation(eng):
    """0.9 + 1e-3 * noise: the variance (1e-6) is far below fp32 round-off of the mean square (0.81 * 6e-8 per element summed raw loses
    it: the raw sum-of-squares form is off by 15 % here).  The centred accumulation gives ~1e-6; the bound is 1e-4 on purpose."""
    N = 3
    img = (0.9 + 1e-3 * rng(41).standard_normal((N, 64, 64, 3))).astype(np.float32)
    eps = rng(42).standard_normal((N, 2, 2, 4)).astype(np.float32)
    x = _f32(img).cuda()
    m, ex = eng.vae_metrics(x, True, 0.5, noise=_f32(eps).cuda(), want=("z", "rec"))
    mom = eng.vae_moments(x)
    want = _scalars_from_device_tensors(img, ex["z"].cpu().numpy(), ex["rec"].cpu().numpy(), mom.cpu().numpy(), True, 0.5)
    _check_scalars(m.cpu().numpy(), want, 1e-5, "nearly constant frame", std_rel=1e-4)


# ---- 4. end to end against the golden ---------------------------------------------------------------------------------------------
def _kl_bound(mom_ref, tol):
    """First-order propagation of a moment error `tol` through kl = 0.5 sum(mean^2 + exp(lv) - 1 - lv), averaged over the images:
    |d kl_n| <= 0.5 sum(2 |mean| + |exp(lv) - 1|) tol."""
    lc = mom_ref.shape[-1] // 2
    mean, lv = mom_ref[..., :lc], np.clip(mom_ref[..., lc:], -30, 20)
    return float(np.mean(0.5 * np.sum(2 * np.abs(mean) + np.abs(np.exp(lv) - 1), axis=(1, 2, 3))) * tol)


def test_get_metrics_matches_the_golden_in_both_arithmetic_forms(vae_params):
    """Reconstruction within 1e-4 of the float64 oracle with vae_split = 0 (exact-fp32 MFMA); with the default split-operand convolutions
    at most max(2 x the exact run's error, 1e-5) and below 1e-4 (the rule of tests/test_hip_vae.py:138-139).  Scalar bounds follow from
    the element tolerances: |d mse| <= 2 sqrt(mse) tol + tol^2, loss_kl by first-order propagation of the moment tolerance (5e-5)."""
    g = np.load(golden_path("vae_model_metrics_b3"))
    ref = {k: float(v) for k, v in zip(VO.METRIC_KEYS, g["out_metrics"])}
    B = g["out_z"].shape[0]
    raw, eps = raw_frames(int(g["seed_frames"]), B), eps_of(int(g["seed_eps"]), B)
    model = _model(vae_params)
    eng = model._engine
    img = model._frames({"obs": {KEY: raw}}, [KEY])
    assert np.abs(img.cpu().numpy() - normalised(raw)).max() < 3e-7
    errs = {}
    try:
        for tag, split in (("fp32_mfma", 0), ("split_default", 1)):
            eng.set_option("vae_split", split)
            model._sync_weights(use_ema=False)
            m, ex = eng.vae_metrics(img, True, BETA, noise=_f32(eps).cuda(), want=("z", "rec"))
            mom = eng.vae_moments(img)
            errs[tag] = dict(rec=float(np.abs(ex["rec"].cpu().numpy() - g["out_rec"]).max()),
                             z=float(np.abs(ex["z"].cpu().numpy() - g["out_z"]).max()),
                             moments=float(np.abs(mom.cpu().numpy() - g["out_moments"]).max()),
                             metrics={k: float(m[i]) for i, k in enumerate(VO.METRIC_KEYS)})
    finally:
        eng.set_option("vae_split", 1)
    print("vae_model golden errors", json.dumps(errs))
    exact, split = errs["fp32_mfma"], errs["split_default"]
    # z = mean + exp(lv / 2) eps: a moment error t moves z by at most t (1 + |std eps| / 2) to first order
    _, _, std_ref = VO.posterior(g["out_moments"], eps)
    zb = 5e-5 * (1 + 0.5 * float(np.abs(std_ref * eps).max()))
    assert exact["rec"] <= 1e-4 and exact["moments"] <= 5e-5 and exact["z"] <= zb, errs
    assert split["rec"] <= max(2 * exact["rec"], 1e-5) and split["rec"] < 1e-4, errs
    assert split["moments"] <= 5e-5 and split["z"] <= zb, errs
    tol = 1e-4
    for tag in errs:
        got = errs[tag]["metrics"]
        assert abs(got["loss_mse"] - ref["loss_mse"]) <= 2 * np.sqrt(ref["loss_mse"]) * tol + tol * tol, (tag, got, ref)
        klb = _kl_bound(g["out_moments"], 5e-5)
        assert abs(got["loss_kl"] - ref["loss_kl"]) <= klb + 1e-6 * ref["loss_kl"], (tag, got["loss_kl"], ref["loss_kl"], klb)
        assert abs(got["loss"] - ref["loss"]) <= 2 * np.sqrt(ref["loss_mse"]) * tol + tol * tol + BETA * klb + 1e-6 * ref["loss"]
        for k in ("img_min", "img_max", "img_mean", "img_std"):       # inputs normalised in fp32 (3e-7 per element)
            assert abs(got[k] - ref[k]) <= 1e-6, (k, got[k], ref[k])
        for k in ("z_min", "z_max", "z_mean", "z_std"):
            assert abs(got[k] - ref[k]) <= zb + 1e-6 * abs(ref[k]), (k, got[k], ref[k])
    # the model's own call (default arithmetic) returns the same eleven scalars
    mm = model.get_metrics({"obs": {KEY: raw}}, 0, noise=eps)
    assert list(mm) == list(VO.METRIC_KEYS)
    for k in VO.METRIC_KEYS:
        assert float(mm[k]) == split["metrics"][k], k


def test_trained_like_weights_through_the_composed_chain():
    """A heavy-tailed set (norm scales over four decades, O(10) biases, x100 channels; activations ~5e3) whose log-variance head was
    scaled into the fixture condition.  Bounds by the rule of tests/test_hip_stress.py: max(1e-4, 3 x the float32 restatement's own
    error), on max|d| / max(1, |ref|); the scalars from the element bounds as above."""
    from tests.util import rel_err
    B = 2
    x = rng(4244).uniform(-1, 1, (B, 64, 64, 3)).astype(np.float32)
    eps = eps_of(4245, B)
    params, _ = VO.trained_like_params(2, x.astype(np.float64))
    m64, z64, r64, mom64 = VO.loss(params, x, eps, True, BETA)
    lv = mom64[..., 4:]
    assert -8 <= lv.min() and lv.max() <= 4
    m32, z32, r32, mom32 = VO.float32_chain(params, x, eps, True, BETA)
    floor = dict(moments=rel_err(mom32, mom64), z=rel_err(z32, z64), rec=rel_err(r32, r64))
    model = _model(params)
    model._sync_weights(use_ema=False)
    eng = model._engine
    m, ex = eng.vae_metrics(_f32(x).cuda(), True, BETA, noise=_f32(eps).cuda(), want=("z", "rec"))
    mom = eng.vae_moments(_f32(x).cuda())
    assert eng.poll_fault_kinds() == 0, "the in-range trained-like set must not trip the range guard"
    got = dict(moments=rel_err(mom.cpu().numpy(), mom64), z=rel_err(ex["z"].cpu().numpy(), z64), rec=rel_err(ex["rec"].cpu().numpy(), r64))
    m = m.cpu().numpy()
    print("trained-like", json.dumps(dict(float32_floor=floor, hip=got, loss_mse=[float(m[K["loss_mse"]]), m64["loss_mse"]],
                                          loss_kl=[float(m[K["loss_kl"]]), m64["loss_kl"]])))
    bound = {k: max(1e-4, 3.0 * floor[k]) for k in floor}
    for k in got:
        assert got[k] <= bound[k], (k, got, floor)
    tol = bound["rec"] * max(1.0, float(np.abs(r64).max()))
    assert abs(m[K["loss_mse"]] - m64["loss_mse"]) <= 2 * np.sqrt(m64["loss_mse"]) * tol + tol * tol
    klb = _kl_bound(mom64, bound["moments"] * max(1.0, float(np.abs(mom64).max())))
    assert abs(m[K["loss_kl"]] - m64["loss_kl"]) <= klb + 1e-6 * m64["loss_kl"]


# ---- 5. use_kl = False ---------------------------------------------------------------------------------------------------------------
def test_without_kl_the_kl_term_is_exactly_zero(eng):
    img = _f32(rng(51).uniform(-1, 1, (2, 64, 64, 3))).cuda()
    m = eng.vae_metrics(img, False, 0.3, seed=5)[0].cpu().numpy()
    on = eng.vae_metrics(img, True, 0.3, seed=5)[0].cpu().numpy()
    assert m[K["loss_kl"]] == 0.0 and m[K["loss"]] == m[K["loss_mse"]]
    assert on[K["loss_kl"]] > 0 and on[K["loss"]] > on[K["loss_mse"]] and on[K["loss_mse"]] == m[K["loss_mse"]]


# ---- 6. params vs ema_params ------------------------------------------------------------------------------------------------------------
def test_reconstruct_reads_the_ema_and_get_metrics_the_params(vae_params):
    """The two sets differ; each call matches ITS golden.  One engine slot holds one set: a switch uploads the set that is needed once,
    and repeated calls of one kind upload nothing (counted on the model, which compares the engine's version token)."""
    ema = W.init_vae_params(seed=EMA_SEED)
    model = _model(vae_params, ema)
    gm, gr = np.load(golden_path("vae_model_metrics_b3")), np.load(golden_path("vae_model_reconstruct_b2"))
    raw_m, eps = raw_frames(int(gm["seed_frames"]), 3), eps_of(int(gm["seed_eps"]), 3)
    raw_r = raw_frames(int(gr["seed_frames"]), 2)
    assert model.uploads == 0
    m = model.get_metrics({"obs": {KEY: raw_m}}, 0, noise=eps)
    mse_ref = float(gm["out_metrics"][K["loss_mse"]])
    assert abs(float(m["loss_mse"]) - mse_ref) <= 2 * np.sqrt(mse_ref) * 1e-4 + 1e-8       # the bound of the end-to-end test
    assert model.uploads == 1
    float(model.get_metrics({"obs": {KEY: raw_m}}, 1)["loss"])
    assert model.uploads == 1, "a loop of get_metrics calls uploads nothing"
    rec = model.reconstruct({"obs": {KEY: raw_r}}, 0, KEY)
    assert rec.shape == (2, 3, 64, 64)
    assert_close(np.array(rec), gr["out_rec"], 1e-4, "reconstruct vs golden (ema_params)")
    assert model.uploads == 2
    np.array(model.reconstruct({"obs": {KEY: raw_r}}, 0, KEY))
    assert model.uploads == 2
    m2 = model.get_metrics({"obs": {KEY: raw_m}}, 0, noise=eps)
    assert float(m2["loss_mse"]) == float(m["loss_mse"]) and model.uploads == 3


# ---- 7. sample -----------------------------------------------------------------------------------------------------------------------
def test_sample_decodes_the_philox_latents_on_the_ema(vae_params):
    g = np.load(golden_path("vae_model_sample"))
    model = _model(vae_params, W.init_vae_params(seed=int(g["seed_params"])))
    img = model.sample(int(g["seed_rng"]))
    assert img.shape == (4, 3, 64, 64)
    # (the golden's latents are the float64 Box-Muller of the same Philox words: 5e-6 apart from the device's float32 ones)
    assert_close(np.array(img), g["out_img"], 1e-4, "sample vs oracle decode of the same Philox latents")
    again = model.sample(int(g["seed_rng"]), noise=sample_latents(int(g["seed_rng"])).astype(np.float32))
    assert_close(np.array(again), g["out_img"], 1e-4, "sample with explicit latents")


# ---- 8. two cameras ------------------------------------------------------------------------------------------------------------------
def test_two_cameras_are_the_2b_frame_batch(vae_params):
    B = 2
    a, b = raw_frames(61, B), raw_frames(62, B)
    eps = eps_of(63, 2 * B)
    two = _model(vae_params, rgb_obs=(KEY, KEY2))
    one = _model(vae_params, rgb_obs=(KEY,))
    m2 = two.get_metrics({"obs": {KEY: a, KEY2: b}}, 0, noise=eps)
    m1 = one.get_metrics({"obs": {KEY: np.concatenate([a, b], axis=0)}}, 0, noise=eps)
    for k in VO.METRIC_KEYS:
        assert float(m2[k]) == float(m1[k]), k


# ---- 9. snapshots --------------------------------------------------------------------------------------------------------------------
def test_snapshot_round_trip_and_vae_pretrain_path(tmp_path, vae_params):
    from latent_diffusion_planning_amd import checkpoint
    from latent_diffusion_planning_amd.agent import LDPAgent
    from tests import cfgs
    ema = W.init_vae_params(seed=EMA_SEED)
    model = _model(vae_params, ema)
    path = str(tmp_path / "100.ckpt")
    checkpoint.save_snapshot(model, path)
    back = checkpoint.load_snapshot(_model(), path)
    for k in vae_params:
        assert np.array_equal(back.vae_state.params[k], vae_params[k]) and np.array_equal(back.vae_state.ema_params[k], ema[k])
    data = cfgs.RM_LIFT
    from_path = LDPAgent.create(0, None, data["shape_meta"], **{**cfgs.agent_kwargs(data), "vae_pretrain_path": path})
    direct = LDPAgent.create(0, None, data["shape_meta"], vae_params=vae_params, **cfgs.agent_kwargs(data))
    raw = raw_frames(71, 2)
    za = from_path.vae_encode({"agentview_image": raw})
    zb = direct.vae_encode({"agentview_image": raw})
    ka = [k for k in za if k.startswith("latent_")][0]
    assert np.array_equal(np.array(za[ka]), np.array(zb[ka]))


# ---- 10. harness ---------------------------------------------------------------------------------------------------------------------
def test_eval_vae_metrics_is_the_mean_over_batches(vae_params):
    from latent_diffusion_planning_amd.harness import eval_vae_metrics
    model = _model(vae_params)
    batches = [{"obs": {KEY: raw_frames(81 + i, 2)}} for i in range(3)]
    out = eval_vae_metrics(model, batches, 9)
    single = [model.get_metrics(b, 9 + i) for i, b in enumerate(batches)]
    assert sorted(out) == sorted(f"evaldata/{k}" for k in VO.METRIC_KEYS)
    for k in VO.METRIC_KEYS:
        assert out[f"evaldata/{k}"] == float(np.mean([float(m[k]) for m in single])), k
    assert len(eval_vae_metrics(model, batches, 9, max_batches=2)) == 11
