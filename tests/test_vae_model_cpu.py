"""StableVAEModel without a GPU: the float64 oracle against an independent float32 evaluation, the goldens against the oracle, `create`'s
checks, the host logic of the model class (frames on the batch axis, get_params / replace, update), snapshots, eval_vae_metrics and the
Philox layout of the posterior's eps."""
import numpy as np
import pytest
import torch

from latent_diffusion_planning_amd import _lib, checkpoint, weights as W
from latent_diffusion_planning_amd.dp_vae_agent import DPState
from latent_diffusion_planning_amd.vae_model import PHILOX_STREAM_VAE_SAMPLE, StableVAEModel
from oracle import philox
from tests import cases, vae_model_oracle as VO
from tests.golden import make_golden_vae_model as G
from tests.util import rng

KEY, KEY2 = G.KEY, G.KEY2
NORM = {"obs": {KEY: dict(min=0, max=255), KEY2: dict(min=0, max=255)}}
VAE_CFG = dict(act_fn="silu", block_out_channels=[128, 256, 256, 256, 256, 256], down_block_types=["DownEncoderBlock2D"] * 6,
               in_channels=3, latent_channels=4, layers_per_block=2, norm_num_groups=32, out_channels=3, sample_size=84,
               scaling_factor=0.18215, up_block_types=["UpDecoderBlock2D"] * 6)


def _kw(**over):
    kw = dict(name="stable_vae_model", vae=dict(VAE_CFG), rgb_obs=[KEY], obs_normalization=NORM, lr=1e-4, end_lr=1e-6, warmup_steps=10,
              decay_steps=100, ema_decay=0.99, use_kl=True, beta=1e-5, data_name="rm_lift")
    kw.update(over)
    return kw


SHAPES = dict(all_shapes={KEY: [64, 64, 3], KEY2: [64, 64, 3]})


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------
def test_oracle_agrees_with_an_independent_float32_evaluation():
    """Measured when the fixture was chosen: reconstruction within 1.34e-5 (scale 3.1), z within 4.3e-6, moments within 3.7e-6,
    loss_mse relative 2e-7, loss_kl relative 6e-7.  The bounds here are 1e-4 / 5e-5 (what the GPU tests grant the HIP path) and 1e-5
    relative on the scalars (float32 evaluation of a float64 definition)."""
    params = cases.vae_params()
    x = rng(4242).uniform(-1, 1, (3, 64, 64, 3))
    eps = rng(4243).standard_normal((3, 2, 2, 4)).astype(np.float32)
    m64, z64, r64, mom64 = VO.loss(params, x, eps, True, 1e-5)
    m32, z32, r32, mom32 = VO.float32_chain(params, x, eps, True, 1e-5)
    lv = mom64[..., 4:]
    assert G.LOGVAR_RANGE[0] <= lv.min() and lv.max() <= G.LOGVAR_RANGE[1]
    assert np.abs(mom32 - mom64).max() < 5e-5 and np.abs(z32 - z64).max() < 5e-5 and np.abs(r32 - r64).max() < 1e-4
    for k in ("loss", "loss_mse", "loss_kl", "img_std", "z_std"):
        assert abs(m32[k] - m64[k]) <= 1e-5 * abs(m64[k]), (k, m32[k], m64[k])
    off, _, _, _ = VO.loss(params, x, eps, False, 1e-5)
    assert off["loss_kl"] == 0.0 and off["loss"] == off["loss_mse"] == m64["loss_mse"]


def test_posterior_definition_on_hand_made_moments():
    """clip(-30, 20), sample, kl and mode of FlaxDiagonalGaussianDistribution on numbers one can check by hand."""
    mom = np.zeros((1, 1, 1, 10))
    mom[0, 0, 0, :5] = [1.0, -2.0, 0.5, 0.0, 3.0]
    mom[0, 0, 0, 5:] = [-40.0, -30.0, 0.0, 20.0, 25.0]
    eps = np.full((1, 1, 1, 5), 2.0)
    z, kl, std = VO.posterior(mom, eps)
    lv = np.array([-30.0, -30.0, 0.0, 20.0, 20.0])
    assert np.allclose(std[0, 0, 0], np.exp(0.5 * lv), rtol=1e-15)
    assert np.allclose(z[0, 0, 0], mom[0, 0, 0, :5] + 2.0 * np.exp(0.5 * lv), rtol=1e-15)
    assert np.isclose(kl[0], 0.5 * np.sum(mom[0, 0, 0, :5] ** 2 + np.exp(lv) - 1 - lv), rtol=1e-15)


def test_trained_like_set_qualifies_once_its_logvar_head_is_scaled():
    """tests.util.vae_params_heavy saturates both clamps (trained_like was tuned for the mean channels); scaling quant_conv's log-variance
    columns brings the heavy-tailed set inside the fixture condition [-8, 4]."""
    x = rng(4244).uniform(-1, 1, (2, 64, 64, 3))
    fit, base = VO.trained_like_params(2, x)
    lv = VO.moments(base, x)[..., 4:]
    assert lv.min() < -30 or lv.max() > 20, "the unscaled heavy set was expected to saturate the clamp"
    lv2 = VO.moments(fit, x)[..., 4:]
    assert G.LOGVAR_RANGE[0] <= lv2.min() and lv2.max() <= G.LOGVAR_RANGE[1], (lv2.min(), lv2.max())


@pytest.mark.parametrize("name", list(G.CASES))
def test_goldens_are_what_the_oracle_computes(name):
    fn, args = G.CASES[name]
    seeds, compute = fn(*args)
    z = np.load(G.golden_path(name))
    for k, v in seeds.items():
        assert int(z[f"seed_{k}"]) == v
    out = compute()
    for k, v in out.items():
        assert np.array_equal(np.asarray(v, np.float64), z[f"out_{k}"]), f"{name}: out_{k}"
        assert z[f"out_{k}"].dtype == np.float64


def test_golden_files_stay_small():
    import os
    for name in G.CASES:
        assert os.path.getsize(G.golden_path(name)) < 450 * 1024, name


# ---- create --------------------------------------------------------------------------------------------------------------------------
def test_create_accepts_the_reference_config():
    """Every check passes for model/stable_vae_model.yaml; without a GPU the call then stops at the engine, loudly."""
    if torch.cuda.is_available():
        m = StableVAEModel.create(0, None, SHAPES, **_kw())
        assert sorted(m.config) == ["beta", "data_name", "n_downsample", "name", "rgb_obs", "use_kl"] and m.config["n_downsample"] == 6
    else:
        with pytest.raises(_lib.LDPHipUnavailable, match="no CPU fallback"):
            StableVAEModel.create(0, None, SHAPES, **_kw())


@pytest.mark.parametrize("over,match", [
    (dict(down_block_types=["DownEncoderBlock2D"] * 5), "6 DownEncoderBlock2D"),
    (dict(layers_per_block=1), "layers_per_block=1"),
    (dict(norm_num_groups=16), "norm_num_groups=16"),
    (dict(block_out_channels=[128, 256, 512, 512, 512, 512]), "block_out_channels"),
    (dict(latent_channels=16), "latent_channels=16"),
    (dict(act_fn="relu"), "act_fn"),
    (dict(in_channels=1), "in_channels=1"),
])
def test_create_refuses_what_the_engine_does_not_build(over, match):
    with pytest.raises(NotImplementedError, match=match):
        StableVAEModel.create(0, None, SHAPES, **_kw(vae={**VAE_CFG, **over}))


def test_create_refuses_frames_the_conv_tiles_are_not_built_for():
    with pytest.raises(NotImplementedError, match="84-pixel frames"):
        StableVAEModel.create(0, None, dict(all_shapes={KEY: [84, 84, 3]}), **_kw())
    with pytest.raises(NotImplementedError, match="different sizes"):
        StableVAEModel.create(0, None, dict(all_shapes={KEY: [64, 64, 3], KEY2: [128, 128, 3]}), **_kw(rgb_obs=[KEY, KEY2]))
    with pytest.raises(KeyError, match="no entry for the camera"):
        StableVAEModel.create(0, None, SHAPES, **_kw(rgb_obs=["sideview_image"]))
    with pytest.raises(NotImplementedError):                       # a 'mean'/'std' table (utils/data_utils.py:31-32)
        StableVAEModel.create(0, None, SHAPES, **_kw(obs_normalization={"obs": {KEY: dict(mean=0, std=1)}}))


# ---- host logic of the class, on a stub engine -----------------------------------------------------------------------------------------
class _StubEngine:
    """Records what the model asks for; the arithmetic that matters here is the normalisation."""
    def __init__(self):
        self.loaded = {"planner": None, "idm": None, "vae": None}
        self.call_seq, self.fault_upto, self.last_fault_kinds = 0, -1, 0
        self.frames, self.uploaded = [], []

    def load_params(self, vae=None, versions=None):
        self.loaded["vae"] = versions["vae"]
        self.uploaded.append(vae)

    def normalize_bounds(self, x, lo, hi, normalize):
        assert normalize is True
        return (x - lo[0]) / (hi[0] - lo[0]) * 2 - 1

    def poll_fault_kinds(self):
        return 0

    def vae_metrics(self, img, use_kl, beta, seed=0, noise=None, row_offset=0, want=()):
        self.frames.append(img)
        self.call_seq += 1
        return torch.arange(11, dtype=torch.float32) + seed, {}


def _stub_model(rgb_obs=(KEY,), params=None):
    p = params if params is not None else {"quant_conv/bias": np.zeros(8, np.float32)}
    cfg = dict(rgb_obs=list(rgb_obs), name="stable_vae_model", use_kl=True, beta=1e-5, n_downsample=6, data_name="rm_lift")
    m = StableVAEModel(DPState(p, None, ema_is_params=True), NORM, cfg, _StubEngine(), W.VAESpec(), 64, "cpu")
    m._sync_weights = lambda use_ema: None
    return m


def test_cameras_are_concatenated_on_the_batch_axis():
    a, b = G.raw_frames(1, 2), G.raw_frames(2, 2)
    m = _stub_model((KEY, KEY2))
    out = m.get_metrics({"obs": {KEY: a, KEY2: b}}, 3)
    img = m._engine.frames[0]
    assert tuple(img.shape) == (4, 64, 64, 3)                                    # frame 0 of each key, keys stacked on axis 0 (:28)
    assert np.allclose(img[:2].numpy(), G.normalised(a), atol=1e-6) and np.allclose(img[2:].numpy(), G.normalised(b), atol=1e-6)
    assert list(out) == list(VO.METRIC_KEYS) == list(_lib.VAE_METRIC_KEYS)
    assert float(out["img_min"]) == 3.0 and float(out["z_std"]) == 13.0
    with pytest.raises(ValueError, match=r"\(B, H, 64, 64, 3\)"):
        m.get_metrics({"obs": {KEY: a[:, 0], KEY2: b}}, 0)
    with pytest.raises(AssertionError, match="obs_normalization keys"):
        m.get_metrics({"obs": {KEY: a, KEY2: b, "unknown": a}}, 0)


def test_update_raises_with_the_reason():
    with pytest.raises(NotImplementedError, match="backward pass of the 2-D convolutions"):
        _stub_model().update({}, 0, 0)


def test_sample_refuses_another_image_size():
    m = _stub_model()
    m._image_size = 128
    with pytest.raises(NotImplementedError, match="64-pixel frames"):
        m.sample(0)


def test_get_params_replace_and_version_tokens():
    p = {"quant_conv/bias": np.zeros(8, np.float32)}
    m = _stub_model(params=p)
    gp = m.get_params()
    assert sorted(gp) == ["ema_params", "vae_params"] and gp["vae_params"] is p and gp["ema_params"] is p    # ema starts equal to params
    assert m.vae_state.step == 0 and m.vae_state.version != m.vae_state.ema_version
    e = {"quant_conv/bias": np.ones(8, np.float32)}
    m2 = m.replace(vae_state=m.vae_state.replace(ema_params=e))
    assert m2 is not m and m.vae_state.ema_params is p and m2.get_params()["ema_params"]["quant_conv/bias"][0] == 1.0
    assert m2.vae_state.version == m.vae_state.version and m2.vae_state.ema_version != m.vae_state.ema_version
    assert m2._engine is m._engine
    with pytest.raises(AttributeError, match="no field 'nope'"):
        m.replace(nope=1)
    assert abs(m2.replace(lr_schedule=lambda c: 0.5).lr_schedule(3) - 0.5) == 0


def test_weight_sets_upload_on_change_only():
    m = _stub_model(params=W.init_vae_params(seed=3))
    del m._sync_weights                                                  # the real one, against the stub engine's slot
    m._sync_weights(use_ema=False)
    m._sync_weights(use_ema=False)
    assert m.uploads == 1
    m._sync_weights(use_ema=True)
    m._sync_weights(use_ema=True)
    assert m.uploads == 2 and m.replace(config=m.config).uploads == 2
    bad = m.replace(vae_state=m.vae_state.replace(params={"quant_conv/bias": np.zeros(8, np.float32)}))
    with pytest.raises(Exception, match="missing|shape|leaf|quant_conv|encoder"):
        bad._sync_weights(use_ema=False)


# ---- snapshots -----------------------------------------------------------------------------------------------------------------------
def test_snapshot_round_trip_into_load_pretrained_vae(tmp_path):
    from latent_diffusion_planning_amd.agent import load_pretrained_vae
    p, e = W.init_vae_params(seed=3, decoder=False), W.init_vae_params(seed=4, decoder=False)
    m = _stub_model(params=p)
    m = m.replace(vae_state=m.vae_state.replace(ema_params=e))
    path = str(tmp_path / "200.ckpt")
    checkpoint.save_snapshot(m, path)
    raw = checkpoint.restore(path)
    assert sorted(raw) == ["ema_params", "vae_params"]                   # the names train_vae.py saves
    got = load_pretrained_vae(path)                                      # what LDPAgent.create(vae_pretrain_path=...) loads
    assert list(got) == list(p) and all(np.array_equal(got[k], p[k]) for k in p)
    back = checkpoint.load_snapshot(_stub_model(), path)
    assert all(np.array_equal(back.vae_state.params[k], p[k]) and np.array_equal(back.vae_state.ema_params[k], e[k]) for k in p)
    checkpoint.save(str(tmp_path / "noema.ckpt"), {"vae_params": p})
    only = checkpoint.load_snapshot(_stub_model(), str(tmp_path / "noema.ckpt"))
    assert only.vae_state.ema_params is only.vae_state.params
    checkpoint.save(str(tmp_path / "other.ckpt"), {"planner_params": {"w": np.zeros(1, np.float32)}})
    with pytest.raises(checkpoint.CheckpointError, match="no vae_params"):
        checkpoint.load_snapshot(_stub_model(), str(tmp_path / "other.ckpt"))


# ---- harness -------------------------------------------------------------------------------------------------------------------------
def test_eval_vae_metrics_averages_and_prefixes():
    from latent_diffusion_planning_amd.harness import eval_vae_metrics

    class Stub:
        def __init__(self):
            self.seeds = []

        def get_metrics(self, batch, rng):
            self.seeds.append(rng)
            return {"loss": np.float32(batch["v"]), "loss_kl": np.float32(2 * batch["v"])}
    s = Stub()
    out = eval_vae_metrics(s, [{"v": float(i)} for i in range(20)], 100)
    assert s.seeds == list(range(100, 111))                              # eleven batches (train_vae.py:152 `if idx >= 10: break`)
    assert out == {"evaldata/loss": 5.0, "evaldata/loss_kl": 10.0}
    assert eval_vae_metrics(Stub(), iter([{"v": 1.0}, {"v": 3.0}]), 0, max_batches=5) == {"evaldata/loss": 2.0, "evaldata/loss_kl": 4.0}
    with pytest.raises(ValueError, match="no batches"):
        eval_vae_metrics(Stub(), [], 0)


# ---- Philox layout of eps ------------------------------------------------------------------------------------------------------------
def test_philox_eps_layout_and_row_offset_split():
    """eps of frame n, latent element e = Philox (seed, (row_offset + n) * per + e, step 0, stream 9): a split batch draws what the whole
    draws, and the stream is none of the other draws' (0, 1: the loops; 7, 8: the loss noise; 10: sample())."""
    assert _lib.PHILOX_STREAM_VAE_EPS == VO.STREAM_VAE_EPS == 9 and PHILOX_STREAM_VAE_SAMPLE == VO.STREAM_VAE_SAMPLE == 10
    seed, N, per = 99, 7, 16
    whole = VO.philox_eps(seed, N, per)
    assert whole.shape == (N, per)
    assert np.array_equal(whole.reshape(-1), philox.normal(seed, 0, 0, 9, N * per))
    a, b = VO.philox_eps(seed, 3, per, row_offset=0), VO.philox_eps(seed, 4, per, row_offset=3)
    assert np.array_equal(np.concatenate([a, b]), whole)
    assert whole[5, 2] == philox.normal(seed, 5 * per + 2, 0, 9, 1)[0]
    for other in (0, 1, 7, 8, 10):
        assert not np.array_equal(philox.normal(seed, 0, 0, other, 8), whole.reshape(-1)[:8])
    import re
    hdr = open(_lib.HEADER_PATH).read()
    ids = [int(v) for v in re.findall(r"#define LDP_PHILOX_STREAM_\w+ (\d+)u", hdr)]
    assert len(ids) == len(set(ids)) and 9 in ids and 10 in ids
