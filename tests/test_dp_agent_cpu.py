"""DPAgent without a GPU: the oracle's own known-answer tests (two independent restatements of the encoder's primitives), the ResNet
parameter tree, the condition layout, the create refusals, get_params / config, snapshots with encoder_params, and the conditions the
committed goldens rest on."""
import copy

import numpy as np
import pytest
import torch

from latent_diffusion_planning_amd import weights as W
from tests import dp_resnet_oracle as RO
from tests.golden.make_golden_dp_resnet import (ACTION_TOL, AH, CASES, OH, T, TIE_TOL, feature_params, frames_to_input, golden_path,
                                                rel_err)
from tests.util import rng


# ---- the oracle's KATs ---------------------------------------------------------------------------------------------------------------
def test_numpy_loops_agree_with_torch_to_float64_roundoff():
    g = rng(1)
    x = g.uniform(-1, 1, (2, 10, 10, 3))
    k7 = g.standard_normal((7, 7, 3, 5))
    np.testing.assert_allclose(RO.np_conv7x7_s2(x, k7), RO.conv7x7_s2(x, k7), rtol=0, atol=1e-12)
    f = g.standard_normal((2, 6, 6, 8))
    k1 = g.standard_normal((1, 1, 8, 12))
    np.testing.assert_allclose(RO.np_conv1x1_s2(f, k1), RO.conv1x1_s2(f, k1), rtol=0, atol=1e-13)
    np.testing.assert_array_equal(RO.np_maxpool(f), RO.maxpool(f))
    sc, bi = 1 + 0.1 * g.standard_normal(8), 0.1 * g.standard_normal(8)
    np.testing.assert_allclose(RO.np_gn(f, sc, bi), RO.gn(f, sc, bi), rtol=0, atol=1e-12)
    np.testing.assert_allclose(RO.np_spatial_softmax(f), RO.spatial_softmax(f), rtol=0, atol=1e-14)


def test_maxpool_pads_with_minus_infinity():
    x = -rng(2).uniform(0.5, 3.0, (1, 8, 8, 4))
    for y in (RO.np_maxpool(x), RO.maxpool(x)):
        assert y.shape == (1, 4, 4, 4) and (y < 0).all()                       # zero padding would give 0 in the last row / column
        np.testing.assert_array_equal(y[0, 3, 3], x[0, 6:8, 6:8].max(axis=(0, 1)))      # the last window is 2 x 2, not 3 x 3
        np.testing.assert_array_equal(y[0, 0, 0], x[0, 0:3, 0:3].max(axis=(0, 1)))


def test_conv1x1_s2_reads_pixel_2y_2x():
    x = np.zeros((1, 4, 4, 2))
    x[0, 2, 2] = [1.0, 2.0]                                                    # the one marked pixel: output (1, 1)
    x[0, 1, 1] = [7.0, 7.0]                                                    # odd coordinates are never read
    k = np.array([[[[1.0, 10.0, 0.0], [100.0, 0.0, 1.0]]]])
    for y in (RO.np_conv1x1_s2(x, k), RO.conv1x1_s2(x, k)):
        want = np.zeros((1, 2, 2, 3))
        want[0, 1, 1] = [201.0, 10.0, 2.0]
        np.testing.assert_array_equal(y, want)


def test_spatial_softmax_axes_and_signs():
    x = np.full((1, 2, 2, 3), -60.0)
    x[0, 0, 1] = 60.0                                                          # all mass in row 0, last column
    for y in (RO.np_spatial_softmax(x), RO.spatial_softmax(x)):
        np.testing.assert_allclose(y[0, :3], 1.0, atol=1e-12)                   # expected_x follows the COLUMN: +1
        np.testing.assert_allclose(y[0, 3:], -1.0, atol=1e-12)                  # expected_y follows the ROW: -1
    u = RO.spatial_softmax(np.zeros((2, 2, 2, 5)))
    np.testing.assert_allclose(u, 0.0, atol=1e-15)                              # a flat map: the centre


def test_feature_width_is_1024():
    p = W.init_resnet_params(seed=4)
    f = RO.encode(p, frames_to_input(RO.synth_frames(2, 4)))
    assert f.shape == (2, 1024) == (2, RO.FEAT) and W.ResNetSpec().feature_dim == 1024
    assert np.all(np.abs(f) <= 1.0)


def test_group_norm_keeps_the_variance_of_a_group_with_a_large_mean():
    g = rng(5)
    z = g.standard_normal((2, 8, 8, 16))
    x = (100.0 + 1e-3 * z).astype(np.float32)
    sc, bi = np.ones(16), np.zeros(16)
    ref = RO.gn(x, sc, bi)
    # the float32 restatement is centred too: its error is the rounding of the mean (half an ulp of 100, times rstd = 301), not a lost variance
    err32 = rel_err(RO.gn(x, sc, bi, dtype=torch.float32), ref)
    assert err32 < 5e-3
    # var = 1e-6 next to eps = 1e-5: with the variance lost (E[x^2] - E[x]^2 in float32 clamps it to 0) every output is 4.9 % too large
    x64 = x.astype(np.float64).reshape(2, 64, 4, 4)
    lost = ((x64 - x64.mean(axis=(1, 3), keepdims=True)) / np.sqrt(1e-5)).reshape(x.shape)
    assert rel_err(lost, ref) > 10 * err32
    np.testing.assert_allclose(RO.np_gn(x, sc, bi), ref, rtol=0, atol=1e-9)


# ---- weights.py ------------------------------------------------------------------------------------------------------------------------
def test_resnet_shapes():
    s = W.resnet_shapes()
    proj = sorted(int(k.split("/")[0].split("_")[1]) for k in s if k.endswith("conv_proj/kernel"))
    assert proj == [2, 4, 6]
    # conv_init 1 + norm_init 2 + 8 blocks x (2 kernels + 2 norms x 2) + 3 projected blocks x (1 kernel + 1 norm x 2)
    assert len(s) == 3 + 8 * 6 + 3 * 3 == 60
    assert s["conv_init/kernel"] == (7, 7, 3, 64) and s["ResNetBlock_6/conv_proj/kernel"] == (1, 1, 256, 512)
    assert s["ResNetBlock_2/Conv_0/kernel"] == (3, 3, 64, 128) and s["ResNetBlock_7/Conv_1/kernel"] == (3, 3, 512, 512)
    assert not any(k.endswith("bias") and "Norm" not in k and "norm" not in k for k in s)      # no conv has a bias
    assert sum(int(np.prod(v)) for v in s.values()) == 11176512
    assert [b[2] for b in W.ResNetSpec().blocks()] == [1, 1, 2, 1, 2, 1, 2, 1]


def test_init_resnet_params_and_tree_check():
    a, b = W.init_resnet_params(seed=7), W.init_resnet_params(seed=7)
    assert list(a) == list(W.resnet_shapes()) and all(np.array_equal(a[k], b[k]) and a[k].dtype == np.float32 for k in a)
    assert not np.array_equal(a["conv_init/kernel"], W.init_resnet_params(seed=8)["conv_init/kernel"])
    plain = W.init_resnet_params(seed=7, perturb=False)
    assert np.all(plain["norm_init/scale"] == 1) and np.all(plain["ResNetBlock_4/norm_proj/bias"] == 0)
    assert np.any(a["norm_init/scale"] != 1) and np.any(a["ResNetBlock_4/norm_proj/bias"] != 0)
    k = a["ResNetBlock_7/Conv_1/kernel"]
    assert abs(k.std() / np.sqrt(2.0 / (9 * 512)) - 1) < 0.01                   # kaiming_normal
    W.check_resnet_params(a)
    miss = dict(a)
    del miss["ResNetBlock_2/norm_proj/scale"]
    with pytest.raises(KeyError, match="ResNetBlock_2/norm_proj/scale"):
        W.check_resnet_params(miss)
    bad = dict(a)
    bad["ResNetBlock_1/Conv_0/kernel"] = np.zeros((3, 3, 64, 32), np.float32)
    with pytest.raises(ValueError, match=r"ResNetBlock_1/Conv_0/kernel.*\(3, 3, 64, 32\)"):
        W.check_resnet_params(bad)
    extra = dict(a)
    extra["ResNetBlock_0/conv_proj/kernel"] = np.zeros((1, 1, 64, 64), np.float32)      # stage 0's first block has no projection
    with pytest.raises(KeyError, match="ResNetBlock_0/conv_proj/kernel"):
        W.check_resnet_params(extra)


# ---- get_obs_cond ----------------------------------------------------------------------------------------------------------------------
def _verbatim_obs_cond(data, batch, feat_fn, oh, shared):
    """agent/dp_agent.py:31-52 line by line, the encoder replaced by `feat_fn(key, frames)`."""
    low = np.concatenate([batch[k][:, :oh] for k in data["lowdim_obs"]], axis=-1).astype(np.float32)
    B = low.shape[0]
    low = low.reshape(low.shape[0], -1)
    if shared:
        init = np.concatenate([batch[k][:, :oh] for k in data["rgb_obs"]], axis=1)
        init = init.reshape(-1, *init.shape[-3:])
        img = feat_fn("shared", init).reshape(B, -1)
    else:
        lst = []
        for k in data["rgb_obs"]:
            init = batch[k][:, :oh]
            init = init.reshape(-1, *init.shape[-3:])
            lst.append(feat_fn(k, init).reshape(B, -1))
        img = np.concatenate(lst, axis=-1)
    return np.concatenate([img, low], axis=-1)


def _fake_features(key, frames):
    """1024 'features' that identify the frame and the encoder: deterministic functions of the frame's pixels."""
    s = frames.reshape(frames.shape[0], -1).astype(np.float64).sum(axis=1, keepdims=True)
    off = {"shared": 0.0, "agentview_image": 1.0, "robot0_eye_in_hand_image": 2.0}[key]
    return (s * 1e-3 + off + np.arange(1024)[None] * 1e-6).astype(np.float32)


@pytest.mark.parametrize("cfg,shared", [("rm_img", False), ("rm_img2", False), ("rm_img2", True)])
@pytest.mark.parametrize("oh", [1, 2])
def test_obs_cond_layout(cfg, shared, oh):
    from latent_diffusion_planning_amd.dp_agent import dp_image_cond
    data = RO.BY_NAME[cfg]
    B = 3
    nobs = RO.normalized_obs(data, RO.synth_image_batch(data, B, 3, 9)["obs"])
    want = _verbatim_obs_cond(data, nobs, _fake_features, oh, shared)
    assert want.shape == (B, RO.cond_dim(data, oh))
    # the oracle's layout
    ins = RO.encoder_inputs(data, nobs, oh, shared)
    feats = {k: _fake_features(k, v) for k, v in ins.items()}
    np.testing.assert_array_equal(RO.obs_cond_from_features(data, nobs, feats, oh, shared), want)
    # the product's assembly (torch.cat of the per-encoder blocks, then the low-dim block)
    low = torch.cat([torch.tensor(nobs[k])[:, :oh] for k in data["lowdim_obs"]], dim=-1)
    blocks = [torch.tensor(feats[k]) for k in RO.encoder_keys(data, shared)]
    np.testing.assert_array_equal(dp_image_cond(blocks, low).numpy(), want)
    if cfg == "rm_img" and oh == 1:
        assert want.shape[1] == 1033


# ---- create ----------------------------------------------------------------------------------------------------------------------------
def _create(cfg="rm_img", shape_meta=None, **over):
    from latent_diffusion_planning_amd.dp_agent import DPAgent
    data = RO.BY_NAME[cfg]
    kw = RO.dp_kwargs(data, OH, T, AH)
    kw.update(over)
    return DPAgent.create(0, None, shape_meta or data["shape_meta"], **kw)


def test_create_without_a_gpu_raises_unavailable(monkeypatch):
    from latent_diffusion_planning_amd._lib import LDPHipUnavailable
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(LDPHipUnavailable):
        _create()


def _enc(**over):
    e = dict(RO.ENCODER_CFG)
    e.update(over)
    return dict(encoder=e)


def _meta(**shapes):
    m = copy.deepcopy(RO.RM_IMG["shape_meta"])
    m["all_shapes"].update(shapes)
    return m


@pytest.mark.parametrize("over,reason", [
    (_enc(stage_sizes=[3, 4, 6, 3]), "stage_sizes"), (_enc(block_cls="BottleneckResNetBlock"), "block_cls"),
    (_enc(feature_layers=[256]), "feature_layers"), (_enc(n_filters=32), "n_filters"), (_enc(act="swish"), "act"),
    (_enc(norm="layer"), "norm"), (_enc(add_spatial_coordinates=True), "add_spatial_coordinates"),
    (_enc(pooling_method="avg"), "pooling_method"), (_enc(softmax_temperature=-1), "softmax_temperature"),
    (_enc(use_multiplicative_cond=True), "use_multiplicative_cond"), (_enc(use_film=True), "use_film"),
    (_enc(use_tanh=True), "use_tanh"), (_enc(use_simnorm=True), "use_simnorm"), (_enc(use_simnorm_rescale=True), "use_simnorm_rescale"),
    (_enc(use_sigmoid=True), "use_sigmoid"), (_enc(dtype="bfloat16"), "dtype"),
    (dict(shape_meta=_meta(agentview_image=[84, 84, 3])), "64x64x3"),
    (dict(rgb_obs=[f"cam{i}" for i in range(5)], shape_meta=_meta(**{f"cam{i}": [64, 64, 3] for i in range(5)})), "at most 4"),
    (dict(obs_horizon=9), "8192"),                                             # 9 * 1033 = 9297 columns
    (dict(planner=dict(down_dims=[256, 512, 1000], kernel_size=5, n_groups=8)), "down_dims"),
    (dict(planner=dict(down_dims=[256, 512, 1024], kernel_size=3, n_groups=8)), "kernel_size"),
    (dict(planner=dict(down_dims=[256, 512, 1024], kernel_size=5, n_groups=4)), "n_groups"),
    (dict(planner=dict(down_dims=[256, 512, 1024], kernel_size=5, n_groups=8, downsample=False)), "downsample"),
])
def test_create_refuses_what_is_not_built(monkeypatch, over, reason):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)             # every refusal comes before the device is looked at
    with pytest.raises(NotImplementedError, match=reason):
        _create(**over)


def _stub_agent(cfg="rm_img", shared=False):
    """A DPAgent without an engine: the host-side surface only."""
    from latent_diffusion_planning_amd.dp_agent import DPAgent, DPState
    data = RO.BY_NAME[cfg]
    small = W.ResNetSpec(n_filters=8)                                          # the tree's names at an eighth of its widths: snapshots stay quick
    enc = {k: DPState(W.init_resnet_params(small, seed=20 + i), None, ema_is_params=True) for i, k in enumerate(RO.encoder_keys(data, shared))}
    pl = DPState({"Dense_0/kernel": rng(3).standard_normal((4, 16)).astype(np.float32), "Dense_0/bias": np.zeros(16, np.float32)}, None,
                 ema_is_params=True)
    config = dict(n_diffusion_steps=100, lowdim_obs=list(data["lowdim_obs"]), rgb_obs=list(data["rgb_obs"]), obs_horizon=1, name="dp_agent",
                  action_dim=7, pred_horizon=T, action_horizon=AH, shared_encoder=shared)
    return DPAgent(pl, enc, data["obs_normalization"], config, None, RO.planner_spec(data, 1), torch.device("cpu"))


def test_get_params_config_and_what_raises():
    ag = _stub_agent("rm_img2")
    p = ag.get_params()
    assert sorted(p) == ["encoder_ema_params", "encoder_params", "planner_ema_params", "planner_params"]
    assert sorted(p["encoder_params"]) == ["agentview_image_params", "robot0_eye_in_hand_image_params"]
    moved = ag.replace(encoder_state_dict={k: v.replace(ema_params={q: w * 0 for q, w in v.params.items()})
                                           for k, v in ag.encoder_state_dict.items()})
    pm = moved.get_params()
    # the reference's quirk: encoder_ema_params holds the PARAMETERS, whatever the EMA is
    assert pm["encoder_ema_params"]["agentview_image_params"] is moved.encoder_state_dict["agentview_image"].params
    assert np.all(moved.encoder_state_dict["agentview_image"].ema_params["conv_init/kernel"] == 0)
    assert sorted(ag.config) == sorted(["n_diffusion_steps", "lowdim_obs", "rgb_obs", "obs_horizon", "name", "action_dim", "pred_horizon",
                                        "action_horizon", "shared_encoder"])
    with pytest.raises(NotImplementedError, match="backward pass of the ResNet encoder.*trained with the reference"):
        ag.update({}, 0, 0)
    for fn in (ag.sample_viz, ag.sample_action_from_plan, ag.update_mixed):
        with pytest.raises(NotImplementedError):
            fn()
    with pytest.raises(AttributeError):
        ag.replace(idm_state=None)
    with pytest.raises(KeyError, match="robot0_eye_in_hand_image"):
        ag.replace(encoder_state_dict={"agentview_image": ag.encoder_state_dict["agentview_image"]})
    sh = _stub_agent("rm_img2", shared=True)
    assert sorted(sh.get_params()["encoder_params"]) == ["shared_params"]


@pytest.mark.parametrize("shared", [False, True])
def test_snapshot_round_trip_with_encoder_params(tmp_path, shared):
    from latent_diffusion_planning_amd import checkpoint as ck
    src = _stub_agent("rm_img2", shared)
    path = str(tmp_path / "5.ckpt")
    ck.save_snapshot(src, path)
    raw = ck.restore(path)
    key = "shared_params" if shared else "agentview_image_params"
    assert raw["encoder_params"][key]["ResNetBlock_2"]["conv_proj"]["kernel"].shape == (1, 1, 8, 16)      # nested, as the reference writes it
    dst = _stub_agent("rm_img2", shared)
    dst = dst.replace(encoder_state_dict={k: v.replace(params={q: w + 1 for q, w in v.params.items()}) for k, v in dst.encoder_state_dict.items()})
    new = ck.load_snapshot(dst, path)
    assert sorted(new.encoder_state_dict) == sorted(src.encoder_state_dict)
    for k, st in new.encoder_state_dict.items():
        assert st.version != dst.encoder_state_dict[k].version
        assert st.ema_params is st.params                                       # params and EMA are both set from the file
        for q, w in src.encoder_state_dict[k].params.items():
            np.testing.assert_array_equal(st.params[q], w)
    for q, w in src.planner_state.params.items():
        np.testing.assert_array_equal(new.planner_state.params[q], w)


def test_snapshot_encoder_params_are_skipped_without_encoder_state_dict(tmp_path):
    from latent_diffusion_planning_amd import checkpoint as ck
    from latent_diffusion_planning_amd.agent import ParamState

    class _Plain:
        def __init__(self):
            self.planner_state = ParamState({"w": np.zeros(2, np.float32)})

        def replace(self, **kw):
            new = copy.copy(self)
            for k, v in kw.items():
                setattr(new, k, v)
            return new
    path = str(tmp_path / "6.ckpt")
    ck.save_snapshot(_stub_agent("rm_img"), path)
    new = ck.load_snapshot(_Plain(), path)
    assert not hasattr(new, "encoder_state_dict") and "Dense_0/kernel" in new.planner_state.params


# ---- the goldens -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_satisfies_the_generators_conditions(name):
    """Recomputed from the stored arrays: the tie condition from the stored frames and the seeded encoders (float64 encoder, here), the
    float32-restatement condition from the two stored action sets."""
    z = np.load(golden_path(name))
    assert all(np.all(np.isfinite(z[k])) for k in z.files if k.startswith("out_"))
    if "features" in name:
        kind = name.rsplit("_", 1)[1]
        assert z["in_frames"].dtype == np.uint8 and z["in_frames"].shape == (5, 64, 64, 3)
        f64, logits = RO.encode(feature_params(kind, int(z["seed_params"])), frames_to_input(z["in_frames"]), torch.float64, return_logits=True)
        np.testing.assert_allclose(f64, z["out_features"], rtol=0, atol=1e-12)
        assert RO.tie_gap(logits) > TIE_TOL
        assert float(z["out_err32"]) == rel_err(z["out_features32"], z["out_features"])
        if kind == "heavy":
            assert np.isfinite(RO.tie_gap(logits)) and np.abs(logits).max() > 50      # the argmax-like regime is really there
        return
    cfg = "rm_img2" if "rm_img2" in name else "rm_img"
    shared = "shared" in name
    data = RO.BY_NAME[cfg]
    obs = {k[len("in_obs__"):]: z[k] for k in z.files if k.startswith("in_obs__")}
    assert all(obs[k].dtype == np.uint8 for k in data["rgb_obs"])
    enc = RO.encoder_params(data, int(z["seed_encoder"]), shared)
    cond, logits = RO.obs_cond(data, enc, RO.normalized_obs(data, obs), OH, shared, torch.float64, return_logits=True)
    np.testing.assert_allclose(cond, z["out_cond"], rtol=0, atol=1e-12)
    assert min(RO.tie_gap(v) for v in logits.values()) > TIE_TOL
    if "sample" in name:
        B = z["in_x_init"].shape[0]
        assert z["out_action"].shape == (B, AH, 7) and np.abs(z["out_action"]).max() <= 1.0
        err = float(np.abs(z["out_action32"] - z["out_action"]).max())
        assert err <= ACTION_TOL and float(z["out_err32"]) == err
    else:
        assert abs(float(z["out_loss32"]) - float(z["out_loss"])) <= 1e-5 * float(z["out_loss"])
