"""StableVAEModel.update without a GPU: the float64 autograd oracle (tests/vae_train_oracle.py) against central differences of the independent
numpy restatement (oracle.np64 through tests/vae_model_oracle.py), the host logic of `update` on a stub engine, the FLOP count of the VAE,
the fixture conditions of the whole-leaf GPU tests (tests/test_hip_vae_train_full.py)."""
import numpy as np
import pytest
import torch

from latent_diffusion_planning_amd import _lib, flops, weights as W
from latent_diffusion_planning_amd.dp_vae_agent import DPState
from latent_diffusion_planning_amd.schedule import warmup_cosine_decay_schedule
from latent_diffusion_planning_amd.vae_model import StableVAEModel
from tests import vae_model_oracle as VO
from tests import vae_train_cases as VC
from tests import vae_train_oracle as VT
from tests.train_stub import TrainStub
from tests.util import rng

KEY, KEY2 = "agentview_image", "robot0_eye_in_hand_image"
NORM = {"obs": {KEY: dict(min=0.0, max=255.0), KEY2: dict(min=0.0, max=255.0)}}


# ---- 1. the oracle's gradient against central differences of oracle.np64 ---------------------------------------------------------------
# one entry of each kind the issue names: a 3x3 kernel at 64 px, a stride-2 kernel, a GroupNorm scale, an attention query kernel, a
# quant_conv log-variance column (LC = 4: output channels 4..7)
ENTRIES = (("encoder/down_blocks_0/resnets_0/conv1/kernel", (1, 2, 5, 17)),
           ("encoder/down_blocks_1/downsamplers_0/conv/kernel", (0, 2, 33, 101)),
           ("decoder/up_blocks_5/resnets_1/norm2/scale", (70,)),
           ("encoder/mid_block/attentions_0/query/kernel", (12, 200)),
           ("quant_conv/kernel", (0, 0, 3, 6)))
H = 1e-4          # central-difference step


def test_oracle_gradient_matches_central_differences_of_np64():
    """Central differences have truncation error h^2 f''' / 6 and cancellation error ~1e-16 |loss| / h; at h = 1e-4 on weights of size
    0.01 - 1 both are below 1e-7 of these entries' gradients (checked: halving h moves the estimates by less than that).  The bound, 1e-5
    relative + 1e-11, is two orders of magnitude above both and seven below an error in the backward pass (a missing term moves a
    gradient by O(1) of itself)."""
    torch.set_num_threads(16)
    p = W.init_vae_params(seed=5)
    x = rng(31).uniform(-1, 1, (1, 64, 64, 3))
    eps = rng(32).standard_normal((1, 2, 2, 4))
    _, g, mom, _ = VT.loss_and_grads(p, x, eps, True, VT.BETA)
    lv = mom[..., 4:]
    assert lv.min() > -29 and lv.max() < 19                         # the clamp is not what this tests

    def loss_at(path, idx, delta):
        q = dict(p)
        a = np.array(p[path], np.float64)
        a[idx] += delta
        q[path] = a
        return VO.loss(q, x, eps, True, VT.BETA)[0]["loss"]
    for path, idx in ENTRIES:
        fd = (loss_at(path, idx, H) - loss_at(path, idx, -H)) / (2 * H)
        ad = float(g[path][idx])
        print(path, idx, "autograd", ad, "central difference", fd)
        assert abs(fd - ad) <= 1e-5 * abs(ad) + 1e-11, (path, idx, ad, fd)


# ---- 2. host logic of update on a stub engine ----------------------------------------------------------------------------------------
@pytest.fixture
def stub_model(monkeypatch):
    from latent_diffusion_planning_amd import vae_model
    monkeypatch.setattr(vae_model.W, "check_params", lambda tree, shapes: None)      # the stub's trees are not 41.7 M parameters

    def make(rgb_obs=(KEY,), use_kl=True, image_size=64):
        cfg = dict(rgb_obs=list(rgb_obs), name="stable_vae_model", use_kl=use_kl, beta=1e-5, n_downsample=6, data_name="rm_lift")
        sched = warmup_cosine_decay_schedule(1e-6, 1e-4, 1000, 300000, 1e-6)
        p = {"quant_conv/bias": np.zeros(8, np.float32)}
        return StableVAEModel(DPState(p, None, ema_is_params=True), NORM, cfg, TrainStub(), W.VAESpec(), image_size, "cpu",
                              lr_schedule=sched, ema_decay=0.99)
    return make


def _raw(seed, B):
    return rng(seed).integers(0, 256, (B, 2, 64, 64, 3)).astype(np.float32)


def test_update_returns_the_reference_metrics_and_advances_the_step(stub_model):
    m0 = stub_model()
    sched = m0.lr_schedule
    m1, met = m0.update({"obs": {KEY: _raw(1, 2)}}, 7, 0)
    assert list(met) == list(_lib.VAE_METRIC_KEYS) + ["vae_lr", "vae_step"]                     # 13 keys, the reference's order
    assert [float(met[k]) for k in _lib.VAE_METRIC_KEYS] == [float(i + 7) for i in range(11)]
    assert met["vae_lr"] == np.float32(sched(0)) and met["vae_step"] == 0
    m2, met2 = m1.update({"obs": {KEY: _raw(2, 2)}}, 8, 1)
    assert met2["vae_lr"] == np.float32(sched(1)) and met2["vae_step"] == 1 and m2.vae_state.step == 2
    kinds = [c[0] for c in m0._engine.calls]
    # the first step loads the arenas (fresh moments) and enables the EMA; the second trains on what the first left there
    assert kinds == ["load", "ema", "grad", "apply", "grad", "apply"]
    assert [c for c in m0._engine.calls if c[0] == "apply"] == [("apply", "vae", float(np.float32(sched(0)))),
                                                                ("apply", "vae", float(np.float32(sched(1))))]


def test_train_sync_of_the_state_warms_the_arenas_for_the_first_update(stub_model):
    """`model._train_sync(model.vae_state)` is how the GPU suites and tools/vae_train_bench.py load the arenas before a first step."""
    m = stub_model()
    m._train_sync(m.vae_state)
    assert [c[0] for c in m._engine.calls] == ["load", "ema"]
    m.update({"obs": {KEY: _raw(1, 2)}}, 7, 0)
    assert [c[0] for c in m._engine.calls] == ["load", "ema", "grad", "apply"]


def test_update_concatenates_the_cameras_and_passes_use_kl(stub_model):
    m = stub_model((KEY, KEY2), use_kl=False)
    a, b = _raw(3, 2), _raw(4, 2)
    m.update({"obs": {KEY: a, KEY2: b}}, 5, 0, row_offset=9)
    grad = [c for c in m._engine.calls if c[0] == "grad"][0]
    assert grad == ("grad", (4, 64, 64, 3), False, 1e-5, 5, 9)
    img = m._engine.frames.numpy()
    assert np.allclose(img[:2], a[:, 0] / 255 * 2 - 1, atol=1e-6) and np.allclose(img[2:], b[:, 0] / 255 * 2 - 1, atol=1e-6)


def test_only_the_newest_model_is_readable(stub_model):
    m0 = stub_model()
    m1, _ = m0.update({"obs": {KEY: _raw(1, 2)}}, 0, 0)
    m2, _ = m1.update({"obs": {KEY: _raw(1, 2)}}, 0, 1)
    with pytest.raises(RuntimeError, match="superseded"):
        m1.vae_state.params
    with pytest.raises(RuntimeError, match="superseded"):
        m1.vae_state.ema_params
    assert float(m2.vae_state.params["quant_conv/bias"][0]) == 0.0            # read from the parameter arena (which = 0)
    assert float(m2.vae_state.ema_params["quant_conv/bias"][0]) == 4.0        # ... and from the EMA arena (which = 4)
    assert m0.vae_state.params["quant_conv/bias"].shape == (8,)               # the host tree the first model was built with


def test_update_refuses_frame_sizes_it_was_not_built_for(stub_model):
    m = stub_model(image_size=128)
    with pytest.raises(NotImplementedError, match="128-pixel"):
        m.update({"obs": {KEY: _raw(1, 2)}}, 0, 0)
    assert m._engine.calls == []


# ---- 3. FLOPs -----------------------------------------------------------------------------------------------------------------------------
def test_vae_forward_flops_counts_live_taps():
    f = flops.vae_forward_flops(W.VAESpec(), 64)
    assert round(f["encoder"] / 1e9, 1) == 11.0 and round(f["decoder"] / 1e9, 1) == 23.9
    assert f["total"] == f["encoder"] + f["decoder"]
    # a 3x3 at 64 px has 62^2 * 9 + edges: fewer live taps than 9 per pixel
    assert flops._taps_same_2d(64) < 9 * 64 * 64 and flops._taps_down_2d(64) == (32 * 3 - 1) ** 2


# ---- 4. the conditions tests/test_hip_vae_train_full.py rests on --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case_b():
    """Case b (seeded parameters 5, B = 3, beta = 1) through the float64 and float32 chains, once."""
    p, frames, eps, use_kl, beta = VC.case_inputs("b")
    return dict(VC.oracle_run(p, frames, eps, use_kl, beta), params=p, frames=frames, eps=eps, beta=beta)


def test_batch_gradient_is_the_weighted_sum_of_chunk_gradients_in_float64(case_b):
    """The loss is a mean over frames and GroupNorm is per sample: G(batch) = sum_c (|c| / B) G(chunk c), here 2 + 1 frames.  Round-off of the
    float64 chain is ~1e-14 of a leaf's maximum; a coupling between frames would show at O(1)."""
    o = case_b
    chunks = [(hi - lo, VC.oracle_run(o["params"], o["frames"][lo:hi], o["eps"][lo:hi], True, o["beta"], with32=False)["grads"])
              for lo, hi in ((0, 2), (2, 3))]
    comb = VC.combine(chunks)
    worst = max(float(np.abs(g - comb[k]).max()) / max(float(np.abs(g).max()), 1e-300) for k, g in o["grads"].items()
                if not k.endswith("attentions_0/key/bias"))
    print("float64 decomposition residual / leafmax", worst)
    assert worst < 1e-12
    for k, g in o["grads"].items():
        if k.endswith("attentions_0/key/bias"):                    # true gradient 0: round-off on both sides
            assert float(np.abs(g).max()) < 1e-15 and float(np.abs(comb[k]).max()) < 1e-15


def test_clamp_fixture_saturates_two_channels_and_no_others():
    """Case d: log-variance channels 0 / 1 at least 10 beyond the clamp (-30, 20), channels 2 / 3 at least 1 inside it."""
    from oracle import torch32
    p, frames, _, _, _ = VC.case_inputs("d")
    lc = VO.latent_channels(p)
    torch.set_num_threads(16)
    mom = torch32.vae_encode_mean(torch32.TorchParams(p, dtype=torch.float64), torch.tensor(frames, dtype=torch.float64),
                                  latent_channels=2 * lc).numpy()
    lv = mom[..., lc:]
    print("case d log-variance ranges per channel", [(float(lv[..., c].min()), float(lv[..., c].max())) for c in range(lc)])
    assert lv[..., 0].min() >= 30.0 and lv[..., 1].max() <= -40.0
    assert lv[..., 2:].min() >= -29.0 and lv[..., 2:].max() <= 19.0


def test_kl_term_dominates_the_encoder_gradients_at_beta_1(case_b):
    """What case b relies on: at beta = 1 switching the KL term off moves at least 90 % of the encoder / quant_conv leaves by more than
    100 x the bound the GPU test applies to them (at beta = 1e-5 it moves 140 of 332 leaves by at most 4 x the bound)."""
    o = case_b
    off = VC.oracle_run(o["params"], o["frames"], o["eps"], False, o["beta"], with32=False)["grads"]
    enc = [k for k in o["grads"] if k.startswith(("encoder/", "quant_conv/"))]
    ratio = np.asarray([float(np.abs(o["grads"][k] - off[k]).max()) / VC.leaf_bound(o["grads"][k], o["err32"][k]) for k in enc])
    print(f"KL on/off at beta = 1: {int((ratio > 100).sum())} of {len(enc)} encoder leaves move by > 100 x their bound, median {np.median(ratio):.0f} x")
    assert len(enc) == 142 and (ratio > 100).sum() >= 0.9 * len(enc)
