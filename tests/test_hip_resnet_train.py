"""The ResNet-18 encoder's training tape on the GPU (csrc/resnet_train.hpp: ldp_train_encoder_forward / _backward and module bits 8 << slot)
against float64 autograd (tests/dp_train_oracle.py), on a handle with encoders only.

Error rule, per entry of every leaf: |got - ref64| <= max(1e-4 * leafmax64, 3 * err32_leaf) + 1e-12, err32_leaf = the float32
autograd restatement's worst error on that leaf, computed here on the CPU.  Every test prints the worst ratio and the leaf it falls on."""
import functools

import numpy as np
import pytest
import torch

from latent_diffusion_planning_amd import weights as W
from tests import dp_resnet_oracle as RO
from tests import dp_train_oracle as TO
from tests.golden.make_golden_dp_resnet import frames_to_input
from tests.util import rng

pytestmark = pytest.mark.gpu

SHAPES = W.resnet_shapes()
N_ENTRIES = sum(int(np.prod(s)) for s in SHAPES.values())


@functools.lru_cache(maxsize=None)
def _engine():
    from latent_diffusion_planning_amd.engine import HipEngine
    return HipEngine(obs_dim=7, action_dim=7, global_cond_dim=1033, pred_horizon=16, action_horizon=8)


def _params(kind, seed):
    if kind == "heavy":
        return RO.heavy_params(seed)
    p = {k: np.asarray(v, np.float32) for k, v in W.init_resnet_params(RO.SPEC, seed=seed, perturb=True).items()}
    if kind == "logits80":                                # the last feature map scaled so that the softmax inputs reach +-80
        p["ResNetBlock_7/MyGroupNorm_1/scale"] = p["ResNetBlock_7/MyGroupNorm_1/scale"] * np.float32(_logit_scale(seed))
    return p


@functools.lru_cache(maxsize=None)
def _logit_scale(seed):
    """The factor on the last norm's scale that brings the largest softmax input to 80 (the residual is not scaled: a few secant steps)."""
    p = {k: np.asarray(v, np.float32) for k, v in W.init_resnet_params(RO.SPEC, seed=seed, perturb=True).items()}
    x, key = frames_to_input(RO.synth_frames(3, seed)), "ResNetBlock_7/MyGroupNorm_1/scale"

    def top(f):
        q = dict(p)
        q[key] = p[key] * np.float32(f)
        return float(np.abs(RO.encode(q, x, torch.float64, return_logits=True)[1]).max())
    f0, f1 = 1.0, 10.0
    y0, y1 = top(f0), top(f1)
    for _ in range(8):
        if abs(y1 - 80.0) < 0.5:
            break
        f0, f1, y0 = f1, f1 + (80.0 - y1) * (f1 - f0) / (y1 - y0), y1
        y1 = top(f1)
    return f1


@functools.lru_cache(maxsize=None)
def _case(kind, N, seed):
    """Inputs and both CPU references of one VJP case (computed once, shared, never modified)."""
    p = _params(kind, seed)
    x = frames_to_input(RO.synth_frames(N, seed))
    dfeat = rng(seed + 77).standard_normal((N, RO.FEAT)).astype(np.float32)
    f64, g64, last = TO.encoder_vjp(p, x, dfeat, torch.float64)
    f32, g32, _ = TO.encoder_vjp(p, x, dfeat, torch.float32)
    return dict(p=p, x=x, dfeat=dfeat, f64=f64, f32=f32, g64=g64, g32=g32, last=last)


def _vjp(eng, slot, c, load=True):
    name = f"encoder{slot}"
    if load:
        eng.train_load(name, c["p"])
    feat = eng.train_encoder_forward(slot, torch.tensor(c["x"], device="cuda"))
    eng.train_encoder_backward(slot, torch.tensor(c["dfeat"], device="cuda"))
    return feat.cpu().numpy(), eng.train_read(name, eng.TRAIN_GRADS, SHAPES)


def _check_grads(what, got, c):
    worst, where, n = 0.0, None, 0
    for k in SHAPES:
        ref, g32 = c["g64"][k], c["g32"][k]
        bound = max(1e-4 * np.abs(ref).max(), 3.0 * np.abs(g32 - ref).max()) + 1e-12
        err = np.abs(got[k].astype(np.float64) - ref).max()
        assert np.isfinite(got[k]).all(), f"{what}: {k} is not finite"
        n += ref.size
        if err / bound > worst:
            worst, where = err / bound, k
    print(f"{what}: {n} entries, worst error / bound = {worst:.3f} on {where}")
    assert n == N_ENTRIES == 11176512
    assert worst <= 1.0, f"{what}: error / bound = {worst:.3f} on {where}"


def _check_feat(what, got, c):
    err32 = float(np.abs(c["f32"] - c["f64"]).max())
    bound = max(1e-5, 3.0 * err32)
    err = float(np.abs(got.astype(np.float64) - c["f64"]).max())
    print(f"{what}: features err {err:.3e}, err32 {err32:.3e}, bound {bound:.3e}")
    assert np.isfinite(err) and err <= bound
    return bound


@pytest.mark.parametrize("N", [1, 6, 33])
def test_forward_and_vjp_match_float64(N):
    """N = 1: 31 of 32 rows are padding and must contribute exactly nothing; N = 33: two row tiles, the second with one live row."""
    eng, c = _engine(), _case("perturbed", N, 900 + N)
    feat, g = _vjp(eng, 0, c)
    bound = _check_feat(f"N={N}", feat, c)
    eng.load_encoder(0, c["p"])                           # the sampling path on the same leaves
    enc = eng.resnet_encode(0, torch.tensor(c["x"], device="cuda")).cpu().numpy()
    err = float(np.abs(enc.astype(np.float64) - feat).max())
    print(f"N={N}: training forward vs ldp_resnet_encode {err:.3e}")
    assert err <= bound
    _check_grads(f"N={N}", g, c)


def test_heavy_tailed_parameters():
    """Mean >> spread groups and O(10) norm biases: where a one-pass variance or an unmasked ReLU shows."""
    eng, c = _engine(), _case("heavy", 3, 940)
    feat, g = _vjp(eng, 0, c)
    _check_feat("heavy", feat, c)
    _check_grads("heavy", g, c)


def test_large_logits_stay_finite():
    eng, c = _engine(), _case("logits80", 3, 950)
    assert 79.0 <= np.abs(c["last"]).max() <= 81.0
    feat, g = _vjp(eng, 0, c)
    assert np.isfinite(feat).all()
    _check_feat("logits +-80", feat, c)
    _check_grads("logits +-80", g, c)


def _arena(eng, slot):
    return eng.train_arena(f"encoder{slot}", eng.TRAIN_GRADS).clone()


def test_determinism_and_slot_independence():
    eng, a, b = _engine(), _case("perturbed", 6, 906), _case("heavy", 3, 940)
    _vjp(eng, 0, a)
    g0 = _arena(eng, 0)
    _vjp(eng, 0, a, load=False)
    assert torch.equal(_arena(eng, 0), g0), "two identical calls differ"
    _vjp(eng, 2, a)
    assert torch.equal(_arena(eng, 2), g0), "slot 2 differs from slot 0 on the same leaves and frames"
    # two tapes alive together: forward 0, forward 1, backward 0, backward 1 = each run apart
    _vjp(eng, 1, b)
    g1 = _arena(eng, 1)
    eng.train_arena("encoder0", eng.TRAIN_GRADS).zero_()
    eng.train_arena("encoder1", eng.TRAIN_GRADS).zero_()
    dev = lambda v: torch.tensor(v, device="cuda")
    fa = eng.train_encoder_forward(0, dev(a["x"]))
    fb = eng.train_encoder_forward(1, dev(b["x"]))
    eng.train_encoder_backward(0, dev(a["dfeat"]))
    eng.train_encoder_backward(1, dev(b["dfeat"]))
    assert torch.equal(_arena(eng, 0), g0) and torch.equal(_arena(eng, 1), g1), "interleaved tapes disturb each other"
    assert np.isfinite(fa.cpu().numpy()).all() and np.isfinite(fb.cpu().numpy()).all()


def test_return_codes():
    from latent_diffusion_planning_amd._lib import LDPHipError
    from latent_diffusion_planning_amd.engine import HipEngine
    eng = HipEngine(obs_dim=7, action_dim=7, global_cond_dim=1033, pred_horizon=16, action_horizon=8)
    with pytest.raises(LDPHipError) as e:
        eng.train_init(["encoder3"])                      # an empty slot
    assert e.value.code == -2
    c = _case("perturbed", 1, 901)
    eng.train_load("encoder0", c["p"])
    with pytest.raises(LDPHipError) as e:
        eng.train_encoder_backward(0, torch.zeros((1, 1024), device="cuda"))
    assert e.value.code == -2                             # LDP_ESTATE: no forward yet
    for n in (0, 1025):
        with pytest.raises(LDPHipError) as e:
            eng.train_encoder_forward(0, torch.zeros((n, 64, 64, 3), device="cuda"))
        assert e.value.code == -1
    assert "1024" in str(e.value)
    eng.train_encoder_forward(0, torch.tensor(c["x"], device="cuda"))
    with pytest.raises(LDPHipError) as e:
        eng.train_encoder_backward(0, torch.zeros((2, 1024), device="cuda"))      # not the forward's N
    assert e.value.code == -2
    eng.train_encoder_backward(0, torch.tensor(c["dfeat"], device="cuda"))


def test_adam_ema_publish_on_an_encoder_module():
    """The encoders take part in the shared optimiser / hand-off code: one Adam step moves every entry by ~lr, the EMA follows, and publishing
    makes ldp_resnet_encode run on the trained leaves (bit-equal to uploading them)."""
    eng, c = _engine(), _case("perturbed", 6, 906)
    eng.train_load("encoder1", c["p"])
    eng.train_ema("encoder1", 0.99)
    x = torch.tensor(c["x"], device="cuda")
    eng.train_encoder_forward(1, x)
    eng.train_encoder_backward(1, torch.tensor(c["dfeat"], device="cuda"))
    lr = 1e-3
    eng.train_apply("encoder1", lr)
    assert eng.train_step_count("encoder1") == 1
    new = eng.train_read("encoder1", eng.TRAIN_PARAMS, SHAPES)
    ema = eng.train_read("encoder1", eng.TRAIN_EMA, SHAPES)
    for k in SHAPES:
        d = new[k].astype(np.float64) - c["p"][k]
        assert 0.9 * lr <= np.abs(d).max() <= 1.1 * lr, k
        assert np.allclose(ema[k], 0.99 * c["p"][k].astype(np.float64) + 0.01 * new[k], rtol=0, atol=1e-6), k
    eng.train_publish(["encoder1"])
    got = eng.resnet_encode(1, x)
    eng.load_encoder(3, new)
    assert torch.equal(got, eng.resnet_encode(3, x))
