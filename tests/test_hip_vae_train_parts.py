"""ldp_train_vae_grad_part and StableVAEModel.update(chunk=...) on the GPU: the gradient of part of a batch, scaled for the whole batch and
added to the gradient arena.  -m gpu.  64-pixel frames, at most 33 of them.

The bounds are the project's own: the per-leaf gradient rule of tests/test_hip_vae_train.py against the float64 golden of the ONE-call
gradient (max(1e-4 leafmax64, 3 err32_leaf) + 1e-12), its _check_metrics, its digest rule at 1e-5 for parameters and EMA."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from latent_diffusion_planning_amd import _lib, weights as W
from tests import vae_train_oracle as VT
from tests.golden.make_golden_vae_update import DIGEST_SEED, KEY, normalised, raw_frames
from tests.test_hip_vae_train import _assert_digest, _check_metrics, _f32, _golden, _grads, _model
from tests.util import tree_digest

pytestmark = pytest.mark.gpu


def _b2():
    z, p = _golden("vae_update_seeded_b2")
    B = int(z["seed_B"])
    model = _model(p)
    model._train_sync(model.vae_state)
    img = _f32(normalised(raw_frames(int(z["seed_frames"][0]), B))).cuda()
    return model, model._engine, img, _f32(z["out_eps"][0]).cuda(), B


def _arena(eng):
    return eng.train_arena("vae", eng.TRAIN_GRADS).clone()


# ---- 1. the existing call is the part with n_total = N, accumulate = 0 -----------------------------------------------------------------
def test_part_of_the_whole_batch_is_bitwise_train_vae_grad():
    model, eng, img, eps, B = _b2()
    m0 = eng.train_vae_grad(img, True, VT.BETA, noise=eps).clone()
    a0 = _arena(eng)
    eng.train_vae_grad_part(img, 2 * B, False, True, VT.BETA, noise=eps)       # other gradients in the arena: accumulate = 0 replaces them
    assert not torch.equal(_arena(eng), a0)
    m1 = eng.train_vae_grad_part(img, B, False, True, VT.BETA, noise=eps).clone()
    a1 = _arena(eng)
    torch.cuda.synchronize()
    assert torch.equal(m0, m1) and torch.equal(a0, a1)
    assert bool(torch.isfinite(a0).all()) and float(a0.abs().max()) > 0
    eng.close()


# ---- 2. the scale is exact, and so is the accumulate kernel ---------------------------------------------------------------------------------
def test_twice_the_batch_halves_the_arena_and_two_halves_add_up_to_it():
    model, eng, img, eps, B = _b2()
    eng.train_vae_grad_part(img, B, False, True, VT.BETA, noise=eps)
    whole = _arena(eng)
    m_half = eng.train_vae_grad_part(img, 2 * B, False, True, VT.BETA, noise=eps).clone()
    half = _arena(eng)
    big = whole.abs() > 1e-30
    print("scaling", json.dumps(dict(entries=int(whole.numel()), above_1e30=int(big.sum()), nonzero=int((whole != 0).sum()))))
    assert int(big.sum()) > 0.9 * int((whole != 0).sum())
    assert torch.equal(half[big], (0.5 * whole)[big])               # 0.5 is a power of two: the same bits, one exponent down
    m_acc = eng.train_vae_grad_part(img, 2 * B, True, True, VT.BETA, noise=eps).clone()       # the same part again, ADDED: x / 2 + x / 2
    both = _arena(eng)
    torch.cuda.synchronize()
    diff = both != whole
    print("accumulate", json.dumps(dict(entries_that_differ=int(diff.sum()))))
    assert torch.equal(both, whole)
    assert torch.equal(m_half, m_acc)                               # the metrics are the part's own: n_total and accumulate do not enter
    eng.close()


# ---- 3. chunked updates against the golden of the one-call gradient ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def b33():
    """The golden, its parameters, the batch, and the digests of parameters and EMA after ONE unchunked update."""
    z, p = _golden("vae_update_seeded_b33")
    B = int(z["seed_B"])
    batch = {"obs": {KEY: raw_frames(int(z["seed_frames"][0]), B)}}
    model = _model(p)
    new, _ = model.update(batch, 0, 0, noise=z["out_eps"][0])
    ref = dict(params=tree_digest(new.vae_state.params, DIGEST_SEED), ema=tree_digest(new.vae_state.ema_params, DIGEST_SEED))
    model._engine.close()
    return dict(z=z, p=p, B=B, batch=batch, ref=ref)


@pytest.mark.parametrize("chunk,parts", [(32, (32, 1)), (16, (16, 16, 1)), (8, (8, 8, 8, 8, 1))])
def test_chunked_update_matches_the_one_call_golden(b33, chunk, parts):
    z, B = b33["z"], b33["B"]
    model = _model(b33["p"])
    eng = model._engine
    seen, grads = [], {}
    part, apply = eng.train_vae_grad_part, eng.train_apply

    def spy_part(img, n_total, accumulate, *a, **k):
        seen.append((int(img.shape[0]), int(n_total), int(accumulate), int(k["row_offset"])))
        return part(img, n_total, accumulate, *a, **k)

    def spy_apply(*a, **k):                                          # the gradient arena as Adam is about to read it
        grads.update(_grads(model))
        return apply(*a, **k)
    eng.train_vae_grad_part, eng.train_apply = spy_part, spy_apply
    new, m = model.update(b33["batch"], 0, 0, noise=z["out_eps"][0], chunk=chunk)
    offs = np.concatenate([[0], np.cumsum(parts)[:-1]])
    assert seen == [(n, B, int(i > 0), int(o)) for i, (n, o) in enumerate(zip(parts, offs))]
    got = tree_digest(grads, DIGEST_SEED)
    ref = z["out_gdig"].astype(np.float64)
    bound = np.maximum(1e-4 * ref[:, 1], 3 * z["out_err32"])[:, None] + 1e-12
    ratio = np.abs(got[:, 3:] - ref[:, 3:]) / bound
    names = list(W.vae_shapes(W.VAESpec()))
    worst = int(ratio.max(axis=1).argmax())
    print(f"chunk {chunk} gradients", json.dumps(dict(worst_err_over_bound=float(ratio.max()), leaf=names[worst])))
    assert float(ratio.max()) <= 1.0, (chunk, names[worst], float(ratio.max()))
    key_bias = [i for i, k in enumerate(names) if k.endswith("attentions_0/key/bias")]
    assert all(float(np.abs(grads[names[i]]).max()) == 0.0 for i in key_bias)       # exact zeros add up to exact zeros
    _check_metrics(np.asarray([float(m[k]) for k in _lib.VAE_METRIC_KEYS]), z)
    assert new.vae_state.step == 1 and m["vae_step"] == 0
    _assert_digest(new.vae_state.params, b33["ref"]["params"], DIGEST_SEED, 1e-5, f"params, chunk {chunk}")
    _assert_digest(new.vae_state.ema_params, b33["ref"]["ema"], DIGEST_SEED, 1e-5, f"EMA, chunk {chunk}")
    eng.close()


# ---- 4. determinism ----------------------------------------------------------------------------------------------------------------------
def test_the_same_parts_twice_give_the_same_bits(b33):
    z, B = b33["z"], b33["B"]
    model = _model(b33["p"])
    model._train_sync(model.vae_state)
    eng = model._engine
    img = _f32(normalised(b33["batch"]["obs"][KEY])).cuda()
    runs = []
    for _ in range(2):
        ms = [eng.train_vae_grad_part(img[lo:hi], B, lo > 0, True, VT.BETA, seed=3, row_offset=lo).clone() for lo, hi in ((0, 16), (16, 32), (32, 33))]
        runs.append((torch.stack(ms), _arena(eng)))
    torch.cuda.synchronize()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert bool(torch.isfinite(runs[0][1]).all()) and float(runs[0][1].abs().max()) > 0
    # the padding between the leaves stays zero through the additions: nothing but the leaves is non-zero
    leaves = _grads(model)
    tot = sum(float(np.abs(v.astype(np.float64)).sum()) for v in leaves.values())
    assert abs(float(runs[1][1].double().abs().sum()) - tot) <= 1e-6 * tot
    eng.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_part_refusals_name_the_limit():
    model = _model(W.init_vae_params(seed=5))
    model._train_sync(model.vae_state)
    eng = model._engine
    img = torch.zeros((2, 64, 64, 3), device="cuda")
    with pytest.raises(_lib.LDPHipError, match="n_total = 1, at least the 2 frames") as e:
        eng.train_vae_grad_part(img, 1, False, True, VT.BETA)
    assert e.value.code == -1
    with pytest.raises(_lib.LDPHipError, match="at most 256") as e:
        eng.train_vae_grad_part(torch.zeros((257, 64, 64, 3), device="cuda"), 300, False, True, VT.BETA)
    assert e.value.code == -1
    with pytest.raises(_lib.LDPHipError, match="accumulate = 2, it is 0 .* or 1") as e:
        eng.train_vae_grad_part(img, 2, 2, True, VT.BETA)
    assert e.value.code == -1
    out = torch.zeros((11,), device="cuda")
    code = eng.lib.ldp_train_vae_grad_part(eng._h, C.c_void_p(img.data_ptr()), 0, 2, 0, 1, C.c_float(VT.BETA), None, C.c_uint64(0), C.c_int64(0),
                                           C.c_void_p(out.data_ptr()), eng._stream())
    assert code == -1 and b"1 to 256" in eng.lib.ldp_last_error()
    eng.close()
