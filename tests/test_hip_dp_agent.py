"""DPAgent on the GPU: the primitives of the ResNet-18 image encoder (csrc/resnet.hip) and ldp_resnet_encode against the float64 oracle
of tests/dp_resnet_oracle.py, DPAgent.sample / get_metrics against the float64 goldens, and the plumbing around them.

Bound of a primitive and of the encoder (the project's rule): max(1e-5, 3 * err32) relative to max(1, |ref|), err32 = the
error of the float32 restatement against float64, computed here on the CPU."""
import functools

import numpy as np
import pytest
import torch

from tests import dp_resnet_oracle as RO
from tests.golden.make_golden_dp_resnet import AH, OH, T, frames_to_input, feature_params, golden_path, rel_err, step_noise
from tests.util import rng

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.tensor(np.asarray(a, np.float32), device="cuda")


def _check(what, got, ref64, ref32):
    err32 = rel_err(ref32, ref64)
    err = rel_err(got.cpu().numpy() if torch.is_tensor(got) else got, ref64)
    bound = max(1e-5, 3.0 * err32)
    print(f"{what}: err {err:.3e}, err32 {err32:.3e}, bound {bound:.3e}")
    assert np.isfinite(err) and err <= bound, f"{what}: err {err:.3e} > bound {bound:.3e} (err32 {err32:.3e})"


def _kaiming(g, shape):
    return (g.standard_normal(shape) * np.sqrt(2.0 / (shape[0] * shape[1] * shape[2]))).astype(np.float32)


# ---- primitives ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 3])
def test_stem_conv7x7_s2(N):
    from latent_diffusion_planning_amd import engine as E
    g = rng(10 + N)
    x = g.uniform(-1, 1, (N, 64, 64, 3)).astype(np.float32)
    k = _kaiming(g, (7, 7, 3, 64))
    y = E.resnet_conv7x7_s2(_dev(x), k)
    assert tuple(y.shape) == (N, 32, 32, 64)
    _check(f"stem N={N}", y, RO.conv7x7_s2(x, k), RO.conv7x7_s2(x, k, torch.float32))


@pytest.mark.parametrize("N,H,cin,cout", [(3, 16, 64, 128), (1, 4, 256, 512)])
def test_conv1x1_s2(N, H, cin, cout):
    from latent_diffusion_planning_amd import engine as E
    g = rng(20 + H)
    x = g.standard_normal((N, H, H, cin)).astype(np.float32)
    k = _kaiming(g, (1, 1, cin, cout))
    y = E.resnet_conv1x1_s2(_dev(x), k)
    assert tuple(y.shape) == (N, H // 2, H // 2, cout)
    _check(f"conv1x1 s2 {cin}->{cout} at {H} px", y, RO.conv1x1_s2(x, k), RO.conv1x1_s2(x, k, torch.float32))


def test_maxpool_all_negative_map():
    from latent_diffusion_planning_amd import engine as E
    x = -rng(30).uniform(0.5, 3.0, (2, 32, 32, 64)).astype(np.float32)
    y = E.resnet_maxpool3x3_s2(_dev(x)).cpu().numpy()
    ref = RO.maxpool(x)
    assert y.shape == (2, 16, 16, 64) and (y < 0).all()              # zero padding would give 0 in the last row and column
    assert np.array_equal(y.astype(np.float64), ref)                 # a maximum has no rounding


def _gn_inputs(seed, N=3, H=8, C=64, mean=0.0, spread=1.0):
    g = rng(seed)
    x = (mean + spread * g.standard_normal((N, H, H, C))).astype(np.float32)
    sc = (1 + 0.1 * g.standard_normal(C)).astype(np.float32)
    bi = (0.02 * g.standard_normal(C)).astype(np.float32)
    return g, x, sc, bi


@pytest.mark.parametrize("mode", ["plain", "relu", "res", "fused", "mean100"])
def test_group_norm(mode):
    from latent_diffusion_planning_amd import engine as E
    if mode == "mean100":
        g, x, sc, bi = _gn_inputs(44, mean=100.0, spread=1e-3)       # 12 groups whose mean is 1e5 spreads away
    else:
        g, x, sc, bi = _gn_inputs(40)
    kw = {}
    if mode in ("relu", "res", "fused"):
        kw["relu"] = True
    if mode in ("res", "fused"):
        kw["res"] = (3.0 + 2.0 * g.standard_normal(x.shape)).astype(np.float32)
    if mode == "fused":
        kw["scale2"] = (1 + 0.1 * g.standard_normal(x.shape[-1])).astype(np.float32)
        kw["bias2"] = (0.02 * g.standard_normal(x.shape[-1])).astype(np.float32)
    dkw = dict(kw)
    if "res" in dkw:
        dkw["res"] = _dev(dkw["res"])
    y = E.resnet_gn(_dev(x), sc, bi, 4, 1e-5, **dkw)
    _check(f"GroupNorm {mode}", y, RO.gn(x, sc, bi, **kw), RO.gn(x, sc, bi, dtype=torch.float32, **kw))


def test_group_norm_in_place():
    from latent_diffusion_planning_amd import _lib, engine as E
    import ctypes as C
    g, x, sc, bi = _gn_inputs(46)
    xd = _dev(x)
    want = E.resnet_gn(xd, sc, bi, relu=True)
    lib = _lib.load()
    s, b = np.ascontiguousarray(sc), np.ascontiguousarray(bi)
    _lib.check(lib.ldp_resnet_gn_f32(C.c_void_p(xd.data_ptr()), None, C.c_void_p(xd.data_ptr()), s.ctypes.data_as(C.c_void_p),
                                     b.ctypes.data_as(C.c_void_p), None, None, 3, 64, 64, 4, C.c_float(1e-5), 1,
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert torch.equal(xd, want)


def test_spatial_softmax_large_logits_and_corner():
    from latent_diffusion_planning_amd import engine as E
    g = rng(50)
    x = g.uniform(-80, 80, (3, 2, 2, 512)).astype(np.float32)
    y = E.resnet_spatial_softmax(_dev(x))
    assert tuple(y.shape) == (3, 1024) and bool(torch.isfinite(y).all())
    _check("spatial softmax +-80", y, RO.spatial_softmax(x), RO.spatial_softmax(x, torch.float32))
    # all mass in the top-right corner (row 0, last column): expected_x = +1, expected_y = -1
    c = np.full((1, 2, 2, 8), -50.0, np.float32)
    c[0, 0, 1, :] = 50.0
    yc = E.resnet_spatial_softmax(_dev(c)).cpu().numpy()
    assert np.allclose(yc[0, :8], 1.0, atol=1e-6) and np.allclose(yc[0, 8:], -1.0, atol=1e-6)


# ---- ldp_resnet_encode -----------------------------------------------------------------------------------------------------------------
def _engine():
    from latent_diffusion_planning_amd.engine import HipEngine
    return HipEngine(obs_dim=7, action_dim=7, global_cond_dim=1033, pred_horizon=16, action_horizon=8)


@functools.lru_cache(maxsize=None)
def _feature_golden(kind):
    z = np.load(golden_path(f"dp_resnet_features_{kind}"))
    return z["in_frames"], feature_params(kind, int(z["seed_params"])), z["out_features"], z["out_features32"]


@pytest.mark.parametrize("kind", ["perturbed", "heavy"])
def test_resnet_encode_matches_golden(kind):
    frames, p, f64, f32 = _feature_golden(kind)
    eng = _engine()
    eng.load_encoder(0, p)
    img = _dev(frames_to_input(frames))
    got = eng.resnet_encode(0, img)
    assert tuple(got.shape) == (5, 1024)
    _check(f"resnet_encode {kind} N=5", got, f64, f32)
    one = eng.resnet_encode(0, img[:1].contiguous())
    _check(f"resnet_encode {kind} N=1", one, f64[:1], f32[:1])
    again = eng.resnet_encode(0, img)
    torch.cuda.synchronize()
    assert torch.equal(got, again)                                   # two runs: the same bits
    assert torch.equal(one, got[:1])                                 # a frame's features do not depend on its batch
    eng.close()


def test_resnet_encode_chunk_seam_is_bitwise():
    from latent_diffusion_planning_amd._lib import RESNET_CHUNK
    frames, p, _, _ = _feature_golden("perturbed")
    eng = _engine()
    eng.load_encoder(0, p)
    N = RESNET_CHUNK + 1
    img = _dev(frames_to_input(np.concatenate([frames] * (N // 5 + 1))[:N]))
    img = img + 0.01 * torch.arange(N, device="cuda", dtype=torch.float32).reshape(N, 1, 1, 1) / N      # no two frames alike
    whole = eng.resnet_encode(0, img)
    parts = torch.cat([eng.resnet_encode(0, img[:40].contiguous()), eng.resnet_encode(0, img[40:].contiguous())])
    torch.cuda.synchronize()
    assert torch.equal(whole, parts)
    eng.close()


def test_resnet_encode_slots_and_call_order():
    from latent_diffusion_planning_amd._lib import LDPHipError
    frames, p, _, _ = _feature_golden("perturbed")
    _, ph, _, _ = _feature_golden("heavy")
    eng = _engine()
    img = _dev(frames_to_input(frames))
    with pytest.raises(LDPHipError) as e:
        eng.resnet_encode(0, img)
    assert e.value.code == -2                                        # LDP_ESTATE before finalize
    eng.load_encoder(0, p)
    a0 = eng.resnet_encode(0, img)
    with pytest.raises(LDPHipError) as e:
        eng.resnet_encode(1, img)                                    # slot 1 has no leaves yet
    assert e.value.code == -2
    with pytest.raises(LDPHipError) as e:
        eng.resnet_encode(4, img)
    assert e.value.code == -1                                        # LDP_EINVAL: no such slot
    eng.load_encoder(1, ph)
    b1 = eng.resnet_encode(1, img)
    b0 = eng.resnet_encode(0, img)
    torch.cuda.synchronize()
    assert torch.equal(a0, b0) and not torch.equal(b0, b1)
    assert eng.encoder_uploads == [1, 1, 0, 0]
    eng.close()


# ---- DPAgent -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _agent(cfg="rm_img", shared=False):
    """One agent (one engine handle) per configuration for the whole module: creating one draws and uploads 65 M U-Net parameters."""
    from latent_diffusion_planning_amd.dp_agent import DPAgent
    data = RO.BY_NAME[cfg]
    return DPAgent.create(0, None, data["shape_meta"], **RO.dp_kwargs(data, OH, T, AH, shared_encoder=shared))


@functools.lru_cache(maxsize=None)
def _planner_params(cfg, seed):
    return RO.planner_params(RO.BY_NAME[cfg], seed, OH)


def _with_params(ag, p, enc):
    return ag.replace(planner_state=ag.planner_state.replace(params=p, ema_params=p),
                      encoder_state_dict={k: ag.encoder_state_dict[k].replace(params=enc[k], ema_params=enc[k]) for k in enc})


def _case(name):
    z = np.load(golden_path(name))
    cfg = "rm_img2" if "rm_img2" in name else "rm_img"
    shared = "shared" in name
    data = RO.BY_NAME[cfg]
    ag = _with_params(_agent(cfg, shared), _planner_params(cfg, int(z["seed_params"])), RO.encoder_params(data, int(z["seed_encoder"]), shared))
    obs = {k[len("in_obs__"):]: z[k] for k in z.files if k.startswith("in_obs__")}
    return z, data, ag, obs


def _check_obs_stats(m, cond64):
    want = RO.stats(cond64)
    for s, v in want.items():
        assert abs(float(m[f"obs_{s}"]) - v) < 1e-4, (s, float(m[f"obs_{s}"]), v)


SAMPLE_GOLDENS = ["dp_resnet_sample_rm_img_ddpm100_b3", "dp_resnet_sample_rm_img_ddim50_b2", "dp_resnet_sample_rm_img2_ddpm100_b2",
                  "dp_resnet_sample_rm_img2_shared_ddim50_b2"]


@pytest.mark.parametrize("name", SAMPLE_GOLDENS)
def test_sample_matches_golden(name):
    z, data, ag, obs = _case(name)
    sampler = "ddim" if "ddim" in name else "ddpm"
    n_steps = 50 if "ddim50" in name else 100
    B, A = z["in_x_init"].shape[0], 7
    noise = dict(x_init=z["in_x_init"])
    if sampler == "ddpm":
        noise["x_noise"] = step_noise(int(z["seed_noise"]), n_steps, B, A)
    act, m = ag.sample({"obs": obs}, 0, noise=noise, sampler=sampler, n_steps=n_steps)
    got = np.array(act)
    assert got.shape == (B, AH, A)
    err = float(np.abs(got - z["out_action"]).max())
    print(f"{name}: max |diff| {err:.3e} (float32 restatement {float(z['out_err32']):.3e})")
    assert err < 1e-4, f"{name}: max |diff| {err:.3e}"
    assert sorted(m) == sorted(["obs_min", "obs_max", "obs_mean", "obs_std"] + [f"{k}_{s}" for k in obs for s in ("min", "max")])
    _check_obs_stats(m, z["out_cond"])
    nobs = RO.normalized_obs(data, obs)
    for k in obs:
        assert abs(float(m[f"{k}_min"]) - nobs[k].min()) < 1e-6 and abs(float(m[f"{k}_max"]) - nobs[k].max()) < 1e-6


def test_sample_is_plan_sample_on_the_oracle_layout():
    z, data, ag, obs = _case("dp_resnet_sample_rm_img_ddim50_b2")
    eng = ag._engine
    got, _ = ag.sample({"obs": obs}, 5, noise=dict(x_init=z["in_x_init"]), sampler="ddim", n_steps=50)
    got = torch.as_tensor(np.array(got))
    nb = ag._postprocess({"obs": obs})
    frames = nb["obs"]["agentview_image"][:, :OH].reshape(-1, 64, 64, 3).contiguous()
    feats = eng.resnet_encode(0, frames).cpu().numpy()
    cond = RO.obs_cond_from_features(data, {k: v.cpu().numpy() for k, v in nb["obs"].items()}, {"agentview_image": feats}, OH, False)
    assert cond.shape == (2, 2 * 1033) and cond.dtype == np.float32
    x = eng.plan_sample(_dev(cond), x_init=_dev(z["in_x_init"]), sampler="ddim", n_steps=50, seed=5)
    ref = eng.normalize_bounds(x[:, :AH].contiguous(), [-1.0], [1.0], 2).cpu()
    assert torch.equal(got, ref)
    assert torch.equal(ag.get_obs_cond(nb["obs"]).cpu(), torch.tensor(cond))


def test_rows_do_not_depend_on_row_offset_sharding():
    _, data, ag, _ = _case("dp_resnet_sample_rm_img_ddim50_b2")
    obs = RO.synth_image_batch(data, 5, OH, 77)["obs"]
    kw = dict(sampler="ddim", n_steps=10)
    full = np.array(ag.sample({"obs": obs}, 99, **kw)[0])
    a = np.array(ag.sample({"obs": {k: v[:2] for k, v in obs.items()}}, 99, row_offset=0, **kw)[0])
    b = np.array(ag.sample({"obs": {k: v[2:] for k, v in obs.items()}}, 99, row_offset=2, **kw)[0])
    assert np.array_equal(full, np.concatenate([a, b]))
    assert not np.array_equal(full, np.array(ag.sample({"obs": obs}, 98, **kw)[0]))
    assert np.array_equal(full, np.array(ag.sample_action({"obs": obs}, 99, **kw)[0]))
    assert np.array_equal(full, np.array(ag.get_action({"obs": obs}, 99, **kw)))


def test_only_a_replaced_encoder_is_uploaded_again():
    z, data, ag, obs = _case("dp_resnet_sample_rm_img2_ddpm100_b2")
    eng = ag._engine
    kw = dict(sampler="ddim", n_steps=10)
    first = np.array(ag.sample({"obs": obs}, 1, **kw)[0])
    base = list(eng.encoder_uploads)
    same = np.array(ag.sample({"obs": obs}, 1, **kw)[0])
    assert eng.encoder_uploads == base and np.array_equal(first, same)           # nothing changed: nothing is uploaded
    wrist = "robot0_eye_in_hand_image"
    other = RO.W.init_resnet_params(RO.SPEC, seed=991, perturb=True)
    esd = dict(ag.encoder_state_dict)
    esd[wrist] = esd[wrist].replace(params=other, ema_params=other)
    ag2 = ag.replace(encoder_state_dict=esd)
    moved = np.array(ag2.sample({"obs": obs}, 1, **kw)[0])
    assert eng.encoder_uploads == [base[0], base[1] + 1, 0, 0]                    # slot 1 = the second camera key, and only it
    assert eng.loaded["encoder0"] == ag2.encoder_state_dict["agentview_image"].version
    assert eng.loaded["encoder1"] == ag2.encoder_state_dict[wrist].version
    assert not np.array_equal(first, moved)
    back = np.array(ag.sample({"obs": obs}, 1, **kw)[0])                          # the first agent shares the engine: its own tree comes back
    assert eng.encoder_uploads == [base[0], base[1] + 2, 0, 0] and np.array_equal(first, back)


def test_get_metrics_matches_golden_and_harness():
    from latent_diffusion_planning_amd import harness
    z, data, ag, obs = _case("dp_resnet_metrics_rm_img_b3")
    batch = {"obs": obs, "actions": z["in_actions"]}
    m = ag.get_metrics(batch, 0, noise=dict(t=z["in_t"].astype(np.int64), noise=z["in_noise"]))
    assert sorted(m) == ["loss", "obs_max", "obs_mean", "obs_min", "obs_std"]
    print(f"loss {float(m['loss']):.8f} golden {float(z['out_loss']):.8f}")
    np.testing.assert_allclose(float(m["loss"]), float(z["out_loss"]), rtol=1e-5)
    _check_obs_stats(m, z["out_cond"])
    hm = harness.eval_loss_metrics(ag, batch, 3)
    assert sorted(hm) == ["full_action_mse", "loss", "obs_max", "obs_mean", "obs_min", "obs_std"]
    assert all(np.isfinite(v) for v in hm.values())
    pred = np.array(ag.sample(batch, 3)[0])
    assert hm["full_action_mse"] == pytest.approx(float(np.mean(np.square(z["in_actions"][:, :AH] - pred))), rel=1e-6)
    with pytest.raises(NotImplementedError, match="backward pass"):
        ag.update(batch, 0, 0)
