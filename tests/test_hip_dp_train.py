"""DPTrainAgent on the GPU: the U-Net tape's gradient of the condition, the joint update of the encoders and the U-Net against the float64
goldens of tests/golden/make_golden_dp_train.py, the Philox draw, and sampling / snapshots after training.

Error rule, per entry: |got - ref64| <= max(1e-4 * leafmax64, 3 * err32_leaf) + 1e-12 (err32 stored by the generator);
digests under the rule of tests/test_hip_dp_vae.py's _assert_digest, on the stored prefix of the sampled entries."""
import functools

import numpy as np
import pytest
import torch

from latent_diffusion_planning_amd import weights as W
from tests import dp_resnet_oracle as RO
from tests import dp_train_oracle as TO
from tests.golden.make_golden_dp_train import AH, CASES, DIGEST_SAMPLES, N_UPDATE, OH, SEED_E, SEED_G, SEED_P, T, golden_path, kwargs
from tests.util import tree_digest

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _agent(cfg="rm_img", shared=False):
    """One agent (one engine handle) per configuration for the whole module."""
    from latent_diffusion_planning_amd.dp_train_agent import DPTrainAgent
    return DPTrainAgent.create(0, None, RO.BY_NAME[cfg]["shape_meta"], **kwargs(cfg, shared))


def _with_params(ag, p, enc):
    return ag.replace(planner_state=ag.planner_state.replace(params=p, ema_params=p),
                      encoder_state_dict={k: ag.encoder_state_dict[k].replace(params=enc[k], ema_params=enc[k]) for k in enc})


@functools.lru_cache(maxsize=None)
def _golden(name):
    cfg, shared, _, _ = CASES[name]
    z = np.load(golden_path(name))
    data = RO.BY_NAME[cfg]
    p = RO.planner_params(data, int(z["seed_params"]), OH)
    enc = RO.encoder_params(data, int(z["seed_encoder"]), shared)
    obs = {k[len("in_obs__"):]: z[k] for k in z.files if k.startswith("in_obs__")}
    batch = {"obs": obs, "actions": z["in_actions"]}
    return z, data, p, enc, batch, dict(t=z["in_t"].astype(np.int64), noise=z["in_noise"])


def _fresh(name):
    cfg, shared, _, _ = CASES[name]
    z, data, p, enc, batch, noise = _golden(name)
    return _with_params(_agent(cfg, shared), p, enc)


def _digest(tree, seed):
    return tree_digest(tree, seed)[:, :3 + DIGEST_SAMPLES]


def _assert_digest(got_tree, want, seed, tol, what):
    got = _digest(got_tree, seed)
    rel = np.abs(got[:, :3] - want[:, :3]) / np.maximum(np.abs(want[:, :3]), 1e-30)
    assert float(rel.max()) < 1e-4, f"{what}: digest statistics off by {float(rel.max()):.3e} relative"
    err = float(np.abs(got[:, 3:] - want[:, 3:]).max())
    assert err < tol, f"{what}: max |diff| {err:.3e}"


def _assert_grad_digest(tree, want, err32, what):
    got = _digest(tree, SEED_G)
    worst, where = 0.0, None
    for j, k in enumerate(tree):                           # sampled entries within the rule of their leaf
        bound = max(1e-4 * want[j, 1], 3.0 * err32[j]) + 1e-12
        r = float(np.abs(got[j, 3:] - want[j, 3:]).max()) / bound
        if r > worst:
            worst, where = r, k
    print(f"{what}: worst error / bound = {worst:.3f} on {where}")
    assert worst <= 1.0, f"{what}: error / bound = {worst:.3f} on {where}"


def _check_obs_stats(m, cond64):
    for s, v in RO.stats(cond64).items():
        assert abs(float(m[f"obs_{s}"]) - v) < 1e-4, (s, float(m[f"obs_{s}"]), v)


def _states(ag):
    return [("planner", "planner", ag.planner_state, W.planner_shapes(ag._planner_spec))] + \
           [(k, f"encoder{i}", ag.encoder_state_dict[k], W.resnet_shapes()) for i, k in enumerate(ag._encoder_keys())]


# ---- the U-Net tape with the gradient of the condition ------------------------------------------------------------------------------------
def test_planner_grad_cond_is_planner_grad_plus_dcond():
    name = "dp_train_update_rm_img_b3"
    z, data, p, enc, batch, noise = _golden(name)
    ag = _fresh(name)
    eng = ag._engine
    ag._train_sync("planner", ag.planner_state, W.planner_shapes(ag._planner_spec), decay=ag.planner_ema_decay)
    a = torch.tensor(TO.np64.apply_norm(np.asarray(z["in_actions"], np.float32), data["obs_normalization"]["actions"], True).astype(np.float32),
                     device="cuda")
    cond = torch.tensor(z["out_cond"], device="cuda")
    assert cond.shape == (3, 2066)                          # the tape has never run at this width
    eps = torch.tensor(noise["noise"], device="cuda")
    l0 = eng.train_planner_grad(a, eps, noise["t"], cond)
    g0 = eng.train_arena("planner", eng.TRAIN_GRADS).clone()
    eng.train_arena("planner", eng.TRAIN_GRADS).zero_()
    l1, dcond = eng.train_planner_grad_cond(a, eps, noise["t"], cond)
    assert torch.equal(l0, l1) and torch.equal(eng.train_arena("planner", eng.TRAIN_GRADS), g0)
    ref = z["out_dcond"].astype(np.float64)
    bound = max(1e-4 * np.abs(ref).max(), 3.0 * float(z["out_err32_dcond"])) + 1e-12
    err = float(np.abs(dcond.cpu().numpy() - ref).max())
    print(f"dcond: err {err:.3e}, bound {bound:.3e} (leafmax {np.abs(ref).max():.3e}, err32 {float(z['out_err32_dcond']):.3e})")
    assert err <= bound
    np.testing.assert_allclose(float(l1), float(z["out_loss"]), rtol=1e-5)


# ---- the three goldens --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_update_matches_golden(name):
    z, data, p, enc, batch, noise = _golden(name)
    ag = _fresh(name)
    eng = ag._engine
    keys = ag._encoder_keys()
    names = ["planner"] + [f"enc_{k}" for k in keys]
    lr0 = float(z["out_lr"][0, 0])
    for i in range(N_UPDATE):
        before = {k: {q: np.array(v) for q, v in st.params.items()} for k, _, st, _ in _states(ag)} if i == 0 else None
        ag, m = ag.update(batch, 0, i, noise=noise)
        assert sorted(m) == sorted(["loss", "obs_min", "obs_max", "obs_mean", "obs_std"] + [f"{n}_{s}" for n in names for s in ("lr", "step")])
        for j, n in enumerate(names):
            assert m[f"{n}_step"] == int(z["out_steps"][i, j]) == i
            assert abs(float(m[f"{n}_lr"]) - z["out_lr"][i, j]) <= 1e-6 * z["out_lr"][i, j]
        if i == 0:
            print(f"{name}: loss {float(m['loss']):.8f} golden {float(z['out_loss']):.8f}")
            np.testing.assert_allclose(float(m["loss"]), float(z["out_loss"]), rtol=1e-5)
            _check_obs_stats(m, z["out_cond"])
            for k, mod, st, shapes in _states(ag):
                g = eng.train_read(mod, eng.TRAIN_GRADS, shapes)
                _assert_grad_digest(g, z[f"out_gdig_{k}"], z[f"out_err32_{k}"], f"{name} gradients of {k}")
        if i + 1 in (1, N_UPDATE):
            for k, mod, st, shapes in _states(ag):
                _assert_digest(st.params, z[f"out_pdig{i + 1}_{k}"], SEED_P, 1e-5, f"{name} {k} params after {i + 1}")
                _assert_digest(st.ema_params, z[f"out_edig{i + 1}_{k}"], SEED_E, 1e-5, f"{name} {k} EMA after {i + 1}")
                if i == 0:                                  # Adam's first step is ~lr per entry: every leaf has moved
                    for q, v in st.params.items():
                        assert np.abs(v.astype(np.float64) - before[k][q]).max() >= 0.9 * lr0, (k, q)
    assert all(st.step == N_UPDATE for _, _, st, _ in _states(ag))


def test_shared_encoder_gradient_is_the_sum_over_both_cameras():
    """The shared encoder sees the cameras concatenated on the time axis: its gradient is the sum of the gradients of each camera's frames
    with the other camera's feature gradient set to zero (the VJP is linear in dfeat)."""
    name = "dp_train_update_rm_img2_shared_b2"
    z, data, p, enc, batch, noise = _golden(name)
    ag = _fresh(name)
    eng = ag._engine
    ag.update(batch, 0, 0, noise=noise)
    shapes = W.resnet_shapes()
    full = eng.train_read("encoder0", eng.TRAIN_GRADS, shapes)
    nb = ag._postprocess(batch)
    frames = ag._encoder_frames(nb["obs"])[0]
    B, ncam = 2, 2
    ag._train_sync("encoder0", ag.encoder_state_dict["shared"], shapes, decay=ag.encoder_ema_decay)
    dcond = torch.tensor(z["out_dcond"], device="cuda")
    dfeat = dcond[:, :ncam * OH * 1024].reshape(B, ncam, OH, 1024)
    parts = []
    for cam in range(ncam):
        d = torch.zeros_like(dfeat)
        d[:, cam] = dfeat[:, cam]
        eng.train_encoder_forward(0, frames)
        eng.train_encoder_backward(0, d.reshape(-1, 1024))
        parts.append(eng.train_read("encoder0", eng.TRAIN_GRADS, shapes))
    for k in shapes:
        s = parts[0][k].astype(np.float64) + parts[1][k]
        assert np.abs(s - full[k]).max() <= 1e-4 * np.abs(full[k]).max() + 1e-12, k
        assert np.abs(parts[0][k]).max() > 0 and np.abs(parts[1][k]).max() > 0, k


# ---- the Philox draw ----------------------------------------------------------------------------------------------------------------------
def test_noise_none_is_the_philox_draw_passed_explicitly():
    from latent_diffusion_planning_amd.agent import _philox_normal
    name = "dp_train_update_rm_img_b3"
    z, data, p, enc, batch, _ = _golden(name)
    seed, B, A = 12345, 3, 7
    t = np.random.Generator(np.random.PCG64(seed)).integers(0, 100, size=B)
    eps = _philox_normal(seed, 0, 0, 7, B * T * A, torch.device("cuda")).reshape(B, T, A)
    arenas = []
    for nz in (None, dict(t=t, noise=eps)):
        ag = _fresh(name)
        new, m = ag.update(batch, seed, 0, noise=nz)
        arenas.append([ag._engine.train_arena(mod, w).clone() for mod in ("planner", "encoder0") for w in (0, 1, 2, 3, 4)] + [float(m["loss"])])
    for a, b in zip(*arenas):
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b


# ---- sampling after training ------------------------------------------------------------------------------------------------------------
def test_sampling_after_training_and_snapshot_round_trip(tmp_path):
    from latent_diffusion_planning_amd import checkpoint
    from latent_diffusion_planning_amd.dp_agent import DPAgent
    from latent_diffusion_planning_amd.dp_train_agent import DPTrainAgent
    name = "dp_train_update_rm_img2_b2"
    cfg, shared, _, _ = CASES[name]
    z, data, p, enc, batch, noise = _golden(name)
    ag0 = _fresh(name)
    eng = ag0._engine
    obs = {"obs": RO.synth_image_batch(data, 3, OH, 55)["obs"]}
    kw = dict(sampler="ddim", n_steps=10)
    before = np.array(ag0.sample(obs, 4, **kw)[0])
    ag = ag0
    for i in range(2):
        ag, _ = ag.update(batch, 0, i, noise=noise)
    uploads = list(eng.encoder_uploads)
    after = np.array(ag.sample(obs, 4, **kw)[0])
    assert eng.encoder_uploads == uploads, "a trained encoder went through the host"
    assert eng.loaded["encoder1"] == ag.encoder_state_dict["robot0_eye_in_hand_image"].version
    assert not np.array_equal(before, after)
    ag0.update(batch, 0, 0, noise=noise)                       # another step from the old states: ag's arenas are donated to it
    for st in (ag.planner_state, ag.encoder_state_dict["agentview_image"]):
        with pytest.raises(RuntimeError, match="superseded by a later update"):
            st.params
    # the untouched evaluation class on the trained parameters
    ag, _ = _fresh(name).update(batch, 0, 0, noise=noise)
    ag, _ = ag.update(batch, 0, 1, noise=noise)
    params = ag.get_params()
    trained = np.array(ag.sample(obs, 4, **kw)[0])
    assert np.array_equal(trained, after)
    plain = DPAgent.create(0, None, data["shape_meta"], **kwargs(cfg, shared))
    plain = _with_params(plain, params["planner_params"], {k: params["encoder_params"][f"{k}_params"] for k in ag._encoder_keys()})
    assert np.array_equal(np.array(plain.sample(obs, 4, **kw)[0]), trained)
    with pytest.raises(NotImplementedError, match="backward pass"):
        plain.update(batch, 0, 0)
    # snapshot -> a new DPTrainAgent: samples bit-equal, trains on with fresh Adam moments
    path = str(tmp_path / "2.ckpt")
    checkpoint.save_snapshot(ag, path)
    new = checkpoint.load_snapshot(DPTrainAgent.create(1, None, data["shape_meta"], **kwargs(cfg, shared)), path)
    assert isinstance(new, DPTrainAgent) and new.planner_ema_decay == ag.planner_ema_decay
    assert np.array_equal(np.array(new.sample(obs, 4, **kw)[0]), trained)
    new2, m = new.update(batch, 0, 0, noise=noise)
    assert np.isfinite(float(m["loss"])) and new2.planner_state.opt_state["count"] == new.planner_state.step + 1
    mu = new2.encoder_state_dict["agentview_image"].opt_state["mu"]
    g = new._engine.train_read("encoder0", new._engine.TRAIN_GRADS, W.resnet_shapes())
    for k in ("conv_init/kernel", "ResNetBlock_7/MyGroupNorm_1/scale"):
        np.testing.assert_allclose(mu[k], 0.1 * g[k], rtol=1e-5, atol=1e-12)       # mu = (1 - b1) g: the moments started from zero
    for fn in (new.update_mixed, new.sample_viz, new.sample_action_from_plan):
        with pytest.raises(NotImplementedError):
            fn()
