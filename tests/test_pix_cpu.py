"""The camera of the reach task on the host: the C ABI of libldp_pix.so against its header and binding, the refusals that
need no GPU, known answers of the NumPy restatement (tests/pix_oracle.py) the kernel is held to, the pixel task's agent configuration
through the host-side checks of LDPAgent.create, and harness.run_device_eval on the NumPy pixel environment.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from latent_diffusion_planning_amd import harness
from tests import pix_oracle as P
from tests import toyenv_oracle as O

F32 = np.float32
FAR = np.array([[3.0, 0.0]], F32)                      # a centre outside the square: its channel is empty


def _frame(p, g=(3.0, 0.0)):
    return P.render(np.array([p], F32), np.array([g], F32))[0]


# ---- the library's C ABI ---------------------------------------------------------------------------------------------------------------
def test_pix_header_binding_and_library_list_the_same_symbols():
    """libldp_pix.so is a library of its own: include/ldp_pix.h, _pixlib.SIGNATURES and its dynamic symbol table agree, and neither the
    agent's library nor the task's exports any of it."""
    from latent_diffusion_planning_amd import _envlib, _lib, _pixlib
    syms = _pixlib.header_symbols()
    assert syms == sorted(_pixlib.SIGNATURES) == ["ldp_pix_last_error", "ldp_pix_render"]
    assert not set(syms) & set(_lib.SIGNATURES) and not set(syms) & set(_envlib.SIGNATURES)
    csrc = os.path.join(os.path.dirname(_pixlib.LIB_PATH), "csrc")
    with open(os.path.join(csrc, "Makefile")) as f:
        assert "libldp_pix.so" in f.read()
    with open(os.path.join(csrc, "exports_pix.map")) as f:
        assert "ldp_pix_*" in f.read()

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return sorted(line.split()[-1] for line in out.splitlines() if line.strip())
    if os.path.exists(_pixlib.LIB_PATH):
        assert exported(_pixlib.LIB_PATH) == syms
    for other in (_lib.LIB_PATH, _envlib.LIB_PATH):
        if os.path.exists(other):
            assert not [s for s in exported(other) if s.startswith("ldp_pix_")]


def test_a_missing_pix_library_fails_loudly(monkeypatch, tmp_path):
    from latent_diffusion_planning_amd import _lib, _pixlib
    monkeypatch.setattr(_pixlib, "_lib", None)
    monkeypatch.setattr(_pixlib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.LDPHipUnavailable, match="no other implementation") as e:
        _pixlib.load()
    assert "build()" in str(e.value)


def test_refusals_before_any_hip_call_name_the_argument():
    """M = 0, a null pointer, stride 1 and a misaligned frames pointer are refused before any HIP call: no device is needed (the
    pointers are made-up integers that nothing dereferences)."""
    from latent_diffusion_planning_amd import _lib, _pixlib
    lib = _pixlib.load()                                   # (build() made it; a missing library is an error, not a skip)
    p, g, f = 1 << 20, (1 << 20) + 8, 1 << 24

    def render(pos=p, ps=8, goal=g, gs=8, M=4, frames=f):
        return lib.ldp_pix_render(pos, ps, goal, gs, M, frames, None)
    for call, word in ((lambda: render(M=0), "M must be"), (lambda: render(M=-3), "M must be"), (lambda: render(pos=None), "null pos"),
                       (lambda: render(goal=None), "null goal"), (lambda: render(frames=None), "null frames"),
                       (lambda: render(ps=1), "pos_stride"), (lambda: render(gs=1), "goal_stride"), (lambda: render(gs=0), "goal_stride"),
                       (lambda: render(frames=f + 8), "16-byte aligned")):
        with pytest.raises(_lib.LDPHipError, match=word) as e:
            _pixlib.check(call())
        assert e.value.code == _pixlib.PIX_EINVAL == -1


# ---- known answers of the restatement ------------------------------------------------------------------------------------------------------
def test_pixel_centres_are_exact_and_rows_count_from_the_bottom():
    assert P.CENTRES[0] == F32(-63 / 64) and P.CENTRES[63] == F32(63 / 64) and np.all(np.diff(P.CENTRES.astype(np.float64)) == 2 / 64)
    f = _frame((P.CENTRES[20], P.CENTRES[5]))                                       # x = c_20, y = c_5: column 20 of row 5 (near the bottom)
    assert f[5, 20, 0] == 255 and np.argwhere(f[..., 0] == 255).tolist() == [[5, 20]]


def test_a_centre_on_a_pixel_centre_gives_255_and_a_mirror_symmetric_blob():
    f = _frame((P.CENTRES[31], P.CENTRES[40]))[..., 0]
    assert f[40, 31] == 255 and f.max() == 255
    blob = f[40 - 9:40 + 10, 31 - 9:31 + 10]                                          # radius 8 pixels: inside the 19 x 19 window
    assert blob.sum() == f.sum() and np.array_equal(blob, blob[::-1]) and np.array_equal(blob, blob[:, ::-1]) and np.array_equal(blob, blob.T)
    assert (f > 0).sum() > 150                                                        # about pi * 8^2 = 201 pixels, less the faint rim


def test_centres_outside_the_square_and_nan_give_an_empty_channel():
    assert not _frame((3.0, 0.0))[..., 0].any() and not _frame((-3.0, 0.5))[..., 0].any()
    for bad in ((np.nan, 0.1), (0.1, np.nan), (np.nan, np.nan), (np.inf, 0.0), (0.0, -np.inf)):
        f = _frame(bad, g=(0.5, 0.5))
        assert not f[..., 0].any() and f[..., 1].any(), bad


def test_a_blob_at_the_corner_is_clipped_not_lost():
    f = _frame((1.0, -1.0))[..., 0]
    assert f.any() and (f > 0).sum() < 80                                             # a quarter of the blob
    assert f[0, 63] == f.max() and not f[10:, :].any() and not f[:, :53].any()           # bottom right: row 0, column 63


def test_the_disc_channel_is_constant():
    a, b = _frame((0.3, 0.2), (0.8, -0.4)), _frame((-0.9, 0.9), (np.nan, 0.0))
    assert np.array_equal(a[..., 2], b[..., 2])
    assert a[..., 2].max() == 252 and (a[..., 2] > 0).sum() == 276                    # no pixel centre at the origin; radius 0.3 = 9.6 pixels
    assert np.array_equal(a[..., 2], a[::-1, :, 2]) and np.array_equal(a[..., 2], a[:, ::-1, 2])


def test_the_channels_do_not_depend_on_each_other():
    a, b, c = _frame((0.3, 0.2), (0.8, -0.4)), _frame((0.3, 0.2), (0.1, 0.1)), _frame((-0.5, 0.0), (0.8, -0.4))
    assert np.array_equal(a[..., 0], b[..., 0]) and not np.array_equal(a[..., 1], b[..., 1])
    assert np.array_equal(a[..., 1], c[..., 1]) and not np.array_equal(a[..., 0], c[..., 0])
    same = _frame((0.3, 0.2), (0.3, 0.2))
    assert np.array_equal(same[..., 0], same[..., 1])                                 # p = g: the R blob on the G blob


def test_a_third_of_a_pixel_changes_the_frame():
    a, b = _frame((0.3, 0.2))[..., 0].astype(int), _frame((0.31, 0.2))[..., 0].astype(int)
    d = np.abs(a - b)
    print(f"a 0.01 shift changes {int((d > 0).sum())} bytes by up to {int(d.max())} levels")
    assert (d > 0).sum() > 100 and 4 <= d.max() <= 32


def test_strided_rows_render_like_packed_ones():
    g = np.random.Generator(np.random.PCG64(5))
    state = g.uniform(-1, 1, (5, 8)).astype(F32)
    want = P.render(np.ascontiguousarray(state[:, 0:2]), np.ascontiguousarray(state[:, 2:4]))
    assert np.array_equal(P.render_state(state), want) and want.dtype == np.uint8 and want.shape == (5, 64, 64, 3)


# ---- the agent's configuration, through the host-side checks of LDPAgent.create ----------------------------------------------------------------
def test_pixel_config_passes_the_host_side_checks_of_create(monkeypatch):
    """Everything LDPAgent.create checks before it needs a device: obs_dim 18 (16 latent + 2 pos), the 64 x 64 x 3 frame accepted for
    vae_feature_dim 16, the goal nowhere among the numbers.  With no device visible the call then stops at the device check."""
    import torch
    from latent_diffusion_planning_amd import agent as A
    from latent_diffusion_planning_amd import weights as W
    from latent_diffusion_planning_amd._lib import LDPHipUnavailable
    from latent_diffusion_planning_amd.toyenv import reach2d_pixel_config, reach2d_vae_config
    lo, hi = np.full(16, -3, F32), np.full(16, 4, F32)
    cfg = reach2d_pixel_config(latent_bounds=(lo, hi))
    kw = cfg["agent_kwargs"]
    assert kw["lowdim_obs"] == ["pos"] and kw["rgb_obs"] == ["latent_image"] and kw["vae_feature_dim"] == 16
    assert "goal" not in cfg["shape_meta"]["all_shapes"] and "goal" not in kw["obs_normalization"]["obs"]
    assert cfg["shape_meta"]["all_shapes"]["image"] == [64, 64, 3]
    norm = kw["obs_normalization"]["obs"]
    assert norm["image"] == dict(min=0.0, max=255.0) and norm["pos"] == dict(min=-1.0, max=1.0) and norm["latent_image"]["min"] is lo
    specs = []
    real = W.init_planner_params
    monkeypatch.setattr(W, "init_planner_params", lambda spec, **k: specs.append(spec) or real(spec, **k))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(LDPHipUnavailable, match="no HIP device"):
        A.LDPAgent.create(0, None, cfg["shape_meta"], **kw)
    assert specs and specs[0].input_dim == 18 and specs[0].global_cond_dim == 18
    bad = dict(cfg["shape_meta"], all_shapes=dict(cfg["shape_meta"]["all_shapes"], image=[84, 84, 3]))
    with pytest.raises(NotImplementedError, match="64x64x3"):
        A.LDPAgent.create(0, None, bad, **kw)
    v = reach2d_vae_config()
    assert v["vae_kwargs"]["rgb_obs"] == ["image"] and v["shape_meta"]["all_shapes"]["image"] == [64, 64, 3]
    assert v["vae_kwargs"]["obs_normalization"]["obs"]["image"] == norm["image"]


# ---- run_device_eval on the NumPy pixel environment ----------------------------------------------------------------------------------------
def test_run_device_eval_hands_the_policy_uint8_frames():
    N, ah = 4, 4
    env, seen = P.NumpyReach2DPixelEnv(N), []

    def act(batch, rng, cycle):
        obs = batch["obs"]
        assert set(obs) == {"pos", "image"}
        img = obs["image"]
        assert img.dtype == np.uint8 and img.shape == (N, 1, 64, 64, 3) and obs["pos"].shape == (N, 1, 2) and obs["pos"].dtype == F32
        assert np.array_equal(img[:, 0], P.render_state(env.state))
        seen.append(img[:, 0, :, :, 0].astype(np.int64).sum())
        return np.tile(np.array([1.0, 0.25], F32), (N, ah, 1))
    res = harness.run_device_eval(env, act, 2 * N, seed=3, eval_rng=1)
    assert res["n_calls"] == 2 * O.H // ah and len(seen) == res["n_calls"] and np.all(env.state[:, O.T] == O.H)
    g = env.goal_observation()
    assert g["image"].dtype == np.uint8 and np.array_equal(g["image"][..., 0], g["image"][..., 1]) and np.array_equal(g["pos"][:, 0], env.state[:, 2:4])
