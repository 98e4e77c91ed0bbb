"""Chunked and data-parallel training steps without a GPU: the rule that cuts a StableVAE step into ldp_train_vae_grad_part calls, the slicing
of explicit noise, merge_vae_metrics against numpy, and DPTrainAgent._update_step under a shard -- on the recording stub engine."""
import numpy as np
import pytest
import torch

from latent_diffusion_planning_amd import _lib, weights as W
from latent_diffusion_planning_amd.dp_vae_agent import DPState
from latent_diffusion_planning_amd.schedule import warmup_cosine_decay_schedule
from latent_diffusion_planning_amd.vae_model import StableVAEModel
from tests.train_stub import TrainStub
from tests.util import rng

KEY, KEY2 = "agentview_image", "robot0_eye_in_hand_image"
NORM = {"obs": {KEY: dict(min=0.0, max=255.0), KEY2: dict(min=0.0, max=255.0)}}


class PartStub(TrainStub):
    """TrainStub plus train_vae_grad_part: the call is recorded with the frames and the noise it was given; the metrics it returns are
    those of a constant image whose value is the part's first global index."""

    def train_vae_grad_part(self, img, n_total, accumulate, use_kl=True, beta=1e-5, seed=0, noise=None, row_offset=0):
        self.calls.append(("part", tuple(img.shape), int(n_total), int(accumulate), use_kl, beta, seed, int(row_offset), img, noise))
        return torch.full((11,), float(row_offset))


def _model(rgb_obs=(KEY,), use_kl=True, monkeypatch=None):
    from latent_diffusion_planning_amd import vae_model
    monkeypatch.setattr(vae_model.W, "check_params", lambda tree, shapes: None)
    cfg = dict(rgb_obs=list(rgb_obs), name="stable_vae_model", use_kl=use_kl, beta=1e-5, n_downsample=6, data_name="rm_lift")
    sched = warmup_cosine_decay_schedule(1e-6, 1e-4, 1000, 300000, 1e-6)
    p = {"quant_conv/bias": np.zeros(8, np.float32)}
    return StableVAEModel(DPState(p, None, ema_is_params=True), NORM, cfg, PartStub(), W.VAESpec(), 64, "cpu", lr_schedule=sched, ema_decay=0.99)


def _raw(seed, B):
    """(B, 1, 64, 64, 3) frames; the first two values of frame b hold b % 256 and b // 256, so a part's frames can be told from the tensor
    it was given."""
    x = rng(seed).integers(0, 256, (B, 1, 64, 64, 3)).astype(np.float32)
    x[:, 0, 0, 0, 0], x[:, 0, 0, 0, 1] = np.arange(B) % 256, np.arange(B) // 256
    return x


def _parts(model):
    return [c[1:8] for c in model._engine.of("part")]


# ---- the part rule ---------------------------------------------------------------------------------------------------------------------------
def test_600_frames_of_one_camera_are_three_parts(monkeypatch):
    m = _model(monkeypatch=monkeypatch)
    new, met = m.update({"obs": {KEY: _raw(1, 600)}}, 7, 0)
    assert _parts(m) == [((256, 64, 64, 3), 600, 0, True, 1e-5, 7, 0), ((256, 64, 64, 3), 600, 1, True, 1e-5, 7, 256),
                         ((88, 64, 64, 3), 600, 1, True, 1e-5, 7, 512)]
    kinds = m._engine.kinds()
    assert kinds == ["load", "ema", "part", "part", "part", "apply"] and m._engine.of("grad") == []
    assert new.vae_state.step == 1 and list(met) == list(_lib.VAE_METRIC_KEYS) + ["vae_lr", "vae_step"]
    # the stub's metrics are the parts' first indices 0 / 256 / 512: the merged means are weighted by frames
    want = (256 * 0 + 256 * 256 + 88 * 512) / 600
    assert abs(float(met["img_mean"]) - want) <= 1e-4 and float(met["img_min"]) == 0.0 and float(met["img_max"]) == 512.0
    # the parts hold the frames in order
    first = [int(round((float(c[8][0, 0, 0, 0]) + 1) / 2 * 255)) + 256 * int(round((float(c[8][0, 0, 0, 1]) + 1) / 2 * 255)) for c in m._engine.of("part")]
    assert first == [0, 256, 512]


def test_a_chunk_crosses_the_camera_boundary(monkeypatch):
    m = _model((KEY, KEY2), monkeypatch=monkeypatch)
    a, b = _raw(2, 10), _raw(3, 10)
    m.update({"obs": {KEY: a, KEY2: b}}, 5, 0, chunk=8, row_offset=100)
    assert [(c[0][0], c[1], c[2], c[6]) for c in _parts(m)] == [(8, 20, 0, 100), (8, 20, 1, 108), (4, 20, 1, 116)]
    second = m._engine.of("part")[1][8].numpy()                      # frames 8, 9 of the first camera, then 0 .. 5 of the second
    np.testing.assert_allclose(second[:2], a[8:, 0] / 255 * 2 - 1, atol=1e-6)
    np.testing.assert_allclose(second[2:], b[:6, 0] / 255 * 2 - 1, atol=1e-6)


@pytest.mark.parametrize("frames,cams", [(256, 1), (128, 2), (2, 1)])
def test_up_to_256_frames_unchunked_are_the_one_legacy_call(frames, cams, monkeypatch):
    m = _model((KEY, KEY2)[:cams], monkeypatch=monkeypatch)
    m.update({"obs": {k: _raw(4 + i, frames) for i, k in enumerate((KEY, KEY2)[:cams])}}, 3, 0, row_offset=11)
    assert m._engine.of("part") == []
    assert m._engine.of("grad") == [("grad", (frames * cams, 64, 64, 3), True, 1e-5, 3, 11)]
    assert m._engine.kinds() == ["load", "ema", "grad", "apply"]


def test_sharded_rows_are_one_part_per_camera(monkeypatch):
    m = _model((KEY, KEY2), monkeypatch=monkeypatch)
    lo, n, B = 3, 7, 2                                                # this rank holds rows 3, 4 of 7
    _in_one_process_group(monkeypatch, lambda: m._update_step({"obs": {KEY: _raw(5, B), KEY2: _raw(6, B)}}, None, 9, True, False, None,
                                                             shard=dict(group=None, rows=(lo, n))))
    assert [(c[0][0], c[1], c[2], c[6]) for c in _parts(m)] == [(B, 2 * n, 0, 0 * n + lo), (B, 2 * n, 1, 1 * n + lo)]
    kinds = m._engine.kinds()
    assert kinds == ["load", "ema", "part", "part", "arena", "apply"]  # ONE all-reduce of the gradient arena, between the last part and Adam
    assert m._engine.of("arena") == [("arena", "vae", TrainStub.TRAIN_GRADS)]
    assert m._gates(0) == (True, False)


def _in_one_process_group(monkeypatch, fn, tmp=None):
    """fn() inside a one-process gloo group on a file store (its collectives are the identity)."""
    import tempfile
    import torch.distributed as dist
    with tempfile.TemporaryDirectory() as d:
        dist.init_process_group("gloo", init_method=f"file://{d}/store", rank=0, world_size=1)
        try:
            return fn()
        finally:
            dist.destroy_process_group()


# ---- explicit noise ------------------------------------------------------------------------------------------------------------------------
def test_explicit_noise_global_and_local_forms_are_sliced_by_part(monkeypatch):
    lo, n, B = 3, 7, 2
    glob = rng(8).standard_normal((2 * n, 2, 2, 4)).astype(np.float32)
    local = np.concatenate([glob[lo:lo + B], glob[n + lo:n + lo + B]])
    batch = {"obs": {KEY: _raw(5, B), KEY2: _raw(6, B)}}
    for noise in (glob, local):
        m = _model((KEY, KEY2), monkeypatch=monkeypatch)
        _in_one_process_group(monkeypatch, lambda: m._update_step(batch, None, 9, True, False, noise, shard=dict(group=None, rows=(lo, n))))
        got = [c[9].numpy() for c in m._engine.of("part")]
        np.testing.assert_array_equal(got[0], glob[lo:lo + B])
        np.testing.assert_array_equal(got[1], glob[n + lo:n + lo + B])
    # unsharded and chunked: global index minus row_offset
    m = _model((KEY, KEY2), monkeypatch=monkeypatch)
    eps = rng(9).standard_normal((20, 2, 2, 4)).astype(np.float32)
    m.update({"obs": {KEY: _raw(2, 10), KEY2: _raw(3, 10)}}, 5, 0, noise=eps, chunk=8, row_offset=100)
    got = [c[9].numpy() for c in m._engine.of("part")]
    assert [len(g) for g in got] == [8, 8, 4]
    np.testing.assert_array_equal(np.concatenate(got), eps)
    with pytest.raises(ValueError, match="noise holds 5 frames"):
        _model(monkeypatch=monkeypatch).update({"obs": {KEY: _raw(1, 4)}}, 0, 0, noise=eps[:5], chunk=2)


@pytest.mark.parametrize("chunk", [0, 257, -1])
def test_chunk_outside_1_to_256_is_refused(chunk, monkeypatch):
    m = _model(monkeypatch=monkeypatch)
    with pytest.raises(ValueError, match="1 to 256"):
        m.update({"obs": {KEY: _raw(1, 4)}}, 0, 0, chunk=chunk)
    assert m._engine.calls == []


# ---- merge_vae_metrics ---------------------------------------------------------------------------------------------------------------------
def _eleven(img, z, mse, kl, use_kl, beta):
    """The eleven quantities of a set of frames: img / z (frames, values per frame), mse / kl one value per frame."""
    return np.array([img.min(), img.max(), img.mean(), img.std(), mse.mean() + beta * kl.mean() if use_kl else mse.mean(), mse.mean(),
                     kl.mean() if use_kl else 0.0, z.min(), z.max(), z.mean(), z.std()])


@pytest.mark.parametrize("use_kl", [True, False])
def test_merge_vae_metrics_equals_the_metrics_of_the_whole_array(use_kl):
    from latent_diffusion_planning_amd.vae_model import merge_vae_metrics
    g = rng(41)
    F, beta = 23, 0.37
    img, z = g.uniform(-1, 1, (F, 50)) + g.uniform(-0.5, 0.5, (F, 1)), g.standard_normal((F, 16)) * g.uniform(0.5, 2, (F, 1)) + 0.3
    mse, kl = g.uniform(0, 1, F), g.uniform(0, 3, F)
    cuts = [(0, 9), (9, 10), (10, 23)]                                # three ragged parts, one of a single frame
    vecs = [torch.tensor(_eleven(img[a:b], z[a:b], mse[a:b], kl[a:b], use_kl, beta), dtype=torch.float64) for a, b in cuts]
    whole = _eleven(img, z, mse, kl, use_kl, beta)
    for counts in ([b - a for a, b in cuts], torch.tensor([float(b - a) for a, b in cuts])):     # ints, or the gathered tensor
        got = merge_vae_metrics(vecs, counts, use_kl, beta)
        assert got.dtype == torch.float32 and got.shape == (11,)
        assert float(np.abs(whole).max()) < 8.0                       # (the float32 result rounds by at most 2.4e-7 below 8)
        np.testing.assert_allclose(got.numpy(), whole, rtol=0, atol=1e-6)
    # weighting matters: equal weights are not the answer
    wrong = merge_vae_metrics(vecs, [1, 1, 1], use_kl, beta).numpy()
    assert abs(wrong[2] - whole[2]) > 1e-4


# ---- DPTrainAgent under a shard ------------------------------------------------------------------------------------------------------------
def _dp_calls(eng):
    return [c for c in eng.calls if c[0] != "stats"]


@pytest.fixture
def philox_calls(monkeypatch):
    """The device Philox draw of DPTrainAgent (stream 7) replaced by a recorder: -> the list of (seed, first element, step, stream, count)."""
    from latent_diffusion_planning_amd import dp_train_agent
    seen = []

    def fake(seed, elem0, step, stream, n, device):
        seen.append((seed, elem0, step, stream, n))
        return torch.arange(n, dtype=torch.float32) + elem0
    monkeypatch.setattr(dp_train_agent, "_philox_normal", fake)
    return seen


def test_dp_train_agent_update_step_with_a_shard(monkeypatch, philox_calls):
    from tests.test_dp_train_cpu import _batch, _stub_agent
    lo, n, B = 3, 5, 2
    ag, data = _stub_agent("rm_img2")
    full, _ = _batch(data, n, 7)
    local = {"obs": {k: v[lo:lo + B] for k, v in full["obs"].items()}, "actions": full["actions"][lo:lo + B]}
    seed = 13
    new, m = _in_one_process_group(monkeypatch, lambda: ag._update_step(local, None, seed, True, False, None, shard=dict(group=None, rows=(lo, n))))
    eng = ag._engine
    call = eng.of("planner_grad_cond")[0]
    t_glob = np.random.Generator(np.random.PCG64(seed)).integers(0, 100, size=n)
    np.testing.assert_array_equal(call[3], t_glob[lo:lo + B])        # the global rows' timesteps, sliced
    assert call[5] == float(np.float32(B) / np.float32(n))           # alpha = B_local / n
    assert call[1].shape[0] == B and call[2].shape == call[1].shape
    T_, A_ = call[1].shape[1:]
    assert philox_calls == [(seed, lo * T_ * A_, 0, 7, B * T_ * A_)]   # the noise of global rows lo .. lo + B
    kinds = [c[0] for c in _dp_calls(eng)]
    assert kinds == ["load", "ema"] * 3 + ["enc_fwd"] * 2 + ["planner_grad_cond"] + ["enc_bwd"] * 2 + ["arena"] * 3 + ["apply"] * 3
    assert eng.of("arena") == [("arena", mod, TrainStub.TRAIN_GRADS) for mod in ("planner", "encoder0", "encoder1")]
    assert float(m["loss"]) == eng.PLAN_LOSS and new.planner_state.step == 1
    assert ag._gates(5) == (True, False)
    # explicit global noise is sliced to the local rows, explicit local noise is taken as it is
    g = rng(3)
    nz = dict(t=g.integers(0, 100, n), noise=g.standard_normal((n, call[1].shape[1], 7)).astype(np.float32))
    for given in (nz, dict(t=nz["t"][lo:lo + B], noise=nz["noise"][lo:lo + B])):
        ag2, _ = _stub_agent("rm_img2")
        _in_one_process_group(monkeypatch, lambda: ag2._update_step(local, None, seed, True, False, given, shard=dict(group=None, rows=(lo, n))))
        c2 = ag2._engine.of("planner_grad_cond")[0]
        np.testing.assert_array_equal(c2[3], nz["t"][lo:lo + B])
        np.testing.assert_array_equal(c2[2].numpy(), nz["noise"][lo:lo + B])


def test_dp_train_agent_update_is_update_step_without_a_shard(philox_calls):
    from tests.test_dp_train_cpu import _batch, _stub_agent

    def flat(eng):
        out = []
        for c in _dp_calls(eng):
            out.append(tuple(v.numpy().tobytes() if torch.is_tensor(v) else v.tobytes() if isinstance(v, np.ndarray) else v for v in c))
        return out
    runs = []
    for how in ("update", "step"):
        ag, data = _stub_agent("rm_img2")
        batch, _ = _batch(data, 3, 5)
        if how == "update":
            ag.update(batch, 21, 0)
        else:
            ag._update_step(batch, None, 21, True, False, None, shard=None)
        runs.append(flat(ag._engine))
    assert runs[0] == runs[1] and "arena" not in [c[0] for c in runs[0]]
    assert philox_calls[0][1] == 0 and philox_calls[0] == philox_calls[1]
    with pytest.raises(NotImplementedError):
        ag._update_step(batch, batch, 21, True, True, None)
