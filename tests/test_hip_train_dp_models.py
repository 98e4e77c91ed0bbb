"""Data-parallel training of the StableVAE and of DPTrainAgent on real hardware: dist.update_sharded with the real classes, structured as
tests/test_hip_train_dp.py -- two ranks share cuda:0 over backend gloo on a one-GPU box, one rank per GPU over "nccl" (RCCL) with two.

Bounds (those of tests/test_hip_train_dp.py): gradient digests within 1e-4 of the leaf's maximum, parameter / EMA digests within 1e-5 of
the one-process update of the whole batch, losses within 2e-5 max(1, |loss|), the two replicas bitwise equal.  The VAE's eleven metrics are
the same kernels' results on the same frames, cut differently: each part's value carries one float32 rounding (6e-8 relative), the merge
runs in float64 and rounds once more; a different summation order inside a frame moves a value by a few 1e-7 at most.  Bound: 1e-6
max(1, |one-process value|), the absolute bound tests/test_hip_vae_train.py's _check_metrics gives the image statistics."""
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KEY, KEY2 = "agentview_image", "robot0_eye_in_hand_image"
VAE_ROWS, DP_ROWS, STEPS = 3, 5, 2


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _init(rank, world, port, backend):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = rank if backend == "nccl" else 0
    torch.cuda.set_device(dev)
    kw = dict(device_id=torch.device("cuda", dev)) if backend == "nccl" else {}
    dist.init_process_group(backend, rank=rank, world_size=world, **kw)


def _two_ranks(worker, *args):
    import torch.multiprocessing as mp
    world = 2
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=worker, args=(r, world, port, backend, q) + args) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=900) for _ in range(world)), key=lambda x: x[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return res


def _grad_err(out, ref):
    return float((np.abs(out - ref) / np.maximum(ref[:, 1:2], 1e-30))[:, 3:].max())


# ---- the StableVAE: 3 rows x 2 cameras, shards 2 + 1, each camera's rows a run of its own -------------------------------------------------
def _vae_model():
    from latent_diffusion_planning_amd import weights as W
    from latent_diffusion_planning_amd.vae_model import StableVAEModel
    from tests import vae_train_oracle as VT
    m = StableVAEModel.create(0, None, dict(all_shapes={KEY: [64, 64, 3], KEY2: [64, 64, 3]}), name="stable_vae_model",
                              vae=dict(latent_channels=4), rgb_obs=[KEY, KEY2],
                              obs_normalization={"obs": {KEY: dict(min=0, max=255), KEY2: dict(min=0, max=255)}}, lr=VT.LR, end_lr=VT.END_LR,
                              warmup_steps=VT.WARMUP, decay_steps=300000, ema_decay=VT.EMA_DECAY, use_kl=True, beta=VT.BETA, data_name="rm_lift")
    p = W.init_vae_params(seed=5)
    return m.replace(vae_state=m.vae_state.replace(params=p, ema_params=p))


def _vae_batch(step):
    from tests.golden.make_golden_vae_update import raw_frames
    return {"obs": {KEY: raw_frames(7000 + step, VAE_ROWS), KEY2: raw_frames(7100 + step, VAE_ROWS)}}


def _vae_run(model, step_fn):
    from latent_diffusion_planning_amd import _lib, weights as W
    from tests.util import tree_digest
    out = dict(metrics=[])
    for s in range(STEPS):
        model, m = step_fn(model, _vae_batch(s), 40 + s, s)
        out["metrics"].append([float(m[k]) for k in _lib.VAE_METRIC_KEYS] + [float(m["vae_lr"]), float(m["vae_step"])])
        if s == 0:
            e = model._engine
            out["grads"] = tree_digest(e.train_read("vae", e.TRAIN_GRADS, W.vae_shapes(model._vae_spec)), 41)
    out["params"], out["ema"] = tree_digest(model.vae_state.params, 42), tree_digest(model.vae_state.ema_params, 43)
    out["step"] = model.vae_state.step
    return model, out


def _vae_worker(rank, world, port, backend, q):
    import torch.distributed as dist
    from latent_diffusion_planning_amd.dist import update_sharded
    _init(rank, world, port, backend)
    try:
        model, out = _vae_run(_vae_model(), lambda m, b, rng, s: update_sharded(m, b, rng, s))
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_two_ranks_train_the_vae_like_one():
    res = _two_ranks(_vae_worker)
    model, ref = _vae_run(_vae_model(), lambda m, b, rng, s: m.update(b, rng, s))
    for rank, out in res:
        assert out["step"] == ref["step"] == STEPS
        for s, (m, r) in enumerate(zip(out["metrics"], ref["metrics"])):
            for k, (a, b) in enumerate(zip(m, r)):
                assert abs(a - b) <= 1e-6 * max(1.0, abs(b)), (rank, s, k, a, b)
        err = _grad_err(out["grads"], ref["grads"])
        print(f"vae rank {rank}: worst gradient digest entry off by {err:.2e} of its leaf's max")
        assert err <= 1e-4, (rank, err)
        for k in ("params", "ema"):
            assert np.abs(out[k][:, 3:] - ref[k][:, 3:]).max() <= 1e-5, (rank, k)
    for k in ("grads", "params", "ema", "metrics"):                 # the replicas never diverge, and every rank reports the GLOBAL metrics
        assert np.array_equal(np.asarray(res[0][1][k]), np.asarray(res[1][1][k])), k
    model._engine.close()


# ---- DPTrainAgent: 5 rows, shards 3 + 2 -------------------------------------------------------------------------------------------------------
def _dp_agent():
    from latent_diffusion_planning_amd.dp_train_agent import DPTrainAgent
    from tests import dp_resnet_oracle as RO
    from tests.golden.make_golden_dp_train import OH, kwargs
    data = RO.BY_NAME["rm_img"]
    ag = DPTrainAgent.create(0, None, data["shape_meta"], **kwargs("rm_img", False))
    p, enc = RO.planner_params(data, 61, OH), RO.encoder_params(data, 62, False)
    return ag.replace(planner_state=ag.planner_state.replace(params=p, ema_params=p),
                      encoder_state_dict={k: ag.encoder_state_dict[k].replace(params=enc[k], ema_params=enc[k]) for k in enc}), data


def _dp_run(ag, data, step_fn):
    from latent_diffusion_planning_amd import weights as W
    from tests import dp_resnet_oracle as RO
    from tests.golden.make_golden_dp_train import OH, T
    from tests.util import tree_digest
    out = dict(loss=[])
    for s in range(STEPS):
        batch = RO.synth_image_batch(data, DP_ROWS, OH, 900 + s, with_actions=True, T=T)
        ag, m = step_fn(ag, batch, 70 + s, s)
        out["loss"].append(float(m["loss"]))
        if s == 0:
            e = ag._engine
            out["grads_planner"] = tree_digest(e.train_read("planner", e.TRAIN_GRADS, W.planner_shapes(ag._planner_spec)), 51)
            out["grads_encoder"] = tree_digest(e.train_read("encoder0", e.TRAIN_GRADS, W.resnet_shapes()), 52)
    enc = ag.encoder_state_dict[ag._encoder_keys()[0]]
    out["planner"], out["encoder"] = tree_digest(ag.planner_state.params, 53), tree_digest(enc.params, 54)
    out["planner_ema"], out["encoder_ema"] = tree_digest(ag.planner_state.ema_params, 55), tree_digest(enc.ema_params, 56)
    out["steps"] = (ag.planner_state.step, enc.step)
    return ag, out


def _dp_worker(rank, world, port, backend, q):
    import torch.distributed as dist
    from latent_diffusion_planning_amd.dist import update_sharded
    _init(rank, world, port, backend)
    try:
        ag, data = _dp_agent()
        ag, out = _dp_run(ag, data, lambda a, b, rng, s: update_sharded(a, b, rng, s))
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_two_ranks_train_the_image_policy_like_one():
    res = _two_ranks(_dp_worker)
    ag, data = _dp_agent()
    ag, ref = _dp_run(ag, data, lambda a, b, rng, s: a.update(b, rng, s))
    for rank, out in res:
        assert out["steps"] == ref["steps"] == (STEPS, STEPS)
        for s, (a, b) in enumerate(zip(out["loss"], ref["loss"])):
            assert abs(a - b) <= 2e-5 * max(1.0, abs(b)), (rank, s, a, b)
        for k in ("grads_planner", "grads_encoder"):
            err = _grad_err(out[k], ref[k])
            print(f"dp rank {rank}: {k}: worst digest entry off by {err:.2e} of its leaf's max")
            assert err <= 1e-4, (rank, k, err)
        for k in ("planner", "encoder", "planner_ema", "encoder_ema"):
            assert np.abs(out[k][:, 3:] - ref[k][:, 3:]).max() <= 1e-5, (rank, k)
    for k in ("loss", "grads_planner", "grads_encoder", "planner", "encoder", "planner_ema", "encoder_ema"):
        assert np.array_equal(np.asarray(res[0][1][k]), np.asarray(res[1][1][k])), k
    ag._engine.close()
