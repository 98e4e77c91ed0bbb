"""DPVAEAgent on the GPU: sampling against the float64 goldens, the one-call policy sampler against the planner loop, the training step
(gradients, Adam, the fused EMA) against the float64 oracle, use_ema, snapshots and data-parallel training."""
import os
import socket

import numpy as np
import pytest
import torch

from tests import cfgs, dp_oracle
from tests.golden.make_golden_dp import AH, DECAY, N_UPDATE, OH, T, golden_path, step_noise
from tests.util import tree_digest

pytestmark = pytest.mark.gpu


def _agent(cfg="rm", **over):
    from latent_diffusion_planning_amd.dp_vae_agent import DPVAEAgent
    data = cfgs.BY_NAME[cfg]
    return DPVAEAgent.create(0, None, data["shape_meta"], **dp_oracle.dp_kwargs(data, OH, T, AH, **over))


def _with_params(agent, p):
    return agent.replace(planner_state=agent.planner_state.replace(params=p, ema_params=p))


def _obs(z, prefix="in_obs__"):
    return {k[len(prefix):]: z[k] for k in z.files if k.startswith(prefix)}


@pytest.mark.parametrize("name", ["dp_vae_sample_rm_ddpm100_b3", "dp_vae_sample_rm_ddim50_b5", "dp_vae_sample_aloha_ddpm100_b2",
                                  "dp_vae_sample_aloha_ddim50_b3"])
def test_sample_matches_golden(name):
    z = np.load(golden_path(name))
    cfg = "aloha" if "aloha" in name else "rm"
    sampler = "ddim" if "ddim" in name else "ddpm"
    n_steps = 50 if "ddim50" in name else 100
    data = cfgs.BY_NAME[cfg]
    ag = _with_params(_agent(cfg), dp_oracle.params(data, int(z["seed_params"]), OH))
    B, A = z["in_x_init"].shape[0], data["shape_meta"]["ac_dim"]
    noise = dict(x_init=z["in_x_init"])
    if sampler == "ddpm":
        noise["x_noise"] = step_noise(int(z["seed_noise"]), n_steps, B, A)
    act, extra = ag.sample({"obs": _obs(z)}, 0, noise=noise, sampler=sampler, n_steps=n_steps)
    got = np.array(act)
    assert extra == {} and got.shape == (B, AH, A)
    err = float(np.abs(got - z["out_action"]).max())
    assert err < 1e-4, f"{name}: max |diff| {err:.3e}"


def _frame_emb(ag, B, seed):
    data_batch = cfgs.synth_latent_batch(cfgs.BY_NAME["rm"], B, OH, seed)
    nb = ag._postprocess(data_batch)
    return ag._frame_emb(nb["obs"])


def test_graph_replay_is_bitwise_eager():
    ag = _agent()
    ag._sync_weights()
    eng = ag._engine
    emb = _frame_emb(ag, 5, 11)
    kw = dict(seed=7, sampler="ddim", n_steps=10)
    eager = eng.policy_sample(emb, OH, 16, use_graph=False, **kw)
    first = eng.policy_sample(emb, OH, 16, use_graph=True, **kw)
    replay = eng.policy_sample(emb, OH, 16, use_graph=True, **kw)
    torch.cuda.synchronize()
    assert torch.equal(eager, first) and torch.equal(first, replay)


def test_policy_sample_equals_plan_sample_on_torch_condition():
    from latent_diffusion_planning_amd.dp_vae_agent import dp_obs_cond
    ag = _agent()
    ag._sync_weights()
    eng = ag._engine
    emb = _frame_emb(ag, 6, 12)
    cond = dp_obs_cond(emb, OH, 16)
    x0 = torch.randn((6, T, 7), generator=torch.Generator().manual_seed(3)).to(emb.device)
    for sampler, n in (("ddpm", 100), ("ddim", 20)):
        x = eng.plan_sample(cond, x_init=x0, sampler=sampler, n_steps=n, seed=5)
        a = eng.policy_sample(emb, OH, 16, x_init=x0, sampler=sampler, n_steps=n, seed=5)
        torch.cuda.synchronize()
        assert torch.equal(a, x[:, :AH]), sampler
    # with the bounds: un-normalised by the existing kernel
    lo, hi = np.full(7, -0.5, np.float32), np.full(7, 2.0, np.float32)
    a = eng.policy_sample(emb, OH, 16, x_init=x0, sampler="ddim", n_steps=20, seed=5, action_bounds=(lo, hi), action_mode=0)
    x = eng.plan_sample(cond, x_init=x0, sampler="ddim", n_steps=20, seed=5)
    ref = eng.normalize_bounds(x[:, :AH].contiguous(), lo, hi, 0)
    torch.cuda.synchronize()
    assert torch.equal(a, ref)


def test_rows_do_not_depend_on_row_offset_sharding():
    ag = _agent()
    ag._sync_weights()
    eng = ag._engine
    emb = _frame_emb(ag, 8, 13)
    full = eng.policy_sample(emb, OH, 16, seed=99, sampler="ddim", n_steps=10)
    a = eng.policy_sample(emb[:3].contiguous(), OH, 16, seed=99, row_offset=0, sampler="ddim", n_steps=10)
    b = eng.policy_sample(emb[3:].contiguous(), OH, 16, seed=99, row_offset=3, sampler="ddim", n_steps=10)
    torch.cuda.synchronize()
    assert torch.equal(full, torch.cat([a, b]))
    other = eng.policy_sample(emb, OH, 16, seed=98, sampler="ddim", n_steps=10)
    assert not torch.equal(full, other)


def _update_steps(z):
    out = []
    for s in range(N_UPDATE):
        obs = _obs(z, f"in_s{s}_obs__")
        out.append(({"obs": obs, "actions": z[f"in_s{s}_actions"]},
                    dict(t=z[f"in_s{s}_t"].astype(np.int64), noise=z[f"in_s{s}_noise"])))
    return out


def _assert_digest(got_tree, want, seed, tol, what):
    got = tree_digest(got_tree, seed)
    # L2 norm, max |x| and the projection relative; the sampled elements absolute
    rel = np.abs(got[:, :3] - want[:, :3]) / np.maximum(np.abs(want[:, :3]), 1e-30)
    assert float(rel.max()) < 1e-4, f"{what}: digest statistics off by {float(rel.max()):.3e} relative"
    err = float(np.abs(got[:, 3:] - want[:, 3:]).max())
    assert err < tol, f"{what}: max |diff| {err:.3e}"


def test_update_matches_oracle_gradients_adam_and_ema():
    from latent_diffusion_planning_amd import weights as W
    z = np.load(golden_path("dp_vae_update_rm"))
    data = cfgs.BY_NAME["rm"]
    ag = _with_params(_agent(), dp_oracle.params(data, int(z["seed_params"]), OH))
    shapes = W.planner_shapes(ag._planner_spec)
    steps = _update_steps(z)
    eng = ag._engine
    losses, norms = [], []
    for i, (batch, noise) in enumerate(steps):
        ag, m = ag.update(batch, 0, i, noise=noise)
        losses.append(float(m["loss"]))
        norms.append(float(eng.train_grad_norm(["planner"])))
        assert m["planner_step"] == i and "g_norm" not in m
        assert abs(float(m["planner_lr"]) - z["out_lr"][i]) <= 1e-6 * z["out_lr"][i]
        if i == 0:
            g = eng.train_read("planner", eng.TRAIN_GRADS, shapes)
            want = z["out_grads"]
            got = tree_digest(g, 11)
            for j, k in enumerate(g):               # every leaf within 1e-4 of its largest |gradient|
                assert np.abs(got[j, 3:] - want[j, 3:]).max() <= 1e-4 * want[j, 1] + 1e-12, k
            _assert_digest(ag.planner_state.params, z["out_params_after_1"], 13, 1e-5, "params after 1")
            _assert_digest(ag.planner_state.ema_params, z["out_ema_after_1"], 17, 1e-5, "EMA after 1")
    np.testing.assert_allclose(losses, z["out_loss"], rtol=1e-5)
    np.testing.assert_allclose(norms, z["out_g_norm"], rtol=1e-5)
    _assert_digest(ag.planner_state.params, z["out_params_after_n"], 15, 1e-5, "params after 10")
    _assert_digest(ag.planner_state.ema_params, z["out_ema_after_n"], 19, 1e-5, "EMA after 10")
    assert ag.planner_state.step == N_UPDATE


def test_use_ema_samples_equal_an_agent_whose_params_are_the_ema():
    z = np.load(golden_path("dp_vae_update_rm"))
    ag = _agent()
    for i, (batch, noise) in enumerate(_update_steps(z)[:3]):
        ag, _ = ag.update(batch, 0, i, noise=noise)
    obs = {"obs": cfgs.synth_latent_batch(cfgs.BY_NAME["rm"], 4, OH, 21)["obs"]}
    ema_agent = ag.replace(config=dict(ag.config, use_ema=True))
    a = np.array(ema_agent.sample(obs, 5, sampler="ddim", n_steps=10)[0])           # EMA arena -> sampling slot
    p = np.array(ag.sample(obs, 5, sampler="ddim", n_steps=10)[0])                  # parameters
    ema = ag.planner_state.ema_params
    other = _with_params(_agent(), ema)
    b = np.array(other.sample(obs, 5, sampler="ddim", n_steps=10)[0])
    np.testing.assert_array_equal(a, b)
    assert not np.array_equal(a, p)
    # get_metrics reads the same weights as sample
    m_ema = float(ema_agent.get_metrics(dict(obs, actions=z["in_s0_actions"]), 3)["loss"])
    m_oth = float(other.get_metrics(dict(obs, actions=z["in_s0_actions"]), 3)["loss"])
    assert m_ema == m_oth


def test_snapshot_round_trip_samples_bit_equal_and_reseeds_the_ema(tmp_path):
    from latent_diffusion_planning_amd import checkpoint
    from latent_diffusion_planning_amd import weights as W
    z = np.load(golden_path("dp_vae_update_rm"))
    ag = _agent()
    for i, (batch, noise) in enumerate(_update_steps(z)[:2]):
        ag, _ = ag.update(batch, 0, i, noise=noise)
    params = ag.get_params()
    assert set(params) == {"planner_params", "planner_ema_params"}
    path = checkpoint.save_snapshot(ag, str(tmp_path / "2.ckpt"))
    trees = checkpoint.param_trees(checkpoint.restore(path))
    for k, v in params["planner_params"].items():
        np.testing.assert_array_equal(trees["planner_params"][k], v)
    raw = checkpoint.restore(path)
    assert "planner_ema_params" in raw
    restored = checkpoint.load_snapshot(_agent(), path)
    obs = {"obs": cfgs.synth_latent_batch(cfgs.BY_NAME["rm"], 3, OH, 22)["obs"]}
    a = np.array(ag.sample(obs, 9, sampler="ddim", n_steps=10)[0])
    b = np.array(restored.sample(obs, 9, sampler="ddim", n_steps=10)[0])
    np.testing.assert_array_equal(a, b)
    # the restored state (params = EMA = restored, train_bc.py:230-237) re-seeds the engine's EMA arena from the parameters
    st = restored.planner_state
    shapes = W.planner_shapes(restored._planner_spec)
    restored._train_sync("planner", st, shapes)
    e = restored._engine.train_read("planner", restored._engine.TRAIN_EMA, shapes)
    for k, v in trees["planner_params"].items():
        np.testing.assert_array_equal(e[k], v)
    # ... and so does a restore into an engine whose EMA has moved away from them (ldp_train_init's re-seed)
    batch, noise = _update_steps(z)[2]
    moved, _ = restored.update(batch, 0, 2, noise=noise)
    assert not np.array_equal(moved.planner_state.ema_params["Dense_0/kernel"], trees["planner_params"]["Dense_0/kernel"])
    again = checkpoint.load_snapshot(moved, path)
    again._train_sync("planner", again.planner_state, shapes)
    e = again._engine.train_read("planner", again._engine.TRAIN_EMA, shapes)
    for k, v in trees["planner_params"].items():
        np.testing.assert_array_equal(e[k], v)


# ---- data parallel: dist.update_sharded, two ranks on one GPU (tests/test_hip_train_dp.py's pattern) ------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _dp_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from latent_diffusion_planning_amd import dist as D
        z = np.load(golden_path("dp_vae_update_rm"))
        ag = _agent()
        for i, (batch, noise) in enumerate(_update_steps(z)[:2]):
            ag, m = D.update_sharded(ag, batch, 0, i, noise=noise)
            float(m["loss"])
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **{k: v for k, v in list(ag.planner_state.params.items())[:6]},
                 **{f"ema__{k}": v for k, v in list(ag.planner_state.ema_params.items())[:6]})
    finally:
        dist.destroy_process_group()


def test_update_sharded_two_ranks_matches_one(tmp_path):
    import torch.multiprocessing as mp
    z = np.load(golden_path("dp_vae_update_rm"))
    ag = _agent()
    for i, (batch, noise) in enumerate(_update_steps(z)[:2]):
        ag, _ = ag.update(batch, 0, i, noise=noise)
    one = dict(list(ag.planner_state.params.items())[:6])
    one_e = dict(list(ag.planner_state.ema_params.items())[:6])
    del ag
    mp.start_processes(_dp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    for k in r0.files:
        np.testing.assert_array_equal(r0[k], r1[k])                 # the replicas never diverge
    for k, v in one.items():
        np.testing.assert_allclose(r0[k], v, atol=1e-6, err_msg=k)  # = the one-GPU step of the whole batch, to fp32 round-off
        np.testing.assert_allclose(r0[f"ema__{k}"], one_e[k], atol=1e-6, err_msg=k)
