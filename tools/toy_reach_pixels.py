#!/usr/bin/env python3
"""reach2d from pixels: render the expert's demonstrations to camera frames on the GPU, train the StableVAE on them, train
an LDP agent on the VAE's latents, and measure closed-loop success with the goal visible in the frame only:
pixels -> StableVAE -> 16-number latent -> planner -> IDM -> action -> environment, no host round trip inside an episode.

Stages, each a GPU process of its own, to be run under its own time limit and chained:

  timeout -k 10 600 python tools/toy_reach_pixels.py vae --dir build_toy_pix \\
    && timeout -k 10 600 python tools/toy_reach_pixels.py train --dir build_toy_pix \\
    && timeout -k 10 600 python tools/toy_reach_pixels.py eval --dir build_toy_pix --out profiles/toy_reach_pixels_eval.json

`vae` collects --episodes expert episodes as frames, trains the StableVAE for --vae-steps steps at --vae-batch and records, on frames of
held-out episodes, loss_mse and the error of a least-squares linear read-out of the goal's height and of the point from the 16 latent means
(fitted on demonstration frames): the figure that tells a failure of the VAE from a failure of the planner.  `train` encodes the frames
(toyenv.encode_demos) and runs harness.fit with the state task's settings.  `eval` runs the scripted policies (which must reproduce the
state task's figures exactly), `sample` under four samplers, and one BLIND arm whose frames have the G channel zeroed: if the goal reaches
the plan through the pixels, that arm falls towards the straight-line policy.  `render-bench` times ldp_pix_render against a device copy.
A TOY task: the figures say what a 16-number latent of this scene preserves, and nothing about a robot."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from toy_reach import scripted_arm                     # the scripted arms are the state task's, on the same episodes

HELD_OUT_EPISODE0 = 500_000                            # the VAE's held-out frames: episodes no stage trains on or evaluates on
PIXELS_PER_UNIT = 32.0                                 # the square [-1, 1] on 64 pixels
STATE_TASK = dict(expert=1.0, straight=0.158203125)    # profiles/toy_reach_eval.json: the same 1024 episodes, the same scripted policies


def _vae_model(args, params=None):
    from latent_diffusion_planning_amd.toyenv import reach2d_vae_config
    from latent_diffusion_planning_amd.vae_model import StableVAEModel
    cfg = reach2d_vae_config(lr=args.vae_lr, warmup_steps=min(200, max(args.vae_steps // 10, 1)), decay_steps=max(args.vae_steps, 1))
    model = StableVAEModel.create(args.seed, None, cfg["shape_meta"], **cfg["vae_kwargs"])
    if params is not None:
        model = model.replace(vae_state=model.vae_state.replace(params=params, ema_params=params))
    return model


def _readout(z_fit, y_fit, z_test, y_test):
    """Least-squares linear map [z, 1] -> y fitted on the demonstration frames; -> RMS error per target on the held-out ones, in pixels."""
    A = np.concatenate([z_fit, np.ones((len(z_fit), 1))], 1).astype(np.float64)
    w, *_ = np.linalg.lstsq(A, y_fit.astype(np.float64), rcond=None)
    pred = np.concatenate([z_test, np.ones((len(z_test), 1))], 1).astype(np.float64) @ w
    return (np.sqrt(np.mean((pred - y_test) ** 2, axis=0)) * PIXELS_PER_UNIT).tolist()


def _frames_and_truth(n, seed, noise, episode0):
    """-> (pixel dataset, truth (n * 48, 3) = px, py, gy of every row): the same rollout recorded twice, once with the camera."""
    from latent_diffusion_planning_amd.toyenv import collect_demos, collect_pixel_demos
    ds = collect_pixel_demos(n, seed, noise, episode0=episode0)
    st = collect_demos(n, seed, noise, episode0=episode0)
    assert torch.equal(st.tables["pos"], ds.tables["pos"])
    truth = torch.cat([st.tables["pos"], st.tables["goal"][:, 1:2]], dim=1).cpu().numpy()
    return ds, truth


def vae(args):
    from latent_diffusion_planning_amd import harness, weights as W
    from latent_diffusion_planning_amd.toyenv import encode_frames
    os.makedirs(args.dir, exist_ok=True)
    t0 = time.time()
    ds, truth = _frames_and_truth(args.episodes, args.seed, args.noise, 0)
    model = _vae_model(args)
    it = ds.batches(args.vae_batch, seed=args.seed + 1)
    curve = []
    t1 = time.time()
    for step in range(args.vae_steps):
        model, m = model.update(next(it), args.seed + 2 + step, step)
        if (step + 1) % args.log_every == 0:
            curve.append(dict(step=step + 1, loss=float(m["loss"]), loss_mse=float(m["loss_mse"]), loss_kl=float(m["loss_kl"])))
            if (step + 1) % (5 * args.log_every) == 0:
                print(f"vae step {step + 1}: loss {curve[-1]['loss']:.6f} (mse {curve[-1]['loss_mse']:.6f}, kl {curve[-1]['loss_kl']:.3f})  "
                      f"{time.time() - t0:.0f} s", flush=True)
    torch.cuda.synchronize()
    train_s = time.time() - t1
    params = dict(model.get_params()["vae_params"])
    W.save_npz(os.path.join(args.dir, "toy_reach_pixels_vae.npz"), vae_params=params)
    # held-out frames: reconstruction error, and what a linear map can read of the scene from the 16 latent means
    held, truth_held = _frames_and_truth(args.held_out, args.seed, args.noise, HELD_OUT_EPISODE0)
    ev = harness.eval_vae_metrics(model, held.batches(256, seed=args.seed + 3), args.seed + 4, max_batches=11)
    model._sync_weights(use_ema=False)
    n_fit = min(args.readout_fit, ds.total_n_sequences)
    z_fit = encode_frames(ds.tables["image"][:n_fit], model._engine, 256).cpu().numpy()
    z_held = encode_frames(held.tables["image"], model._engine, 256).cpu().numpy()
    rms = _readout(z_fit, truth[:n_fit], z_held, truth_held)
    meta = dict(episodes=args.episodes, demo_seed=args.seed, demo_noise=args.noise, demo_frames=ds.total_n_sequences, vae_steps=args.vae_steps,
                vae_batch=args.vae_batch, vae_lr=args.vae_lr, train_seconds=train_s, ms_per_step=1e3 * train_s / max(args.vae_steps, 1),
                held_out=dict(episodes=args.held_out, episode0=HELD_OUT_EPISODE0, frames=held.total_n_sequences, loss_mse=ev["evaldata/loss_mse"],
                              loss_kl=ev["evaldata/loss_kl"], z_min=ev["evaldata/z_min"], z_max=ev["evaldata/z_max"]),
                readout=dict(fit_frames=n_fit, rms_pixels=dict(px=rms[0], py=rms[1], gy=rms[2]),
                             note="least-squares linear read-out from the 16 latent means, fitted on demonstration frames, RMS on held-out frames"),
                loss_curve=curve)
    with open(os.path.join(args.dir, "toy_reach_pixels_vae.json"), "w") as f:
        json.dump(meta, f)
    print(json.dumps({k: v for k, v in meta.items() if k != "loss_curve"}), flush=True)
    model._engine.close()


def _agent(args, decay_steps, vae_params, bounds=None):
    from latent_diffusion_planning_amd.agent import LDPAgent
    from latent_diffusion_planning_amd.toyenv import reach2d_pixel_config
    cfg = reach2d_pixel_config(latent_bounds=bounds, lr=args.lr, warmup_steps=min(500, max(decay_steps // 10, 1)), decay_steps=decay_steps)
    return LDPAgent.create(args.seed, None, cfg["shape_meta"], vae_params=vae_params, **cfg["agent_kwargs"]), cfg


def train(args):
    from latent_diffusion_planning_amd import harness, weights as W
    from latent_diffusion_planning_amd.toyenv import collect_pixel_demos, encode_demos, with_latent_bounds
    with open(os.path.join(args.dir, "toy_reach_pixels_vae.json")) as f:
        vm = json.load(f)
    vae_params = W.load_npz(os.path.join(args.dir, "toy_reach_pixels_vae.npz"))["vae_params"]
    t0 = time.time()
    pix = collect_pixel_demos(vm["episodes"], vm["demo_seed"], vm["demo_noise"], episode0=0)
    agent, _ = _agent(args, args.steps, vae_params)               # encodes first: its latent map is still the unit map
    ds, (lo, hi) = encode_demos(pix, agent, chunk=256)
    del pix
    torch.cuda.empty_cache()
    encode_s = time.time() - t0
    if np.any(hi - lo < 1e-6):
        raise RuntimeError(f"a latent component is constant over the demonstrations (min {lo}, max {hi}): the VAE has collapsed")
    agent = with_latent_bounds(agent, (lo, hi))
    curve = []

    def on_log(step, m):
        curve.append(dict(step=step, loss=m["loss"], plan_loss=m["plan_loss"], idm_loss=m["idm_loss"], g_norm=m.get("g_norm")))
        if step % (10 * args.log_every) == 0:
            print(f"step {step}: loss {m['loss']:.5f} (plan {m['plan_loss']:.5f}, idm {m['idm_loss']:.5f})  {time.time() - t0:.0f} s", flush=True)
    t1 = time.time()
    agent, _ = harness.fit(agent, ds.batches(args.batch, seed=args.seed + 1), args.steps, args.seed + 2, log_every=args.log_every, on_log=on_log)
    planner, idm = dict(agent.planner_state.params), dict(agent.idm_state.params)
    train_s = time.time() - t1
    W.save_npz(os.path.join(args.dir, "toy_reach_pixels_params.npz"), planner=planner, idm=idm)
    meta = dict(steps=args.steps, batch=args.batch, lr=args.lr, demo_rows=ds.total_n_sequences, encode_seconds=encode_s, train_seconds=train_s,
                ms_per_step=1e3 * train_s / max(args.steps, 1), latent_min=lo.tolist(), latent_max=hi.tolist(), loss_curve=curve)
    with open(os.path.join(args.dir, "toy_reach_pixels_train.json"), "w") as f:
        json.dump(meta, f)
    print(json.dumps({k: v for k, v in meta.items() if k != "loss_curve"}), flush=True)
    agent._engine.close()


def evaluate(args):
    from latent_diffusion_planning_amd import _lib, harness, weights as W
    from latent_diffusion_planning_amd.toyenv import Reach2DPixelEnv
    with open(os.path.join(args.dir, "toy_reach_pixels_vae.json")) as f:
        vm = json.load(f)
    with open(os.path.join(args.dir, "toy_reach_pixels_train.json")) as f:
        tr = json.load(f)
    vae_params = W.load_npz(os.path.join(args.dir, "toy_reach_pixels_vae.npz"))["vae_params"]
    bounds = (np.asarray(tr["latent_min"], np.float32), np.asarray(tr["latent_max"], np.float32))
    agent, _ = _agent(args, tr["steps"], vae_params, bounds)
    trees = W.load_npz(os.path.join(args.dir, "toy_reach_pixels_params.npz"))
    pp, ip = trees["planner"], trees["idm"]
    agent = agent.replace(planner_state=agent.planner_state.replace(params=pp, ema_params=pp), idm_state=agent.idm_state.replace(params=ip, ema_params=ip))
    N, rounds, seed, noise = args.envs, args.rounds, vm["demo_seed"], vm["demo_noise"]
    env = Reach2DPixelEnv(N)

    def blind(batch):
        img = batch["obs"]["image"].clone()
        img[..., 1] = 0                                       # the goal's channel: the agent still sees itself and the disc
        return {"obs": {"pos": batch["obs"]["pos"], "image": img}}
    arms = [
        ("sample ddpm-100", lambda b, r, c: agent.sample(b, r)),
        ("sample ddim-50", lambda b, r, c: agent.sample(b, r, sampler="ddim", n_steps=50)),
        ("sample ddim-10", lambda b, r, c: agent.sample(b, r, sampler="ddim", n_steps=10)),
        ("sample dpmpp-10", lambda b, r, c: agent.sample(b, r, sampler="dpmpp", n_steps=10)),
        ("blind (G zeroed) sample ddim-10", lambda b, r, c: agent.sample(blind(b), r, sampler="ddim", n_steps=10)),
    ]
    results = {}
    for policy in ("expert", "straight"):
        results[policy] = scripted_arm(env, policy, noise, rounds, seed, args.eval_episode0)
        print(policy, json.dumps(results[policy]), flush=True)
        if (N * rounds, seed, noise, args.eval_episode0) == (1024, 0, 0.1, 1_000_000):
            assert results[policy]["success_rate"] == STATE_TASK[policy], \
                f"{policy}: {results[policy]['success_rate']} on the state task's episodes, where it measured {STATE_TASK[policy]}: the task has changed"
    for name, act in arms:
        harness.run_device_eval(env, act, N, seed, args.eval_rng, episode0=args.eval_episode0)                    # warm-up: graphs, tables
        results[name] = harness.run_device_eval(env, act, N * rounds, seed, args.eval_rng, episode0=args.eval_episode0)
        print(name, json.dumps(results[name]), flush=True)
    for res in results.values():
        p, n = res["success_rate"], res["n_rollout"]
        res["success_stderr"] = float(np.sqrt(p * (1 - p) / n))
        if np.isnan(res["mean_first_success"]):
            res["mean_first_success"] = None                   # no success at all (JSON has no NaN)
    out = dict(task="reach2d from pixels", note="toy task: what a 16-number StableVAE latent of this scene preserves; says nothing about a robot",
               ldp_version=_lib.load().ldp_version().decode(), device=torch.cuda.get_device_name(0), episodes_per_arm=N * rounds, envs=N,
               rounds=rounds, env_seed=seed, eval_episode0=args.eval_episode0, eval_rng=args.eval_rng, scripted_noise=noise,
               ms_per_call_note="a control call of a pixel arm includes the StableVAE encode of its 256 frames",
               vae=vm, training=tr, arms=results)
    bench_path = os.path.join(args.dir, "toy_reach_pixels_render.json")
    if os.path.exists(bench_path):
        with open(bench_path) as f:
            out["render"] = json.load(f)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"{'arm':44s} success  +-se   first  blocked  ms/call")
    for name, r in results.items():
        first = "    -" if r["mean_first_success"] is None else f"{r['mean_first_success']:5.1f}"
        print(f"{name:44s} {r['success_rate']:.4f}  {r['success_stderr']:.4f}  {first}  {r['blocked_share']:.4f}  {r['ms_per_call']:8.2f}")
    agent._engine.close()


def render_bench(args):
    """ldp_pix_render at M frames against a torch device-to-device copy_ of a uint8 tensor of the same size: both timed in this process with
    events, alternating, medians over --bench-reps launches after a warm-up.  The copy writes the same bytes and also reads them."""
    from latent_diffusion_planning_amd import _pixlib
    from latent_diffusion_planning_amd.toyenv import _render
    os.makedirs(args.dir, exist_ok=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    lib, stream = _pixlib.load(), torch.cuda.current_stream(dev)
    out = {}
    for M in (98304, 256):
        g = torch.Generator(device="cpu").manual_seed(M)
        pos = (torch.rand((M, 2), generator=g) * 2 - 1).to(dev)
        goal = (torch.rand((M, 2), generator=g) * 2 - 1).to(dev)
        frames = _render(pos.data_ptr(), 2, goal.data_ptr(), 2, M, dev)
        src, dst = frames.clone(), torch.empty_like(frames)
        nbytes = frames.numel()

        def render():
            _pixlib.check(lib.ldp_pix_render(pos.data_ptr(), 2, goal.data_ptr(), 2, M, frames.data_ptr(), stream.cuda_stream))
        times = dict(render=[], copy=[])
        for rep in range(args.bench_warmup + args.bench_reps):
            for name, fn in (("render", render), ("copy", lambda: dst.copy_(src))):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream); fn(); b.record(stream)
                b.synchronize()
                if rep >= args.bench_warmup:
                    times[name].append(a.elapsed_time(b))
        med = {k: float(np.median(v)) for k, v in times.items()}
        out[f"M={M}"] = dict(frames=M, bytes=nbytes, reps=args.bench_reps, render_ms=med["render"], copy_ms=med["copy"],
                             render_ms_min=float(np.min(times["render"])), copy_ms_min=float(np.min(times["copy"])),
                             render_GBps=nbytes / med["render"] / 1e6, copy_GBps=nbytes / med["copy"] / 1e6,
                             note="GB/s = bytes WRITTEN per second; the copy also reads as many")
        print(f"M={M}", json.dumps(out[f"M={M}"]), flush=True)
    out["device"] = torch.cuda.get_device_name(0)
    with open(os.path.join(args.dir, "toy_reach_pixels_render.json"), "w") as f:
        json.dump(out, f)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("stage", choices=["vae", "train", "eval", "render-bench"])
    ap.add_argument("--dir", default="build_toy_pix", help="where a stage leaves its parameters and the next finds them")
    ap.add_argument("--out", default="profiles/toy_reach_pixels_eval.json")
    ap.add_argument("--episodes", type=int, default=2048)
    ap.add_argument("--noise", type=float, default=0.1)
    ap.add_argument("--vae-steps", type=int, default=3000)
    ap.add_argument("--vae-batch", type=int, default=64)
    ap.add_argument("--vae-lr", type=float, default=1e-4)
    ap.add_argument("--held-out", type=int, default=64, help="held-out episodes for the VAE's figures")
    ap.add_argument("--readout-fit", type=int, default=12288, help="demonstration frames the linear read-out is fitted on")
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--log-every", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--eval-episode0", type=int, default=1_000_000)
    ap.add_argument("--eval-rng", type=int, default=17)
    ap.add_argument("--bench-reps", type=int, default=50)
    ap.add_argument("--bench-warmup", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "toy_reach_pixels.py needs a GPU"
    {"vae": vae, "train": train, "eval": evaluate, "render-bench": render_bench}[args.stage](args)


if __name__ == "__main__":
    main()
