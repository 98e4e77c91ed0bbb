#!/usr/bin/env python3
"""reach2d: collect expert demonstrations on the GPU, train an LDP agent on them, and measure closed-loop success of
every planning mode of this package against the scripted expert (ceiling) and the straight-line policy (floor) on the same episodes.

Two stages, each a GPU process of its own, to be run under its own time limit and chained:

  timeout -k 10 900 python tools/toy_reach.py train --dir build_toy \\
    && timeout -k 10 900 python tools/toy_reach.py eval --dir build_toy --out profiles/toy_reach_eval.json

`train` collects --episodes expert episodes (global episodes 0 .. of --seed) at --noise, runs harness.fit for --steps steps at --batch from
DeviceDataset.batches and writes the parameters and the loss curve into --dir.  `eval` loads them and runs every arm on --rounds rounds
of --envs environments (global episodes --eval-episode0 .., disjoint from the demonstrations'), then writes the table.
A TOY task: the figures rank the planning modes on it and say nothing about a robot."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def make_agent(args, decay_steps, config=None):
    """config: the task's counterpart of toyenv.reach2d_config (default: reach2d's own)."""
    from latent_diffusion_planning_amd.agent import LDPAgent
    from latent_diffusion_planning_amd.toyenv import reach2d_config
    cfg = (config or reach2d_config)(action_dim=args.action_dim, lr=args.lr, warmup_steps=min(500, max(decay_steps // 10, 1)), decay_steps=decay_steps)
    return LDPAgent.create(args.seed, None, cfg["shape_meta"], **cfg["agent_kwargs"]), cfg


def train(args):
    from latent_diffusion_planning_amd import harness, weights as W
    from latent_diffusion_planning_amd.toyenv import collect_demos
    os.makedirs(args.dir, exist_ok=True)
    t0 = time.time()
    ds = collect_demos(args.episodes, args.seed, args.noise, episode0=0, action_dim=args.action_dim)
    agent, _ = make_agent(args, args.steps)
    curve = []

    def on_log(step, m):
        curve.append(dict(step=step, loss=m["loss"], plan_loss=m["plan_loss"], idm_loss=m["idm_loss"], g_norm=m.get("g_norm")))
        if step % (10 * args.log_every) == 0:
            print(f"step {step}: loss {m['loss']:.5f} (plan {m['plan_loss']:.5f}, idm {m['idm_loss']:.5f})  {time.time() - t0:.0f} s", flush=True)
    t1 = time.time()
    agent, _ = harness.fit(agent, ds.batches(args.batch, seed=args.seed + 1), args.steps, args.seed + 2, log_every=args.log_every, on_log=on_log)
    planner, idm = dict(agent.planner_state.params), dict(agent.idm_state.params)          # (fetched from the training arenas)
    train_s = time.time() - t1
    W.save_npz(os.path.join(args.dir, "toy_reach_params.npz"), planner=planner, idm=idm)
    meta = dict(episodes=args.episodes, demo_seed=args.seed, demo_noise=args.noise, demo_rows=ds.total_n_sequences, steps=args.steps, batch=args.batch,
                lr=args.lr, action_dim=args.action_dim, train_seconds=train_s, ms_per_step=1e3 * train_s / max(args.steps, 1), loss_curve=curve)
    with open(os.path.join(args.dir, "toy_reach_train.json"), "w") as f:
        json.dump(meta, f)
    print(json.dumps({k: v for k, v in meta.items() if k != "loss_curve"}), flush=True)


def scripted_arm(env, policy, noise, rounds, seed, episode0):
    """A scripted policy on the same episodes: one launch per round."""
    first, blocked, wall = [], [], 0.0
    for r in range(rounds):
        env.reset(seed, episode0 + r * env.n_envs)
        t0 = time.perf_counter()
        env.step_scripted(policy, noise, n_sub=env.episode_len)
        first.append(env.first_success().cpu().numpy()); blocked.append(env.blocked().cpu().numpy())
        wall += time.perf_counter() - t0
    first, blocked = np.concatenate(first).astype(np.int64), np.concatenate(blocked).astype(np.int64)
    ok = first != 0
    return dict(success_rate=float(ok.mean()), mean_first_success=float(first[ok].mean()) if ok.any() else float("nan"),
                blocked_share=float(blocked.sum() / (blocked.size * env.episode_len)), ms_per_call=1e3 * wall / rounds, n_rollout=int(first.size),
                n_calls=rounds, cycles_per_episode=1)


def add_stderr(results):
    """success_stderr = sqrt(p (1 - p) / n) for every arm, in place; a mean over no success becomes None (JSON has no NaN)."""
    for res in results.values():
        p, n = res["success_rate"], res["n_rollout"]
        res["success_stderr"] = float(np.sqrt(p * (1 - p) / n))
        if res["mean_first_success"] is not None and np.isnan(res["mean_first_success"]):
            res["mean_first_success"] = None                   # no success at all (JSON has no NaN)


def print_table(results, extra=()):
    """One line per arm; extra: (heading, format, key) of further columns (default: none, reach2d's table)."""
    print(f"{'arm':44s} success  +-se   first  blocked  ms/call" + "".join(f"  {h}" for h, _, _ in extra))
    for name, r in results.items():
        first = "    -" if r["mean_first_success"] is None else f"{r['mean_first_success']:5.1f}"
        more = "".join("  " + ("-".rjust(len(h)) if r.get(k) is None else format(r[k], f).rjust(len(h))) for h, f, k in extra)
        print(f"{name:44s} {r['success_rate']:.4f}  {r['success_stderr']:.4f}  {first}  {r['blocked_share']:.4f}  {r['ms_per_call']:8.2f}" + more)


def evaluate(args):
    from latent_diffusion_planning_amd import _lib, harness, weights as W
    from latent_diffusion_planning_amd.toyenv import Reach2DEnv
    with open(os.path.join(args.dir, "toy_reach_train.json")) as f:
        tr = json.load(f)
    args.action_dim = tr["action_dim"]
    agent, cfg = make_agent(args, tr["steps"])
    trees = W.load_npz(os.path.join(args.dir, "toy_reach_params.npz"))
    pp, ip = trees["planner"], trees["idm"]
    agent = agent.replace(planner_state=agent.planner_state.replace(params=pp, ema_params=pp), idm_state=agent.idm_state.replace(params=ip, ema_params=ip))
    N, rounds = args.envs, args.rounds
    env = Reach2DEnv(N, action_dim=args.action_dim)
    slots = list(range(N))
    T = cfg["agent_kwargs"]["pred_horizon"]
    rp = agent.replanner(N, warm_steps=10, sampler="ddim", n_steps=50)
    ct = agent.controller(N, warm_steps=2, sampler="dpmpp", n_steps=10)
    guide = agent.build_guide(N, smooth=args.smooth, anchor=True)
    arms = [
        ("sample ddpm-100", lambda b, r, c: agent.sample(b, r), None),
        ("sample ddim-50", lambda b, r, c: agent.sample(b, r, sampler="ddim", n_steps=50), None),
        ("sample ddim-10", lambda b, r, c: agent.sample(b, r, sampler="ddim", n_steps=10), None),
        ("sample dpmpp-10", lambda b, r, c: agent.sample(b, r, sampler="dpmpp", n_steps=10), None),
        ("replanner ddim-50 warm 10", lambda b, r, c: rp.act(b, r, slots), rp.reset),
        ("controller dpmpp-10 warm 2", lambda b, r, c: ct.act(b, r, slots), ct.reset),                       # the next arm without its guide
        (f"controller dpmpp-10 warm 2 smooth {args.smooth:g}", lambda b, r, c: ct.act(b, r, slots, guide=guide), ct.reset),
        ("best-of-16 goal ddim-10", lambda b, r, c: agent.sample_best_of(b, r, 16, score="goal", goal=env.goal_observation(), t_goal=T - 1,
                                                                         sampler="ddim", n_steps=10), None),
    ]
    results = {}
    for policy in ("expert", "straight"):
        results[policy] = scripted_arm(env, policy, tr["demo_noise"], rounds, tr["demo_seed"], args.eval_episode0)
        print(policy, json.dumps(results[policy]), flush=True)
    for name, act, on_reset in arms:
        harness.run_device_eval(env, act, N, tr["demo_seed"], args.eval_rng, on_reset=on_reset, episode0=args.eval_episode0)      # warm-up: graphs, tables
        results[name] = harness.run_device_eval(env, act, N * rounds, tr["demo_seed"], args.eval_rng, on_reset=on_reset, episode0=args.eval_episode0)
        print(name, json.dumps(results[name]), flush=True)
    add_stderr(results)
    out = dict(task="reach2d", note="toy task: ranks the planning modes on reach2d, says nothing about a robot", ldp_version=_lib.load().ldp_version().decode(),
               device=torch.cuda.get_device_name(0), episodes_per_arm=N * rounds, envs=N, rounds=rounds, env_seed=tr["demo_seed"],
               eval_episode0=args.eval_episode0, eval_rng=args.eval_rng, scripted_noise=tr["demo_noise"],
               training={k: v for k, v in tr.items()}, arms=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print_table(results)
    agent._engine.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("stage", choices=["train", "eval"])
    ap.add_argument("--dir", default="build_toy", help="where train leaves the parameters and eval finds them")
    ap.add_argument("--out", default="profiles/toy_reach_eval.json")
    ap.add_argument("--episodes", type=int, default=2048)
    ap.add_argument("--noise", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--log-every", type=int, default=200)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--action-dim", type=int, default=2)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--eval-episode0", type=int, default=1_000_000)
    ap.add_argument("--eval-rng", type=int, default=17)
    ap.add_argument("--smooth", type=float, default=0.25, help="lam of the controller arm's smoothness guide")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "toy_reach.py needs a GPU"
    train(args) if args.stage == "train" else evaluate(args)


if __name__ == "__main__":
    main()
