#!/usr/bin/env python3
"""push2d: two measurements on the pushing task, every stage a GPU process of its own, to be run under its own time limit
and chained.

(a) The planning modes.  An LDP agent is trained on --episodes expert episodes and every arm runs on the same held-out episodes:

  timeout -k 10 600 python tools/toy_push.py train --dir build_push \\
    && timeout -k 10 600 python tools/toy_push.py eval --dir build_push --out profiles/toy_push_eval.json

(b) Mixed data: does a planner trained on action-free demonstrations, with an IDM trained on a few labelled (and on suboptimal) episodes,
control better than an agent trained on the few labelled episodes alone?  One process per arm, then the report:

  for every L in 16 64 and ARM in few af af_sub_half af_sub_prop:
      timeout -k 10 600 python tools/toy_push.py arm --dir build_push --labelled L --arm ARM  &&  ...
  python tools/toy_push.py report --dir build_push --out profiles/toy_push_mixed.json

  few          update        planner and IDM on the L labelled expert episodes
  af           update_mixed  planner on the --episodes expert episodes with their actions zeroed, IDM on the L labelled ones
  af_sub_half  update_mixed  as af, the IDM on DeviceDataset.mix of the L labelled episodes and --episodes random-policy episodes, split 0.5 / 0.5
  af_sub_prop  update_mixed  the same with the split proportional to the rows

Every arm has the same steps, batch, schedule and seeds, is evaluated under `sample` DDIM-10 on the episodes of (a), and reports its final
planner and IDM losses on --heldout held-out expert episodes.  The labelled episodes are the first L of the expert's.
A TOY task: the figures rank methods on it and say nothing about a robot."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tools.toy_reach import add_stderr, make_agent, print_table, scripted_arm

ARMS = ("few", "af", "af_sub_half", "af_sub_prop")
EXTRA = (("contact", ".4f", "contact_share"), ("left", ".4f", "success_left"), ("right", ".4f", "success_right"))


def _push_env(n, action_dim):
    """A Push2DEnv that keeps the state at the end of every round (keyed by the round's first episode, so that a round run again replaces
    its own entry): run_device_eval and scripted_arm read `first_success()` once, when a round is over."""
    from latent_diffusion_planning_amd.pushenv import Push2DEnv

    class Recording(Push2DEnv):
        rounds: dict = {}

        def first_success(self):
            self.rounds[self.episode0] = self.state.clone()
            return super().first_success()
    env = Recording(n, action_dim=action_dim)
    env.rounds = {}
    return env


def _by_side(env, res):
    """The columns push2d adds to reach2d's: the share of moves that moved the disc, and success with the goal on the left (the point
    starts on the wrong side of the disc) and on the right."""
    s = torch.cat([env.rounds[k] for k in sorted(env.rounds)]).cpu().numpy()
    assert len(s) == res["n_rollout"], (len(s), res["n_rollout"])
    ok, left = s[:, 8] != 0, s[:, 4] < 0
    res.update(contact_share=float(s[:, 10].sum() / (len(s) * env.episode_len)), n_left=int(left.sum()), n_right=int((~left).sum()),
               success_left=float(ok[left].mean()), success_right=float(ok[~left].mean()))
    for side in ("left", "right"):
        p, n = res["success_" + side], res["n_" + side]
        res[f"success_{side}_stderr"] = float(np.sqrt(p * (1 - p) / n))
    return res


def _config(**kw):
    from latent_diffusion_planning_amd.pushenv import push2d_config
    return push2d_config(**kw)


def _curve(curve, args, t0):
    def on_log(step, m):
        curve.append(dict(step=step, loss=m["loss"], plan_loss=m["plan_loss"], idm_loss=m["idm_loss"], g_norm=m.get("g_norm")))
        if step % (10 * args.log_every) == 0:
            print(f"step {step}: loss {m['loss']:.5f} (plan {m['plan_loss']:.5f}, idm {m['idm_loss']:.5f})  {time.time() - t0:.0f} s", flush=True)
    return on_log


def _identity():
    from latent_diffusion_planning_amd import _lib
    return dict(ldp_version=_lib.load().ldp_version().decode(), device=torch.cuda.get_device_name(0))


def _with_params(args, steps, planner, idm):
    """A fresh agent that samples with the trained parameters (as toy_reach.py's eval stage: the parameters stand for their EMA too)."""
    agent, cfg = make_agent(args, steps, _config)
    return agent.replace(planner_state=agent.planner_state.replace(params=planner, ema_params=planner),
                         idm_state=agent.idm_state.replace(params=idm, ema_params=idm)), cfg


def train(args):
    from latent_diffusion_planning_amd import harness, weights as W
    from latent_diffusion_planning_amd.pushenv import collect_push_demos
    os.makedirs(args.dir, exist_ok=True)
    t0 = time.time()
    ds = collect_push_demos(args.episodes, args.seed, args.noise, episode0=0, action_dim=args.action_dim)
    agent, _ = make_agent(args, args.steps, _config)
    curve = []
    t1 = time.time()
    agent, _ = harness.fit(agent, ds.batches(args.batch, seed=args.seed + 1), args.steps, args.seed + 2, log_every=args.log_every,
                           on_log=_curve(curve, args, t0))
    planner, idm = dict(agent.planner_state.params), dict(agent.idm_state.params)          # (fetched from the training arenas)
    train_s = time.time() - t1
    W.save_npz(os.path.join(args.dir, "toy_push_params.npz"), planner=planner, idm=idm)
    meta = dict(episodes=args.episodes, demo_seed=args.seed, demo_noise=args.noise, demo_rows=ds.total_n_sequences, steps=args.steps, batch=args.batch,
                lr=args.lr, action_dim=args.action_dim, batch_seed=args.seed + 1, fit_seed=args.seed + 2, train_seconds=train_s,
                ms_per_step=1e3 * train_s / max(args.steps, 1), loss_curve=curve, **_identity())
    with open(os.path.join(args.dir, "toy_push_train.json"), "w") as f:
        json.dump(meta, f)
    print(json.dumps({k: v for k, v in meta.items() if k != "loss_curve"}), flush=True)


def _eval_arm(env, act, args, seed, on_reset=None):
    from latent_diffusion_planning_amd import harness
    N = env.n_envs
    harness.run_device_eval(env, act, N, seed, args.eval_rng, on_reset=on_reset, episode0=args.eval_episode0)                 # warm-up: graphs, tables
    env.rounds.clear()
    return _by_side(env, harness.run_device_eval(env, act, N * args.rounds, seed, args.eval_rng, on_reset=on_reset, episode0=args.eval_episode0))


def evaluate(args):
    from latent_diffusion_planning_amd import weights as W
    with open(os.path.join(args.dir, "toy_push_train.json")) as f:
        tr = json.load(f)
    args.action_dim = tr["action_dim"]
    trees = W.load_npz(os.path.join(args.dir, "toy_push_params.npz"))
    agent, _ = _with_params(args, tr["steps"], trees["planner"], trees["idm"])
    N, rounds = args.envs, args.rounds
    env = _push_env(N, args.action_dim)
    slots = list(range(N))
    rp = agent.replanner(N, warm_steps=10, sampler="ddim", n_steps=50)
    arms = [
        ("sample ddpm-100", lambda b, r, c: agent.sample(b, r), None),
        ("sample ddim-50", lambda b, r, c: agent.sample(b, r, sampler="ddim", n_steps=50), None),
        ("sample ddim-10", lambda b, r, c: agent.sample(b, r, sampler="ddim", n_steps=10), None),
        ("sample dpmpp-10", lambda b, r, c: agent.sample(b, r, sampler="dpmpp", n_steps=10), None),
        ("replanner ddim-50 warm 10", lambda b, r, c: rp.act(b, r, slots), rp.reset),
    ]
    results = {}
    for policy in ("expert", "straight", "random"):
        env.rounds.clear()
        results[policy] = _by_side(env, scripted_arm(env, policy, tr["demo_noise"], rounds, tr["demo_seed"], args.eval_episode0))
        print(policy, json.dumps(results[policy]), flush=True)
    for name, act, on_reset in arms:
        results[name] = _eval_arm(env, act, args, tr["demo_seed"], on_reset)
        print(name, json.dumps(results[name]), flush=True)
    add_stderr(results)
    out = dict(task="push2d", note="toy task: ranks the planning modes on push2d, says nothing about a robot", episodes_per_arm=N * rounds, envs=N,
               rounds=rounds, env_seed=tr["demo_seed"], eval_episode0=args.eval_episode0, eval_rng=args.eval_rng, scripted_noise=tr["demo_noise"],
               agent_seed=args.seed, training={k: v for k, v in tr.items()}, arms=results, **_identity())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print_table(results, EXTRA)
    agent._engine.close()


def arm(args):
    """One arm of the mixed-data table: train, evaluate under `sample` DDIM-10, held-out losses -> <dir>/toy_push_arm_<L>_<arm>.json."""
    from latent_diffusion_planning_amd import harness
    from latent_diffusion_planning_amd.data import DeviceDataset
    from latent_diffusion_planning_amd.pushenv import collect_push_demos, without_actions
    os.makedirs(args.dir, exist_ok=True)
    t0 = time.time()
    L, A = args.labelled, args.action_dim
    few = collect_push_demos(L, args.seed, args.noise, episode0=0, action_dim=A)            # the first L of the expert's episodes, labelled
    data = dict(labelled_episodes=L, labelled_rows=few.total_n_sequences)
    if args.arm == "few":
        plan_iter, mixed_iter = few.batches(args.batch, seed=args.seed + 1), None
    else:
        free = without_actions(collect_push_demos(args.episodes, args.seed, args.noise, episode0=0, action_dim=A))
        assert not bool(free.tables["actions"].any())
        plan_iter, idm_data = free.batches(args.batch, seed=args.seed + 1), few
        data.update(action_free_episodes=args.episodes)
        if args.arm != "af":
            sub = collect_push_demos(args.episodes, args.seed, args.noise, episode0=args.suboptimal_episode0, policy="random", action_dim=A)
            share = 0.5 if args.arm == "af_sub_half" else few.total_n_sequences / (few.total_n_sequences + sub.total_n_sequences)
            idm_data = DeviceDataset.mix([few, sub], share)
            data.update(suboptimal_episodes=args.episodes, suboptimal_policy="random", suboptimal_episode0=args.suboptimal_episode0,
                        split=[share, 1 - share])
        mixed_iter = idm_data.batches(args.batch, seed=args.seed + 3)
    agent, _ = make_agent(args, args.steps, _config)
    curve = []
    t1 = time.time()
    agent, _ = harness.fit(agent, plan_iter, args.steps, args.seed + 2, log_every=args.log_every, on_log=_curve(curve, args, t0), mixed_iter=mixed_iter)
    planner, idm = dict(agent.planner_state.params), dict(agent.idm_state.params)
    train_s = time.time() - t1
    agent._engine.close()
    agent, _ = _with_params(args, args.steps, planner, idm)
    held = collect_push_demos(args.heldout, args.seed, args.noise, episode0=args.heldout_episode0, action_dim=A)
    losses = [agent.get_metrics(held.sample(args.batch, args.seed + 4, i), args.seed + 5 + i) for i in range(args.heldout_batches)]
    heldout = {k: float(np.mean([float(m[k]) for m in losses])) for k in ("plan_loss", "idm_loss")}
    env = _push_env(args.envs, A)
    res = _eval_arm(env, lambda b, r, c: agent.sample(b, r, sampler="ddim", n_steps=10), args, args.seed)
    out = dict(arm=args.arm, call="update" if args.arm == "few" else "update_mixed", data=data, steps=args.steps, batch=args.batch, lr=args.lr,
               agent_seed=args.seed, demo_seed=args.seed, demo_noise=args.noise, batch_seed=args.seed + 1, fit_seed=args.seed + 2,
               idm_batch_seed=args.seed + 3, train_seconds=train_s, ms_per_step=1e3 * train_s / max(args.steps, 1), wall_seconds=time.time() - t0,
               heldout_episodes=args.heldout, heldout_episode0=args.heldout_episode0, heldout_plan_loss=heldout["plan_loss"],
               heldout_idm_loss=heldout["idm_loss"], eval=res, loss_curve=curve, **_identity())
    with open(os.path.join(args.dir, f"toy_push_arm_{L}_{args.arm}.json"), "w") as f:
        json.dump(out, f)
    print(json.dumps({k: v for k, v in out.items() if k != "loss_curve"}), flush=True)
    agent._engine.close()


def report(args):
    """Weld the arms found in --dir (and the `full` ceiling of stage eval's table, when --full names it) into --out.  No GPU."""
    arms = {}
    for L in (16, 64):
        for name in ARMS:
            path = os.path.join(args.dir, f"toy_push_arm_{L}_{name}.json")
            if os.path.exists(path):
                with open(path) as f:
                    arms[f"L={L} {name}"] = json.load(f)
    if not arms:
        raise SystemExit(f"no toy_push_arm_*.json in {args.dir}")
    first = next(iter(arms.values()))
    results = {k: v["eval"] for k, v in arms.items()}
    full = None
    if args.full and os.path.exists(args.full):
        with open(args.full) as f:
            ev = json.load(f)
        full = dict(source=os.path.basename(args.full), training_episodes=ev["training"]["episodes"], **ev["arms"]["sample ddim-10"])
        results = {"full (ceiling)": full, **results}
    add_stderr(results)
    for v in arms.values():
        v["eval"]["heldout_plan_loss"], v["eval"]["heldout_idm_loss"], v["eval"]["train_seconds"] = v["heldout_plan_loss"], v["heldout_idm_loss"], v["train_seconds"]
    out = dict(task="push2d", note="toy task, one training seed per arm: says nothing about a robot", ldp_version=first["ldp_version"], device=first["device"],
               evaluation="sample ddim-10", episodes_per_arm=first["eval"]["n_rollout"], eval_episode0=args.eval_episode0, eval_rng=args.eval_rng,
               full=full, arms=arms)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print_table(results, EXTRA + (("plan loss", ".5f", "heldout_plan_loss"), ("idm loss", ".5f", "heldout_idm_loss"), ("train s", ".0f", "train_seconds")))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("stage", choices=["train", "eval", "arm", "report"])
    ap.add_argument("--dir", default="build_push", help="where a stage leaves its results and the next finds them")
    ap.add_argument("--out", default=None, help="default: profiles/toy_push_eval.json (eval), profiles/toy_push_mixed.json (report)")
    ap.add_argument("--full", default="profiles/toy_push_eval.json", help="report: the table of stage eval, for the ceiling")
    ap.add_argument("--arm", choices=ARMS, default="few")
    ap.add_argument("--labelled", type=int, default=16, help="L: labelled expert episodes of an arm")
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
    ap.add_argument("--suboptimal-episode0", type=int, default=500_000)
    ap.add_argument("--heldout", type=int, default=64)
    ap.add_argument("--heldout-episode0", type=int, default=2_000_000)
    ap.add_argument("--heldout-batches", type=int, default=8)
    args = ap.parse_args()
    if args.out is None:
        args.out = "profiles/toy_push_mixed.json" if args.stage == "report" else "profiles/toy_push_eval.json"
    if args.stage == "report":
        return report(args)
    assert torch.cuda.is_available(), "toy_push.py needs a GPU"
    dict(train=train, eval=evaluate, arm=arm)[args.stage](args)


if __name__ == "__main__":
    main()
