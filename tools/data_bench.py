#!/usr/bin/env python3
"""The device-resident data layer, timed on one GPU with synthetic rm-shaped latents (200 episodes x 150 rows, batch 256):

  (a) `DeviceDataset.sample` alone                                  (one launch per batch)
  (b) `agent.update` alone on fixed device batches                  (what `bench.py --train` times)
  (c) the `harness.fit` loop: sample -> update                      (acceptance: (c) - (b) within the spread of (b))
  (d) a NumPy per-sample loader + torch.as_tensor(...).cuda()       (the host path the layer replaces; single process, this host's CPU)
  (e) (a) on a two-camera uint8 64x64x3 image set

Every figure is the median of --repeats runs with their (min, max); (b) and (c) alternate inside one process.  Times are host clocks around
work that ends in a device synchronise.  Prints one JSON line; --out also writes the table as text.

  python tools/data_bench.py --out profiles/data_bench.txt
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


class HostLoader:
    """The per-sample host path, restated: an index -> episode dictionary, two more dictionaries for the episode's start and length, a
    NumPy slice of the welded table per key, and edge padding by concatenating copies of the first / last row."""

    def __init__(self, tables, lengths, obs_keys, fs, sl):
        self.tables, self.obs_keys, self.fs, self.sl = tables, obs_keys, fs, sl
        self.ep_of, self.start_of, self.len_of = {}, {}, {}
        at = 0
        for n, T in enumerate(lengths):
            name = f"demo_{n}"
            self.start_of[name], self.len_of[name] = at, T
            for _ in range(T):
                self.ep_of[at] = name
                at += 1
        self.total = at

    def _window(self, key, lo, hi, front, back):
        seq = self.tables[key][lo:hi]
        if front > 0:
            seq = np.concatenate([seq[:1]] * front + [seq], axis=0)
        if back > 0:
            seq = np.concatenate([seq] + [seq[-1:]] * back, axis=0)
        return seq

    def item(self, i):
        ep = self.ep_of[i]
        s = self.start_of[ep]
        e = s + self.len_of[ep]
        lo, hi = max(i - self.fs + 1, s), min(i + self.sl, e)
        front, back = max(self.fs - (i - lo + 1), 0), max(self.sl - (hi - i), 0)
        out = {"actions": self._window("actions", lo, hi, front, back)[self.fs - 1:], "obs": {}}
        for k in self.obs_keys:
            out["obs"][k] = self._window(k, lo, hi, front, back)
        return out

    def batch(self, B, g):
        items = [self.item(int(g.integers(self.total))) for _ in range(B)]
        host = {"actions": np.stack([it["actions"] for it in items]), "obs": {k: np.stack([it["obs"][k] for it in items]) for k in self.obs_keys}}
        return {"actions": torch.as_tensor(host["actions"]).cuda(), "obs": {k: torch.as_tensor(v).cuda() for k, v in host["obs"].items()}}


def timed(fn, n):
    """ms per call of fn over n calls, the device drained before and after."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def stat(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--episodes", type=int, default=200)
    ap.add_argument("--rows", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50, help="update / fit steps per repeat")
    ap.add_argument("--sample-steps", type=int, default=500, help="sample calls per repeat")
    ap.add_argument("--host-batches", type=int, default=10, help="host-loader batches per repeat")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "data_bench needs a GPU: nothing here is a CPU measurement"
    from latent_diffusion_planning_amd import harness
    from latent_diffusion_planning_amd.data import DeviceDataset
    from tests import cfgs
    from tests.util import idm_params, make_agent, planner_params
    torch.cuda.set_device(0)
    B, T = a.batch, 8
    ag, data = make_agent("rm", planner_params(), idm_params())
    keys = list(data["lowdim_obs"]) + list(data["rgb_obs"])
    eps = []
    for n in range(a.episodes):
        b = cfgs.synth_latent_batch(data, 1, a.rows, 1000 + n, with_actions=True)
        eps.append(dict({k: v[0] for k, v in b["obs"].items()}, actions=b["actions"][0]))
    fs, sl = data["obs_horizon"], T + 1
    ds = DeviceDataset.from_episodes(eps, keys, frame_stack=fs, seq_length=sl)
    table_mb = sum(t.numel() * t.element_size() for t in ds.tables.values()) / 1e6
    fixed = [ds.sample(B, 1, i) for i in range(4)]
    state = {"ag": ag, "step": 0}

    def upd(i):
        state["ag"], _ = state["ag"].update(fixed[i % 4], 100 + state["step"], state["step"])
        state["step"] += 1

    it = ds.batches(B, seed=2)

    def fit_n(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        state["ag"], _ = harness.fit(state["ag"], it, n, 100, log_every=0, start_step=state["step"])
        torch.cuda.synchronize()
        state["step"] += n
        return (time.perf_counter() - t0) / n * 1e3

    timed(upd, 5)
    fit_n(5)
    timed(lambda i: ds.sample(B, 3, i), 20)
    t_a, t_b, t_c = [], [], []
    for _ in range(a.repeats):
        t_a.append(timed(lambda i: ds.sample(B, 3, i), a.sample_steps))
        t_b.append(timed(upd, a.steps))
        t_c.append(fit_n(a.steps))
    # (d) the host path: tables on the host, a batch collated per sample and uploaded
    host_tables = {k: t.cpu().numpy() for k, t in ds.tables.items()}
    hl = HostLoader(host_tables, [a.rows] * a.episodes, keys, fs, sl)
    g = np.random.Generator(np.random.PCG64(0))
    hl.batch(B, g)
    t_d = [timed(lambda i: hl.batch(B, g), a.host_batches) for _ in range(a.repeats)]
    # (e) two cameras of uint8 frames, generated on the device
    n_img = a.episodes * a.rows
    cams = {c: torch.randint(0, 256, (n_img, 64, 64, 3), dtype=torch.uint8, device="cuda") for c in ("agentview_image", "robot0_eye_in_hand_image")}
    st = (torch.arange(n_img, device="cuda", dtype=torch.int32) // a.rows) * a.rows
    ids = DeviceDataset(dict(cams, actions=ds.tables["actions"]), torch.stack([st, st + a.rows], 1).contiguous(), list(cams), ("actions",), 2, 16,
                        [0], [n_img], [1.0], a.episodes)
    img_bytes = 2 * B * 17 * 12288 * 2                       # read + written per batch
    timed(lambda i: ids.sample(B, 3, i), 10)
    t_e = [timed(lambda i: ids.sample(B, 3, i), 100) for _ in range(a.repeats)]
    sa, sb, sc, sd, se = stat(t_a), stat(t_b), stat(t_c), stat(t_d), stat(t_e)
    res = {
        "batch": B, "episodes": a.episodes, "rows_per_episode": a.rows, "tables_MB": round(table_mb, 2), "repeats": a.repeats,
        "a_sample_ms": sa, "b_update_ms": sb, "c_fit_ms": sc, "d_host_loader_ms_per_batch": sd, "e_sample_images_ms": se,
        "b_samples_per_s": B / sb["median"] * 1e3, "c_minus_b_ms": sc["median"] - sb["median"], "b_spread_ms": sb["max"] - sb["min"],
        "c_minus_b_within_spread_of_b": bool(abs(sc["median"] - sb["median"]) <= sb["max"] - sb["min"]),
        "d_batches_per_s": 1e3 / sd["median"], "d_over_b": sd["median"] / sb["median"],
        "e_GBps_read_plus_write": img_bytes / se["median"] / 1e6,
        "note": "(d) is single-process on this host's CPU; d_over_b is the factor by which that loader alone would hold the step back",
    }
    print(json.dumps(res))
    if a.out:
        rows = [("(a) sample alone, rm latents", sa), ("(b) update alone, fixed device batch", sb), ("(c) fit loop: sample -> update", sc),
                ("(d) NumPy per-sample loader + upload (1 process, this host)", sd), ("(e) sample alone, two uint8 cameras, W = 17", se)]
        with open(a.out, "w") as f:
            f.write(f"tools/data_bench.py  batch {B}, {a.episodes} episodes x {a.rows} rows ({table_mb:.1f} MB of tables), median of {a.repeats} (min .. max), ms\n")
            for name, s in rows:
                f.write(f"{name:62s} {s['median']:9.4f}  ({s['min']:.4f} .. {s['max']:.4f})\n")
            f.write(f"(b) = {res['b_samples_per_s']:.0f} samples/s; (c) - (b) = {res['c_minus_b_ms']:+.4f} ms, spread of (b) = {res['b_spread_ms']:.4f} ms; "
                    f"(d) / (b) = {res['d_over_b']:.1f}x; (e) = {res['e_GBps_read_plus_write']:.0f} GB/s read + written\n")
            f.write(json.dumps(res) + "\n")
    ag._engine.close()


if __name__ == "__main__":
    main()
