"""ORACLE (test infrastructure, NOT a product path) -- the training data layer's semantics restated in NumPy with
plain loops, independently of latent_diffusion_planning_amd/data.py and csrc/data.hip: weld, window, draw.

Weld: episodes in `demo_<n>` order (by n), `n_overfit` applied after the sort, every key's episodes one behind the other.
Window: sample i of episode [s, e): observation row j is welded row clamp(i - (fs - 1) + j, s, e - 1), j < W = fs + sl - 1; the dataset
keys (actions) take rows j = fs - 1 .. W - 1.
Draw: row r of a call takes the Philox words w of (seed, elem r, step, stream 11): dataset = first d with w[1] < thr[d], index =
base[d] + (w[0] * total[d] >> 32).
"""
import numpy as np

from oracle import philox

STREAM_DATA = 11


def demo_sort(names):
    return sorted(names, key=lambda n: int(n[len("demo_"):]))


def select(names, n_overfit):
    """names: already sorted.  None: all; int: the first n; list: the named ones, in sorted order."""
    if n_overfit is None:
        return list(names)
    if isinstance(n_overfit, int):
        assert n_overfit <= len(names)
        return list(names[:n_overfit])
    return [n for n in names if n in list(n_overfit)]


def episode_rows(obs, next_obs, actions, latents, obs_keys, optimal, append_last):
    """One episode of a file -> {key: rows}.  obs / next_obs: {key: (T, ...)}, latents: {cam: (T + 1 | T, ...)}.  robomimic
    (append_last): T + 1 rows -- obs + the last next_obs row, actions + its last row again; ALOHA: T rows."""
    T = len(actions)
    n = T + 1 if append_last else T
    out = {}
    for k in obs_keys:
        if k == "optimal":
            out[k] = np.full((n, 1), float(optimal), np.float32)
        elif "latent" in k:
            out[k] = np.asarray(latents[k.replace("latent_", "")])
            assert len(out[k]) == n
        else:
            rows = [obs[k][t] for t in range(T)]
            if append_last:
                rows.append(next_obs[k][T - 1])
            out[k] = np.stack(rows)
    rows = [actions[t] for t in range(T)]
    if append_last:
        rows.append(actions[T - 1])
    out["actions"] = np.stack(rows)
    return out


def weld(episodes, keys, optimal=1):
    """episodes: list of {key: (T, ...)} -> ({key: (total, ...)}, starts, ends) with the episode [starts[i], ends[i]) of every welded row i."""
    tables = {k: [] for k in keys}
    starts, ends = [], []
    at = 0
    for ep in episodes:
        T = len(ep[keys[0]]) if keys[0] in ep else len(ep["actions"])
        for k in keys:
            for t in range(T):
                tables[k].append(np.full((1,), float(optimal), np.float32) if (k == "optimal" and k not in ep) else np.asarray(ep[k][t]))
        for _ in range(T):
            starts.append(at)
            ends.append(at + T)
        at += T
    out = {}
    for k in keys:
        a = np.stack(tables[k])
        a = a if a.dtype == np.uint8 else a.astype(np.float32)
        out[k] = a.reshape(len(a), -1) if a.ndim == 1 else a
    return out, np.asarray(starts), np.asarray(ends)


def window_rows(i, s, e, fs, sl, first=0):
    """Welded rows of the window of sample i in episode [s, e), from window row `first` on."""
    rows = []
    for j in range(first, fs + sl - 1):
        r = i - (fs - 1) + j
        r = s if r < s else (e - 1 if r > e - 1 else r)
        rows.append(r)
    return rows


def batch(tables, starts, ends, indices, obs_keys, dataset_keys, fs, sl):
    """-> {'obs': {key: (B, W, ...)}, dataset key: (B, sl, ...)} for the welded-row indices given."""
    out = {"obs": {}}
    for k in list(dataset_keys) + list(obs_keys):
        first = fs - 1 if k in dataset_keys else 0
        win = []
        for i in indices:
            i = int(i)
            win.append(np.stack([tables[k][r] for r in window_rows(i, int(starts[i]), int(ends[i]), fs, sl, first)]))
        if k in dataset_keys:
            out[k] = np.stack(win)
        else:
            out["obs"][k] = np.stack(win)
    return out


def thresholds(split):
    """floor(cumulative split * 2^32) as Python ints, the last forced to 2^32; a float s means [s, 1 - s]."""
    if isinstance(split, float):
        split = [split, 1.0 - split]
    thr, c = [], 0.0
    for s in split:
        c = c + float(s)
        thr.append(int(np.floor(c * 2.0 ** 32)))
    thr[-1] = 2 ** 32
    return thr


def draw(seed, step, row_offset, B, totals, split=(1.0,)):
    """-> (dataset (B,), index within the dataset (B,), welded index (B,)) as Python-int arrays."""
    thr = thresholds(list(split))
    base = [0]
    for t in totals[:-1]:
        base.append(base[-1] + int(t))
    w = philox.words(seed, row_offset, step, STREAM_DATA, B)
    ds, idx, welded = [], [], []
    for b in range(B):
        w0, w1 = int(w[b, 0]), int(w[b, 1])
        d = 0
        while not w1 < thr[d]:
            d += 1
        i = (w0 * int(totals[d])) >> 32
        ds.append(d)
        idx.append(i)
        welded.append(base[d] + i)
    return np.asarray(ds, np.int64), np.asarray(idx, np.int64), np.asarray(welded, np.int64)
