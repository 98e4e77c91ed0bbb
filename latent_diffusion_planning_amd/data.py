"""Device-resident training data -- counterpart of data/robomimic_latent_data.py, data/alohasim_latent_data.py and the `*_mixed_*`
variants.

The reference welds every episode into one table per key on the host and then, per SAMPLE, looks up three dictionaries, slices a NumPy
window and pads it with up to 2 * (keys) `np.concatenate` calls (robomimic_latent_data.py:116-147); the batch is collated in DataLoader
workers, turned into NumPy (train_bc.py:78) and uploaded.  Here the welded tables are uploaded ONCE; every batch after that is one kernel
launch (csrc/data.hip: `ldp_data_sample`) that draws the window indices from Philox and gathers the episode-clamped windows of every key.
The batch dict holds device tensors, which `update` / `get_metrics` / `dist.update_sharded` take as they are (arrays.as_tensor passes
a device tensor through): no host work, no H2D copy, no synchronisation per step.  A batch is a pure function of (tables, seed, step,
row_offset), so every rank of `update_sharded` -- which wants the FULL batch on every rank -- draws the same one without communication.

Semantics in one place: DESIGN.md 4.15 (weld, window, draw); tests/data_oracle.py restates them in NumPy.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Dict, Iterator, List, Mapping, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .preencode import demo_order


def split_thresholds(split: Sequence[float]) -> List[int]:
    """uint64 thresholds of the dataset choice: floor(cumulative split * 2^32), the last one forced to 2^32 (a draw w1 < 2^32 always
    lands somewhere).  Computed on the host, in float64, adding the entries in order."""
    thr, c = [], 0.0
    for s in split:
        c += float(s)
        thr.append(min(max(int(np.floor(c * 4294967296.0)), 0), 1 << 32))
    thr[-1] = 1 << 32
    return thr


def _as_split(split, n: int) -> List[float]:
    """`train_split` of the mixed classes (robomimic_mixed_latent_data.py:44-47): a float s means [s, 1 - s]; a list must sum to 1."""
    if isinstance(split, (int, float, np.floating)):
        split = [float(split), 1.0 - float(split)]
    split = [float(s) for s in split]
    if len(split) != n:
        raise ValueError(f"split has {len(split)} entries for {n} datasets")
    if any(s < 0 for s in split) or abs(sum(split) - 1.0) > 1e-9:
        raise ValueError(f"split must be non-negative and sum to 1, got {split}")
    return split


def _table(a) -> np.ndarray:
    """uint8 stays uint8 (camera frames: the agents cast on the device); everything else becomes float32 (the reference's float64
    low-dim rows reach its networks as float32 too)."""
    a = np.asarray(a)
    return np.ascontiguousarray(a if a.dtype == np.uint8 else a.astype(np.float32))


class DeviceDataset:
    """One welded dataset, or a mixture of welded datasets, resident in HBM.

    tables[key] is the (total, ...) device tensor of every episode's rows of `key`, one episode behind the other; `bounds` (total, 2)
    int32 holds the episode [start, end) of every welded row.  Build one with `from_episodes`, `from_files` or `mix`."""

    def __init__(self, tables: Mapping[str, torch.Tensor], bounds: torch.Tensor, obs_keys: Sequence[str], dataset_keys: Sequence[str],
                 frame_stack: int, seq_length: int, set_base: Sequence[int], set_total: Sequence[int], split: Sequence[float],
                 n_demos: int, env_meta: Optional[dict] = None):
        self.obs_keys, self.dataset_keys = tuple(obs_keys), tuple(dataset_keys)
        self.frame_stack, self.seq_length = int(frame_stack), int(seq_length)
        if self.frame_stack < 1 or self.seq_length < 1:
            raise ValueError("frame_stack and seq_length must be >= 1")
        self.tables = {k: tables[k] for k in self.dataset_keys + self.obs_keys}
        self.bounds = bounds
        self.device = bounds.device
        self.total_n_sequences = int(bounds.shape[0])
        self.n_demos = int(n_demos)
        self.env_meta = env_meta
        self.split = [float(s) for s in split]
        self.set_base, self.set_total = [int(v) for v in set_base], [int(v) for v in set_total]
        n = len(self.set_base)
        if len(self.tables) > _lib.DATA_MAX_KEYS:
            raise ValueError(f"{len(self.tables)} keys: one launch gathers at most {_lib.DATA_MAX_KEYS}")
        if n > _lib.DATA_MAX_SETS:
            raise ValueError(f"{n} datasets: a mixture holds at most {_lib.DATA_MAX_SETS}")
        if any(t < 1 or t >= 2**31 for t in self.set_total) or self.total_n_sequences >= 2**31:
            raise ValueError("every dataset needs 1 <= total < 2^31 welded rows (the draw's multiply-shift map, int32 episode bounds)")
        for k, t in self.tables.items():
            if t.shape[0] != self.total_n_sequences or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"table {k!r}: expected a contiguous ({self.total_n_sequences}, ...) tensor on {self.device}")
            if self._row_bytes(t) % 4:
                raise ValueError(f"table {k!r}: rows of {self._row_bytes(t)} bytes; the copy moves 4-byte words")
        self._base = (C.c_int64 * n)(*self.set_base)
        self._total = (C.c_int64 * n)(*self.set_total)
        self._thr = (C.c_uint64 * n)(*split_thresholds(self.split))
        self._n_sets = n

    # ---- construction ------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_episodes(cls, episodes: Sequence[Mapping[str, np.ndarray]], obs_keys: Sequence[str], dataset_keys: Sequence[str] = ("actions",),
                      frame_stack: int = 1, seq_length: int = 1, optimal=1, device=None, env_meta: Optional[dict] = None) -> "DeviceDataset":
        """episodes: a list of {key: ndarray (T, ...)}, already in weld order and with the rows the flavour wants (robomimic: T + 1).  The
        key 'optimal', when asked for and absent, is a one-column table filled with `optimal`.  One upload per key, here."""
        if not episodes:
            raise ValueError("no episodes")
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        keys = tuple(dataset_keys) + tuple(obs_keys)
        lengths = [int(np.asarray(ep[keys[0]]).shape[0]) for ep in episodes]
        if min(lengths) < 1:
            raise ValueError("an episode needs at least one row")
        host: Dict[str, np.ndarray] = {}
        for k in keys:
            parts = []
            for ep, T in zip(episodes, lengths):
                a = np.full((T, 1), float(optimal), np.float32) if (k == "optimal" and k not in ep) else _table(ep[k])
                if a.shape[0] != T:
                    raise ValueError(f"key {k!r}: {a.shape[0]} rows in an episode of {T}")
                parts.append(a.reshape(T, -1) if a.ndim == 1 else a)
            host[k] = np.concatenate(parts, axis=0)
        starts = np.concatenate([[0], np.cumsum(lengths)])
        bounds = np.empty((int(starts[-1]), 2), np.int32)
        for s, e in zip(starts[:-1], starts[1:]):
            bounds[s:e] = (s, e)
        tables = {k: torch.from_numpy(v).to(device) for k, v in host.items()}
        return cls(tables, torch.from_numpy(bounds).to(device), obs_keys, dataset_keys, frame_stack, seq_length, [0], [int(starts[-1])], [1.0],
                   len(episodes), env_meta)

    @classmethod
    def from_files(cls, hdf5_path: str, latent_path: Optional[str], obs_keys: Sequence[str], dataset_keys: Sequence[str] = ("actions",),
                   frame_stack: int = 1, seq_length: int = 1, n_overfit=None, optimal=1, append_last: bool = True, device=None) -> "DeviceDataset":
        """The weld of RobomimicLatentDataset (append_last=True: every episode has num_samples + 1 rows -- low-dim / image keys get the last
        `next_obs` row, `actions` its last row again) or ALOHASimLatentDataset (False: T rows).  `latent_<cam>` keys come from
        `data/<ep>/latent/<cam>` of the latent file; both files may be .hdf5 (hdf5_io.File: HDF5Unavailable without a libhdf5) or the .npz
        container of preencode.save_latents (dataset paths as keys).  n_overfit: None, an int (the first n after the sort) or a list of names."""
        src = _Container(os.path.expanduser(hdf5_path))
        lat = _Container(os.path.expanduser(latent_path)) if latent_path else None
        try:
            demos = demo_order(src.children("data"))
            if isinstance(n_overfit, (int, np.integer)) and not isinstance(n_overfit, bool):
                if n_overfit > len(demos):
                    raise ValueError(f"n_overfit = {n_overfit} but the file has {len(demos)} episodes")
                demos = demos[:int(n_overfit)]
            elif n_overfit is not None:
                chosen = set(str(d) for d in n_overfit)
                demos = [d for d in demos if d in chosen]
            episodes = []
            for ep in demos:
                actions = src.read(f"data/{ep}/actions")
                rows: Dict[str, np.ndarray] = {"actions": np.concatenate([actions, actions[-1:]], 0) if append_last else actions}
                for k in tuple(dataset_keys) + tuple(obs_keys):
                    if k in rows or k == "optimal":
                        continue
                    if "latent" in k:
                        if lat is None:
                            raise ValueError(f"key {k!r} needs a latent file")
                        rows[k] = lat.read(f"data/{ep}/latent/{k.replace('latent_', '')}")
                    else:
                        a = src.read(f"data/{ep}/obs/{k}")
                        rows[k] = np.concatenate([a, src.read(f"data/{ep}/next_obs/{k}")[-1:]], 0) if append_last else a
                episodes.append(rows)
            env_meta = src.env_args()
        finally:
            src.close()
            if lat is not None:
                lat.close()
        return cls.from_episodes(episodes, obs_keys, dataset_keys, frame_stack, seq_length, optimal, device, env_meta)

    @classmethod
    def mix(cls, datasets: Sequence["DeviceDataset"], split) -> "DeviceDataset":
        """A mixture (RobomimicMixedLatentData._sample): every sample first picks dataset d with probability split[d], then an index in it.
        The datasets' tables are welded one behind the other on the device, so a mixed batch is still one launch."""
        ds = list(datasets)
        split = _as_split(split, len(ds))
        d0 = ds[0]
        for d in ds:
            if d._n_sets != 1:
                raise ValueError("mix takes single datasets, not mixtures")
            if (d.obs_keys, d.dataset_keys, d.frame_stack, d.seq_length) != (d0.obs_keys, d0.dataset_keys, d0.frame_stack, d0.seq_length):
                raise ValueError("mixed datasets must share keys, frame_stack and seq_length")
            for k in d0.tables:
                if d.tables[k].shape[1:] != d0.tables[k].shape[1:] or d.tables[k].dtype != d0.tables[k].dtype:
                    raise ValueError(f"key {k!r}: row shape / dtype differ between the mixed datasets")
        base = np.concatenate([[0], np.cumsum([d.total_n_sequences for d in ds])])
        tables = {k: torch.cat([d.tables[k] for d in ds], dim=0) for k in d0.tables}
        bounds = torch.cat([d.bounds + int(b) for d, b in zip(ds, base[:-1])], dim=0)
        if d0.device.type == "cuda":                                # construction: the welded tables are complete before any stream samples them
            torch.cuda.current_stream(d0.device).synchronize()
        return cls(tables, bounds, d0.obs_keys, d0.dataset_keys, d0.frame_stack, d0.seq_length, base[:-1], [d.total_n_sequences for d in ds], split,
                   sum(d.n_demos for d in ds), d0.env_meta)

    # ---- sampling ----------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _row_bytes(t: torch.Tensor) -> int:
        return int(np.prod(t.shape[1:], dtype=np.int64)) * t.element_size()

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def draw(self, batch_size: int, seed: int, step: int, row_offset: int = 0) -> torch.Tensor:
        """The (B,) int64 welded-row indices `sample(batch_size, seed, step, row_offset)` uses, on the device: what a rank logs or replays."""
        out = torch.empty((int(batch_size),), dtype=torch.int64, device=self.device)
        _lib.check(_lib.load().ldp_data_draw(self._base, self._total, self._thr, self._n_sets, C.c_uint64(int(seed) & (2**64 - 1)),
                                             C.c_int64(int(row_offset)), C.c_uint32(int(step) & 0xFFFFFFFF), int(batch_size), out.data_ptr(),
                                             self._stream()))
        return out

    def sample(self, batch_size: int, seed: int, step: int, row_offset: int = 0, indices=None, index_out: Optional[torch.Tensor] = None) -> dict:
        """-> {'obs': {key: (B, W, ...)}, 'actions': (B, seq_length, A)} of device tensors, W = frame_stack + seq_length - 1: sample b is the
        window around welded row Philox(seed, row_offset + b, step) -- or around indices[b] (clamped into the table) when `indices` is given.
        One launch on the CURRENT stream, no host synchronisation, no H2D copy (an explicit host `indices` apart).  `index_out`: an optional
        (B,) int64 device tensor that receives the welded rows used (what `draw` returns), written by the same launch.

        Stream contract: the outputs belong to the calling stream.  A consumer on another stream waits for it first (an event, or
        `other.wait_stream(this)`), as for any tensor PyTorch produces."""
        B = int(batch_size)
        idx = None
        if indices is not None:
            idx = torch.as_tensor(indices).to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()
            if idx.shape[0] != B:
                raise ValueError(f"{idx.shape[0]} indices for a batch of {B}")
        if index_out is not None and (index_out.dtype != torch.int64 or index_out.device != self.device or tuple(index_out.shape) != (B,)
                                      or not index_out.is_contiguous()):
            raise ValueError(f"index_out must be a contiguous ({B},) int64 tensor on {self.device}")
        fs, sl = self.frame_stack, self.seq_length
        keys = (_lib.LdpDataKey * len(self.tables))()
        outs = {}
        for d, (k, t) in zip(keys, self.tables.items()):
            first, rows = (fs - 1, sl) if k in self.dataset_keys else (0, fs + sl - 1)
            o = torch.empty((max(B, 0), rows) + tuple(t.shape[1:]), dtype=t.dtype, device=self.device)
            d.table, d.out, d.row_bytes, d.first_row, d.n_rows = t.data_ptr(), o.data_ptr(), self._row_bytes(t), first, rows
            outs[k] = o
        _lib.check(_lib.load().ldp_data_sample(keys, len(self.tables), self.bounds.data_ptr(), self.total_n_sequences, self._base, self._total,
                                               self._thr, self._n_sets, C.c_uint64(int(seed) & (2**64 - 1)), C.c_int64(int(row_offset)),
                                               C.c_uint32(int(step) & 0xFFFFFFFF), B, fs, sl, None if idx is None else idx.data_ptr(),
                                               None if index_out is None else index_out.data_ptr(),
                                               self._stream()))
        batch = {k: outs[k] for k in self.dataset_keys}
        batch["obs"] = {k: outs[k] for k in self.obs_keys}
        return batch

    def batches(self, batch_size: int, seed: int = 0) -> "BatchIterator":
        return BatchIterator(self, batch_size, seed)


class BatchIterator:
    """Endless iterator of device batches: batch n is `dataset.sample(batch_size, seed, step = n)`.  Stands where the reference's
    DataLoader does (`.dataset` included: train_bc.py:172 reads `train_dataloader.dataset.env_meta`)."""

    def __init__(self, dataset: DeviceDataset, batch_size: int, seed: int = 0):
        self.dataset, self.batch_size, self.seed, self.step = dataset, int(batch_size), int(seed), 0

    def __iter__(self) -> Iterator[dict]:
        return self

    def __next__(self) -> dict:
        batch = self.dataset.sample(self.batch_size, self.seed, self.step)
        self.step += 1
        return batch


class _Container:
    """Read side of the two file kinds `from_files` takes: an HDF5 file through hdf5_io.File, or an .npz whose keys are dataset paths
    (`data/<ep>/...`, attributes as `data.attrs/<name>`: what preencode.save_latents writes)."""

    def __init__(self, path: str):
        self.npz = self.h5 = None
        if path.endswith(".npz"):
            self.npz = np.load(path, allow_pickle=False)
        else:
            from .hdf5_io import File
            self.h5 = File(path, "r")                   # raises HDF5Unavailable when no libhdf5 can be loaded

    def children(self, group: str) -> List[str]:
        if self.h5 is not None:
            return self.h5.keys(group)
        pre = group.strip("/") + "/"
        return sorted({k[len(pre):].split("/")[0] for k in self.npz.files if k.startswith(pre)})

    def read(self, name: str) -> np.ndarray:
        return self.h5.read_dataset_raw(name) if self.h5 is not None else self.npz[name]

    def env_args(self) -> Optional[dict]:
        """robomimic's `env_args` JSON of the `data` group, when there is one and it can be read."""
        try:
            if self.h5 is not None:
                return json.loads(self.h5.read_attr_str("data", "env_args"))
            return json.loads(str(self.npz["data.attrs/env_args"])) if "data.attrs/env_args" in self.npz.files else None
        except Exception:                                                  # noqa: BLE001
            return None

    def close(self):
        if self.h5 is not None:
            self.h5.close()
        if self.npz is not None:
            self.npz.close()


def _get(cfg, key, default=None):
    if isinstance(cfg, Mapping):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def _plain(cfg):
    """An OmegaConf node -> plain containers (the reference: OmegaConf.to_container(env_params, resolve=True)); anything else as it is."""
    try:
        from omegaconf import OmegaConf
        if OmegaConf.is_config(cfg):
            return OmegaConf.to_container(cfg, resolve=True)
    except ImportError:
        pass
    return cfg


def _overfit(n):
    n = _plain(n)
    return list(n) if isinstance(n, (list, tuple)) else n


class _LatentData:
    """What the three data classes share: the reference's constructor keywords (data/robomimic_latent_data.py:222-245), lazily built
    device datasets and endless device-batch iterators.  `n_workers` / `prefetch_factor` are accepted and unused: there are no workers."""
    append_last = True

    def __init__(self, name, train_path, eval_path, train_latent_path, eval_latent_path, train_n_episode_overfit, eval_n_episode_overfit,
                 batch_size, n_workers=0, prefetch_factor=None, obs_horizon=1, seq_length=1, env_params=None, meta=None, hdf5_use_swmr=True,
                 seed: int = 0, device=None):
        self.name, self.batch_size, self.obs_horizon, self.seq_length = name, int(batch_size), int(obs_horizon), int(seq_length)
        self.train_path, self.eval_path = train_path, eval_path
        self.train_latent_path, self.eval_latent_path = train_latent_path, eval_latent_path
        self.train_n_episode_overfit, self.eval_n_episode_overfit = train_n_episode_overfit, eval_n_episode_overfit
        self.n_workers, self.prefetch_factor, self.seed, self.device = n_workers, prefetch_factor, int(seed), device
        self.meta, self.env_params, self.shape_meta = meta, _plain(env_params), _get(meta, "shape_meta")
        self.obs_keys = list(_get(meta, "lowdim_obs", [])) + list(_get(meta, "rgb_obs", []))
        self._train_dataset = self._val_dataset = None

    def _load(self, path, latent_path, n_overfit, optimal=1) -> DeviceDataset:
        return DeviceDataset.from_files(path, latent_path, self.obs_keys, ("actions",), self.obs_horizon, self.seq_length, _overfit(n_overfit),
                                        optimal, self.append_last, self.device)

    @property
    def train_dataset(self) -> DeviceDataset:
        if self._train_dataset is None:
            self._train_dataset = self._load(self.train_path, self.train_latent_path, self.train_n_episode_overfit)
        return self._train_dataset

    @property
    def val_dataset(self) -> DeviceDataset:
        if self._val_dataset is None:
            self._val_dataset = self._load(self.eval_path, self.eval_latent_path, self.eval_n_episode_overfit)
        return self._val_dataset

    def train_dataloader(self) -> BatchIterator:
        return self.train_dataset.batches(self.batch_size, self.seed)

    def eval_dataloader(self) -> BatchIterator:
        return self.val_dataset.batches(self.batch_size, self.seed + 1)


class RobomimicLatentData(_LatentData):
    """data/robomimic_latent_data.py `RobomimicData`: episodes of num_samples + 1 rows."""


class ALOHASimLatentData(_LatentData):
    """data/alohasim_latent_data.py `ALOHASimData`: episodes of T rows, nothing appended."""
    append_last = False


class RobomimicMixedLatentData(_LatentData):
    """data/robomimic_mixed_latent_data.py: one dataset per entry of `train_paths`, mixed by `train_split` (a float s: [s, 1 - s]);
    `optimal` is 1 for the first dataset and 0 for the others.  The evaluation set is the first of `eval_paths` (or of `train_paths`),
    `optimal` 0, ten episodes unless `eval_n_episode_overfit` is a list whose first entry says otherwise (:92-113)."""

    def __init__(self, name, train_paths, eval_paths, train_latent_paths, eval_latent_paths, batch_size, n_workers=0, prefetch_factor=None,
                 train_n_episode_overfit=None, eval_n_episode_overfit=None, train_split=0.5, eval_split=0.5, obs_horizon=1, seq_length=1,
                 env_params=None, meta=None, seed: int = 0, device=None):
        super().__init__(name, None, None, None, None, train_n_episode_overfit, eval_n_episode_overfit, batch_size, n_workers, prefetch_factor,
                         obs_horizon, seq_length, env_params, meta, True, seed, device)
        self.train_paths, self.eval_paths = list(_plain(train_paths)), _plain(eval_paths)
        self.train_latent_paths, self.eval_latent_paths = list(_plain(train_latent_paths)), _plain(eval_latent_paths)
        over = _plain(train_n_episode_overfit)
        self.train_n_episode_overfit = list(over) if over is not None else [None] * len(self.train_paths)
        if len(self.train_n_episode_overfit) != len(self.train_paths):
            raise ValueError("train_n_episode_overfit needs one entry per train path")
        self.train_split = _as_split(_plain(train_split), len(self.train_paths))
        self.eval_split = _plain(eval_split)

    @property
    def train_dataset(self) -> DeviceDataset:
        if self._train_dataset is None:
            parts = [self._load(p, lp, n, optimal=int(i == 0))
                     for i, (p, lp, n) in enumerate(zip(self.train_paths, self.train_latent_paths, self.train_n_episode_overfit))]
            self._train_dataset = DeviceDataset.mix(parts, self.train_split)
        return self._train_dataset

    @property
    def val_dataset(self) -> DeviceDataset:
        if self._val_dataset is None:
            first = lambda v, alt: (v[0] if len(v) else alt) if isinstance(v, (list, tuple)) else v      # noqa: E731
            n = _plain(self.eval_n_episode_overfit)
            n = n[0] if isinstance(n, (list, tuple)) and len(n) else 10
            self._val_dataset = self._load(first(self.eval_paths, self.train_paths[0]), first(self.eval_latent_paths, self.train_latent_paths[0]),
                                           n, optimal=0)
        return self._val_dataset
