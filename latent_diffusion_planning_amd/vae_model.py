"""StableVAEModel -- the reference's VAE model class (model/stable_vae_model.py:18-175) on the HIP engine.

`create`, `.vae_state` (`.params`, `.ema_params`, `.step`, `.replace`), `.config[...]`, `.obs_normalization`, `.replace`, `get_params`,
`get_metrics`, `reconstruct`, `sample` and `update` have the reference's names, argument meaning and return structure: what `train_vae.py`
calls.  `update` runs the loss, its hand-written backward pass (csrc/vae_train.hpp: exact-fp32 2-D convolutions, GroupNorm, attention),
Adam and the EMA on the engine's VAE arena (module bit 4 of the training calls); the new model's `params` / `ema_params` are fetched from
the arenas on first access, and only the newest model's are readable (the reference donates the old state's buffers the same way).
Training is built for 64-pixel frames, the reference's `init` shape; `update` refuses other sizes.

Deliberate differences, the same as for the agents (agent.py):
  * `rng`: an int seed, a uint32[2] key or a torch.Generator seeds the in-kernel Philox stream (JAX's threefry stream is a non-goal);
    `noise=` gives the explicit-noise parity mode (`get_metrics`: the eps of the posterior draw; `sample`: the four latents).
  * metrics are device-resident scalars that read like the reference's 0-d arrays (`float(m["loss"])`, `np.mean([...])`); images are
    `arrays.DeviceArray`s.
  * `get_metrics` concatenates the cameras of `rgb_obs` on the batch axis like the reference (:28), so more than one camera works here.
  * `params` and `ema_params` are two weight sets for ONE engine slot: each has a version token and is uploaded only when the slot holds
    something else (a loop of `get_metrics` calls uploads nothing; a `reconstruct` in between swaps the EMA in and back).
"""
from __future__ import annotations

import copy
from typing import Optional

import numpy as np
import torch

from . import _lib
from . import weights as W
from .agent import DPState, _Elem, _EngineCalls, _get, _norm_entry, _philox_normal, _seed_of
from .arrays import DeviceArray
from .engine import HipEngine

IMAGE_SIZES = (64, 96, 128)               # what the 3x3 conv tiles of csrc/vae.hip are built for (latent side 2 / 3 / 4)
LATENT_CHANNELS = (4, 8)
PHILOX_STREAM_VAE_SAMPLE = 10             # the four latents of sample(): a stream of its own (include/ldp_hip.h lists them)
SAMPLE_COUNT = 4                          # model/stable_vae_model.py:112


def _check_vae_cfg(vae) -> W.VAESpec:
    """The `vae:` mapping of model/stable_vae_model.yaml:4-16 against what the engine builds; anything else is refused with the reason."""
    ref = W.VAESpec()
    n = len(ref.block_out_channels)
    down = list(_get(vae, "down_block_types", ["DownEncoderBlock2D"] * n))
    up = list(_get(vae, "up_block_types", ["UpDecoderBlock2D"] * n))
    if len(down) != n or any(str(b) != "DownEncoderBlock2D" for b in down):
        raise NotImplementedError(f"vae.down_block_types={down}: the engine builds {n} DownEncoderBlock2D stages (n_downsample = {n})")
    if len(up) != n or any(str(b) != "UpDecoderBlock2D" for b in up):
        raise NotImplementedError(f"vae.up_block_types={up}: the engine builds {n} UpDecoderBlock2D stages")
    ch = tuple(int(c) for c in _get(vae, "block_out_channels", ref.block_out_channels))
    if ch != ref.block_out_channels:
        raise NotImplementedError(f"vae.block_out_channels={ch}: the engine builds {ref.block_out_channels}")
    for key, want in (("layers_per_block", ref.layers_per_block), ("norm_num_groups", ref.norm_num_groups),
                      ("in_channels", ref.in_channels), ("out_channels", ref.out_channels)):
        got = int(_get(vae, key, want))
        if got != want:
            raise NotImplementedError(f"vae.{key}={got}: the engine builds {want}")
    act = str(_get(vae, "act_fn", "silu"))
    if act not in ("silu", "swish"):
        raise NotImplementedError(f"vae.act_fn={act!r}: the GroupNorm kernels fuse silu")
    lc = int(_get(vae, "latent_channels", ref.latent_channels))
    if lc not in LATENT_CHANNELS:
        raise NotImplementedError(f"vae.latent_channels={lc}: built for {LATENT_CHANNELS}")
    return W.VAESpec(latent_channels=lc)


def merge_vae_metrics(vectors, frame_counts, use_kl, beta) -> torch.Tensor:
    """The eleven metrics (_lib.VAE_METRIC_KEYS order) of a batch from those of its parts: `vectors` one (11,) device tensor per part,
    `frame_counts` the parts' frames (ints, or a device tensor).  min / max: of the parts; means, loss_mse and loss_kl: weighted by frames
    (every frame has the same number of pixels and of latent entries); std: var = sum_i w_i (std_i^2 + (mean_i - mean)^2); loss =
    loss_mse + beta loss_kl (loss_mse without the KL term).  Float64 on the tensors' device, no host synchronisation -> (11,) float32."""
    v = [x.reshape(-1).double() for x in vectors]
    if torch.is_tensor(frame_counts):
        c = frame_counts.reshape(-1).to(device=v[0].device, dtype=torch.float64)
        w = list(c / c.sum())
    else:
        total = float(sum(frame_counts))
        w = [float(c) / total for c in frame_counts]
    K = {k: i for i, k in enumerate(_lib.VAE_METRIC_KEYS)}
    out = sum(wi * x for wi, x in zip(w, v))                                    # the weighted means; the other entries are replaced below
    both = torch.stack(v)
    for k in ("img", "z"):
        out[K[k + "_min"]] = both[:, K[k + "_min"]].min()
        out[K[k + "_max"]] = both[:, K[k + "_max"]].max()
        s, m = K[k + "_std"], K[k + "_mean"]
        out[s] = sum(wi * (x[s] * x[s] + (x[m] - out[m]) ** 2) for wi, x in zip(w, v)).sqrt()
    out[K["loss"]] = out[K["loss_mse"]] + float(beta) * out[K["loss_kl"]] if use_kl else out[K["loss_mse"]]
    return out.float()


class StableVAEModel(_EngineCalls):
    def __init__(self, vae_state: DPState, obs_normalization, config, engine: Optional[HipEngine], vae_spec: W.VAESpec, image_size: int,
                 device, lr_schedule=None, ema_decay: float = 0.99):
        self.vae_state = vae_state
        self.ema_decay = float(ema_decay)            # TrainStateEMA.apply_ema (update)
        self.obs_normalization = obs_normalization
        self.config = config
        self.lr_schedule = lr_schedule
        self._engine = engine
        self._vae_spec = vae_spec
        self._image_size = int(image_size)
        self._device = device
        self._uploads = [0]                   # weight uploads of this model and its .replace copies (they share the engine)

    # ---------------------------------------------------------------------------------------------
    @classmethod
    def create(cls, rng, batch, shape_meta, *,
               # Hydra config (model/stable_vae_model.yaml)
               name, vae, rgb_obs, obs_normalization,
               lr, end_lr, warmup_steps, decay_steps, ema_decay,
               use_kl, beta, data_name, device=None, exclusive_gpu=True):
        """model/stable_vae_model.py:128-175.  `batch` is accepted for signature parity; the frame size comes from `shape_meta`
        (64 when it does not list the cameras, the reference's `jnp.zeros((2, 3, 64, 64))` of :139)."""
        rgb_obs = list(rgb_obs)
        if not rgb_obs:
            raise ValueError("rgb_obs is empty: the VAE trains on at least one camera")
        spec = _check_vae_cfg(vae)
        sizes = set()
        for k in rgb_obs:
            shp = (shape_meta or {}).get("all_shapes", {}).get(k)
            if shp is None:
                continue
            shp = tuple(int(v) for v in shp)
            if len(shp) != 3 or shp[0] != shp[1] or shp[2] != 3:
                raise NotImplementedError(f"image key {k!r} has shape {shp}: the StableVAE takes square (S, S, 3) frames")
            sizes.add(shp[0])
        if len(sizes) > 1:
            raise NotImplementedError(f"rgb_obs cameras of different sizes {sorted(sizes)}: they are concatenated on the batch axis")
        image_size = sizes.pop() if sizes else 64
        if image_size not in IMAGE_SIZES:
            raise NotImplementedError(f"{image_size}-pixel frames: the 3x3 conv tiles are built for {IMAGE_SIZES} pixel squares")
        decay = float(ema_decay)
        if not 0.0 <= decay <= 1.0:
            raise ValueError(f"ema_decay={decay} must lie in [0, 1]")
        if not np.isfinite(float(beta)):
            raise ValueError(f"beta={beta} must be finite")
        seed = _seed_of(rng)
        params = W.init_vae_params(spec, seed=seed * 3 + 1, perturb=False)
        state = DPState(params, None, ema_is_params=True)                     # TrainStateEMA.create(..., ema_params=params) (:157-163)
        from .schedule import warmup_cosine_decay_schedule
        sched = warmup_cosine_decay_schedule(float(end_lr), float(lr), int(warmup_steps), int(decay_steps), float(end_lr))   # :144-150
        config = dict(rgb_obs=rgb_obs, name=name, use_kl=use_kl, beta=beta, n_downsample=len(spec.block_out_channels),
                      data_name=data_name)                                     # :166-169, the reference's six keys
        norm = {"obs": {k: _norm_entry(v) for k, v in dict(obs_normalization["obs"]).items()}}
        if "actions" in obs_normalization:
            norm["actions"] = _norm_entry(obs_normalization["actions"])
        missing = [k for k in rgb_obs if k not in norm["obs"]]
        if missing:
            raise KeyError(f"obs_normalization has no entry for the camera(s) {missing}")
        if not torch.cuda.is_available():
            raise _lib.LDPHipUnavailable("no HIP device visible: StableVAEModel has no CPU fallback")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        # the handle's planner / IDM slots stay empty: the smallest shapes the library accepts
        engine = HipEngine(obs_dim=25, action_dim=7, global_cond_dim=25, pred_horizon=8, action_horizon=4, image_size=image_size,
                           vae_latent_channels=spec.latent_channels, device=dev)
        if not exclusive_gpu:
            engine.set_option("safe_mode", 1)
        return cls(state, norm, config, engine, spec, image_size, dev, lr_schedule=sched, ema_decay=decay)

    # ---------------------------------------------------------------------------------------------
    def replace(self, **fields):
        """flax.struct `.replace`: a shallow copy sharing the engine (weights re-upload lazily, by version token)."""
        new = copy.copy(self)
        for k, v in fields.items():
            if k not in ("vae_state", "obs_normalization", "config", "lr_schedule"):
                raise AttributeError(f"StableVAEModel has no field {k!r}")
            setattr(new, k, v)
        return new

    def get_params(self):
        """model/stable_vae_model.py:125-126: the names train_vae.py saves and load_pretrained_vae looks for."""
        return dict(vae_params=self.vae_state.params, ema_params=self.vae_state.ema_params)

    @property
    def uploads(self) -> int:
        """How many times this model (or a .replace copy) put a weight set into the engine."""
        return self._uploads[0]

    _ema_decay = property(lambda self: self.ema_decay)

    def _sync_weights(self, use_ema: bool) -> None:
        """The engine's VAE slot must hold `params` (get_metrics) or `ema_params` (reconstruct, sample): each set has its own token."""
        st, eng = self.vae_state, self._engine
        want = st.ema_version if use_ema else st.version
        if eng.loaded["vae"] == want:
            return
        tree = self._slot_weights(eng, "vae", st, self._shapes, use_ema)          # None: published from the training arena
        if tree is not None:
            eng.load_params(vae=tree, versions={"vae": want})
        self._uploads[0] += 1

    def _shapes(self):
        return W.vae_shapes(self._vae_spec)

    def _train_sync(self, st: DPState) -> None:
        """The shared hand-off for the model's one slot: the VAE arenas must hold THIS state (tests and tools warm the arenas through it)."""
        super()._train_sync("vae", st, self._shapes())

    # ---- model/stable_vae_model.py:28 after postprocess_batch (utils/data_utils.py:70-80) ------------------------------------------
    def _frames(self, batch, keys) -> torch.Tensor:
        """Frame 0 of every key, normalised with the camera's own bounds, concatenated on the BATCH axis -> (len(keys) * B, S, S, 3) NHWC
        (the reference transposes to NCHW for Flax's wrapper, which transposes back)."""
        obs = batch["obs"]
        table = self.obs_normalization["obs"]
        assert set(obs.keys()).issubset(table), f"obs_normalization keys {table.keys()} do not match batch keys {obs.keys()}"
        S = self._image_size
        out = []
        for k in keys:
            v = self._t(obs[k])
            if v.dim() != 5 or tuple(v.shape[2:]) != (S, S, 3):
                raise ValueError(f"batch['obs'][{k!r}] must have shape (B, H, {S}, {S}, 3), got {tuple(v.shape)}")
            out.append(self._apply_norm(v[:, 0].contiguous(), table[k], True))
        return out[0] if len(out) == 1 else torch.cat(out, dim=0).contiguous()

    # ---- model/stable_vae_model.py:25-55, 75-87 ---------------------------------------------------------------------------------------
    def get_metrics(self, batch, rng, noise=None, row_offset: int = 0):
        """`get_metrics_step` on `params`: ONE ldp_vae_metrics call -> the eleven keys of `loss` (img_min / max / mean / std, loss, loss_mse,
        loss_kl, z_min / max / mean / std).  noise: optional eps (frames, S/32, S/32, LC) of the posterior draw for parity runs;
        row_offset: global index of the first frame (the Philox eps of a frame does not depend on how a batch is sharded)."""
        seed = _seed_of(rng)
        use_kl, beta = bool(self.config["use_kl"]), float(self.config["beta"])
        eps = None if noise is None else self._t(noise)

        def run():
            self._sync_weights(use_ema=False)
            img = self._frames(batch, self.config["rgb_obs"])
            return [self._engine.vae_metrics(img, use_kl, beta, seed=seed, noise=eps, row_offset=row_offset)[0]]
        res, rec = self._call(run)
        vec = DeviceArray(res[0], record=rec)
        return {k: _Elem(vec, i) for i, k in enumerate(_lib.VAE_METRIC_KEYS)}

    # ---- model/stable_vae_model.py:89-101 --------------------------------------------------------------------------------------------
    def reconstruct(self, batch, rng, rgb_key):
        """decode(encode(frame 0 of `rgb_key`).latent_dist.mode()) on `ema_params` -> (B, 3, S, S).  The mode of the diagonal Gaussian is
        its mean, which is what vae_encode returns; `rng` is unused, as in the reference."""
        if rgb_key not in batch["obs"]:
            raise KeyError(f"batch['obs'] has no {rgb_key!r}")

        def run():
            self._sync_weights(use_ema=True)
            img = self._frames(batch, [rgb_key])
            return [self._engine.vae_decode(self._engine.vae_encode(img))]
        res, rec = self._call(run)
        return DeviceArray(res[0], record=rec)

    # ---- model/stable_vae_model.py:103-123 -------------------------------------------------------------------------------------------
    def sample(self, rng, noise=None):
        """decode of four N(0, I) latents (4, 2, 2, LC) on `ema_params` -> (4, 3, 64, 64): the `n_downsample == 6` branch (z_dim = 2).
        noise: the latents themselves, for parity runs."""
        if self.config["n_downsample"] != 6:
            raise NotImplementedError                                            # :110-111
        if self._image_size != 64:
            raise NotImplementedError(f"sample(): the reference draws (4, 2, 2, LC) latents for n_downsample == 6, i.e. 64-pixel frames; this "
                                      f"model was built for {self._image_size}-pixel frames, whose latent side is {self._image_size // 32}")
        seed = _seed_of(rng)
        shape = (SAMPLE_COUNT, 2, 2, self._vae_spec.latent_channels)
        z_in = None if noise is None else self._t(noise)
        if z_in is not None and tuple(z_in.shape) != shape:
            raise ValueError(f"noise must have shape {shape}, got {tuple(z_in.shape)}")

        def run():
            self._sync_weights(use_ema=True)
            z = z_in if z_in is not None else _philox_normal(seed, 0, 0, PHILOX_STREAM_VAE_SAMPLE, int(np.prod(shape)),
                                                             self._device).reshape(shape)
            return [self._engine.vae_decode(z)]
        res, rec = self._call(run)
        return DeviceArray(res[0], record=rec)

    # ---- model/stable_vae_model.py:57-73 ---------------------------------------------------------------------------------------------
    TRAIN_SIZES = (64,)                       # frame sizes the training tape is built and tested for

    def _gates(self, step):
        """update() trains the VAE on every step: (use_planner, use_idm) in the form dist.update_sharded asks every trainable class for."""
        return True, False

    def update(self, batch, rng, step, noise=None, row_offset: int = 0, chunk=None):
        """`update_step`: jax.grad of `loss` on `params`, one optax.adam step with the warmup-cosine schedule, then the EMA -> (new model,
        metrics).  metrics: the eleven keys of `loss` on the pre-update parameters (device scalars, as get_metrics), then vae_lr =
        schedule(old step) and vae_step = old step.  rng / noise / row_offset: the eps of the posterior draw, as get_metrics (the same seed draws
        the same eps here and there).  `step` is unused, as in the reference.
        chunk: at most this many frames per gradient call (1 .. 256, default 256).  A batch of more frames is differentiated part by part
        into the same gradient arena (ldp_train_vae_grad_part): one Adam step on the whole batch's gradient at the activation memory of
        `chunk` frames; the metrics are those of the whole batch (merge_vae_metrics)."""
        return self._update_step(batch, None, rng, True, False, noise, row_offset=row_offset, chunk=chunk)

    def _parts(self, n_local: int, n_cams: int, rows, row_offset: int, chunk: int):
        """The ONE rule that cuts a step's frames into gradient calls -> [(first local frame, frames, first global index)].  This process's
        frames in `_frames` order (cameras concatenated on the batch axis); frame b of camera `cam` has the global index
        row_offset + cam * n_rows_global + first_row + b.  A new part starts where the index is not the previous one plus 1, or when the
        part holds `chunk` frames."""
        lo, n = rows
        parts, prev = [], None
        for cam in range(n_cams):
            for b in range(n_local):
                g = row_offset + cam * n + lo + b
                if prev is None or g != prev + 1 or parts[-1][1] == chunk:
                    parts.append([cam * n_local + b, 0, g])
                parts[-1][1] += 1
                prev = g
        return [tuple(p) for p in parts]

    def _update_step(self, batch, mixed_batch, rng, use_planner, use_idm, noise, shard=None, row_offset: int = 0, chunk=None):
        """shard (dist.update_sharded): dict(group, rows=(lo, n)) -- `batch` holds rows [lo, lo + B) of a global batch of n rows per camera.
        Every camera's rows are one run of global frames (cam * n + lo ...), each differentiated with the weight frames / (cameras * n);
        ONE all-reduce of the gradient arena after the last part, Adam and the EMA replicated; the metrics are those of the GLOBAL batch
        on every rank (one all_gather of 12 floats per rank, merged in rank order).  noise: eps of the global frames or of exactly the
        local ones."""
        if mixed_batch is not None or use_idm:
            raise NotImplementedError("StableVAEModel trains one network on one batch")
        eng = self._engine
        if not hasattr(eng, "train_vae_grad"):
            raise NotImplementedError("StableVAEModel.update: this engine has no backward pass of the 2-D convolutions (HipEngine.train_vae_grad); "
                                      "train the VAE with a build that has it, or import a snapshot (checkpoint.load_snapshot)")
        if self._image_size not in self.TRAIN_SIZES:
            raise NotImplementedError(f"StableVAEModel.update: the backward pass of the 2-D convolutions is built for {self.TRAIN_SIZES}-pixel frames; "
                                      f"this model takes {self._image_size}-pixel frames")
        if self.lr_schedule is None:
            raise ValueError("update() needs the optimiser settings of StableVAEModel.create (lr, end_lr, warmup_steps, decay_steps)")
        chunk = _lib.VAE_TRAIN_MAX_FRAMES if chunk is None else int(chunk)
        if not 1 <= chunk <= _lib.VAE_TRAIN_MAX_FRAMES:
            raise ValueError(f"chunk={chunk}: a gradient call takes 1 to {_lib.VAE_TRAIN_MAX_FRAMES} frames")
        seed = _seed_of(rng)
        use_kl, beta = bool(self.config["use_kl"]), float(self.config["beta"])
        eps = None if noise is None else self._t(noise)
        st = self.vae_state
        lr = np.float32(self.lr_schedule(st.step))
        shapes = self._shapes()
        n_cams = len(self.config["rgb_obs"])

        def run():
            self._train_sync(st)
            img = self._frames(batch, self.config["rgb_obs"])
            n_local = img.shape[0] // n_cams
            rows = (0, n_local) if shard is None else shard["rows"]
            n_total = n_cams * int(rows[1])
            parts = self._parts(n_local, n_cams, rows, int(row_offset), chunk)
            if eps is not None and eps.shape[0] not in (n_total, img.shape[0]):
                raise ValueError(f"noise holds {eps.shape[0]} frames: give the eps of the {n_total} global frames or of the {img.shape[0]} local ones")
            is_global = eps is not None and eps.shape[0] == n_total

            def eps_of(first, cnt, g0):
                if eps is None:
                    return None
                a = g0 - int(row_offset) if is_global else first
                return eps[a:a + cnt]
            if len(parts) == 1 and parts[0][1] == n_total:                      # the whole batch in one call: the call it has always been
                out = eng.train_vae_grad(img, use_kl, beta, seed=seed, noise=eps, row_offset=parts[0][2])
            else:
                vecs = [eng.train_vae_grad_part(img[first:first + cnt], n_total, k > 0, use_kl, beta, seed=seed, noise=eps_of(first, cnt, g0),
                                                row_offset=g0) for k, (first, cnt, g0) in enumerate(parts)]
                out = vecs[0] if len(vecs) == 1 else merge_vae_metrics(vecs, [p[1] for p in parts], use_kl, beta)
            if shard is not None:                                               # data parallel: the weighted shard gradients sum to the global batch's
                import torch.distributed as tdist
                group = shard.get("group")
                tdist.all_reduce(eng.train_arena("vae", eng.TRAIN_GRADS), group=group)
                mine = torch.cat([out.reshape(-1).float(), torch.full((1,), float(img.shape[0]), dtype=torch.float32, device=out.device)])
                every = [torch.empty_like(mine) for _ in range(tdist.get_world_size(group))]
                tdist.all_gather(every, mine, group=group)
                every = torch.stack(every)
                out = merge_vae_metrics(list(every[:, :-1]), every[:, -1], use_kl, beta)
            eng.train_apply("vae", float(lr))                                   # Adam + EMA, one launch
            return [out]
        # the tape runs on exact-fp32 kernels only (no range guard, no in-launch exchange): a later fault poll has nothing to recompute here,
        # and re-running the step would apply it twice
        res, rec = self._call(run, lambda: [None])
        new_state = self._trained_state("vae", st, shapes)
        vec = DeviceArray(res[0], record=rec)
        metrics = {k: _Elem(vec, i) for i, k in enumerate(_lib.VAE_METRIC_KEYS)}
        metrics["vae_lr"], metrics["vae_step"] = lr, st.step                  # the OLD state's count (:71-72)
        return self.replace(vae_state=new_state), metrics
