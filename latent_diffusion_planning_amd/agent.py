"""LDPAgent -- the reference's agent surface (agent/ldp_agent.py:28-672) on the HIP engine.

Drop-in for the *sampling* side of the reference class: `create`, `.config[...]`, `.replace`,
`.planner_state/.idm_state` (`.params`, `.replace(params=, ema_params=)`), `sample`,
`sample_viz`, `sample_action`, `sample_action_from_plan`, `vae_encode`, `vae_decode`,
`get_obs_cond`, `get_params`, `get_metrics` (the losses, forward only), `update`, `update_mixed` (the
training step: losses, gradients, global norm, optax.adam -- csrc/train.hip) -- same names, argument
meaning, return structure and error behaviour (e.g. the `assert len(batch.keys()) == 1` of
agent/ldp_agent.py:439).

Differences that are deliberate and documented:
  * `rng`: the reference takes a JAX PRNGKey; here an int seed, a uint32[2] key array or a
    torch.Generator is accepted and used as the seed of the in-kernel Philox stream.  JAX's
    threefry stream is not reproduced; `noise=` gives the explicit-noise parity mode.
  * inputs may be numpy arrays, torch tensors or DeviceArrays.  Outputs (`action`, every value of
    `metrics`) are `arrays.DeviceArray`s: device-resident (`.tensor`) and numpy-like on demand, so
    the reference's call sites run verbatim -- `np.array(batch_action)`, `batch_action[idx]`,
    `np.array(plan_viz)` (utils/rm_env_utils.py:186-196), `((plan_viz + 1) / 2 * 255).astype(np.uint8)
    .transpose(0, 1, 3, 4, 2)` (utils/aloha_env_utils.py:96), `np.mean(np.square(actions - pred))`
    (eval_bc.py:135-151), `float(stats['plan_mse'])`.
  * `metrics['plan_viz']` is always present; `sample()` leaves it lazy (decoded on first access),
    `sample_viz()` enqueues the decode right away like the reference (agent/ldp_agent.py:483).
  * all arithmetic runs in libldp_hip.so; there is no CPU path.
"""
from __future__ import annotations

import collections
import contextlib
import copy
import itertools
import warnings
from typing import Any, Dict, Mapping, Optional, Sequence

import numpy as np
import torch

from . import weights as W
from .arrays import CallRecord, DeviceArray, as_tensor
from .engine import HipEngine

_versions = itertools.count(1)        # tokens of parameter trees (never reused, unlike id())

# one diffusion network of an agent (LDPAgent._nets): where it lives and how one training step drives it
_Net = collections.namedtuple("_Net", "key eng slot shapes grad stream noise steps")

# vae_feature_dim -> (latent side, latent channels) as agent/ldp_agent.py:69-80 reshapes them; the image side is
# 32 x the latent side (five stride-2 stages): 64-pixel frames for 16 / 32, 96-pixel frames for 36 (3x3x4), 128 for 64.
LATENT_SHAPES = {16: (2, 4), 32: (2, 8), 36: (3, 4), 64: (4, 4)}


# ------------------------------------------------------------------------------------------------
# small stand-ins for flax_utils.TrainStateEMA (utils/flax_utils.py:18-27) as seen by the callers
# ------------------------------------------------------------------------------------------------
def _as_flat(params) -> Dict[str, np.ndarray]:
    if params is None:
        return None
    if any(isinstance(v, Mapping) for v in params.values()):
        return W.flatten(params)
    return {k: np.ascontiguousarray(np.asarray(v), dtype=np.float32) for k, v in params.items()}


class ParamState:
    """Stand-in for flax_utils.TrainStateEMA (utils/flax_utils.py:18-27) as the callers see it: `.params`, `.ema_params`, `.step`, `.opt_state`
    and the `.replace(...)` the reference's load_snapshot uses (train_bc.py:210-240, eval_bc.py:228).

    A state that came out of `LDPAgent.update` lives in the engine's training arenas (fp32 master parameters + the two Adam moments on the
    GPU); its `.params` / `.opt_state` are fetched on first access.  Like a jitted step with donated buffers, only the NEWEST state of a
    module is materialisable: reading a state that a later `update` superseded raises (keep `agent = agent.update(...)[0]` as the reference's
    training loop does, train_bc.py:107).

    version: token of `params` (fresh on every construction / .replace(params=...)): the engine records the token of what it holds, so two
    agents sharing one engine can never sample or train with each other's weights.  Like a flax pytree the dict is treated as immutable --
    publish changes with .replace."""

    def __init__(self, params=None, ema_params=None, step: int = 0, version: Optional[int] = None, opt_state=None, _fetch=None):
        self._params = params
        self.ema_params = ema_params
        self.step = int(step)
        self.version = next(_versions) if version is None else version
        self._opt_state = opt_state
        self._fetch = _fetch                  # (what) -> tree, for a state that lives in the engine

    @property
    def params(self):
        if self._params is None and self._fetch is not None:
            self._params = self._fetch("params")
        return self._params

    @property
    def opt_state(self):
        """{'mu': tree, 'nu': tree, 'count': step} (optax ScaleByAdamState) or None for a state that was never trained."""
        if self._opt_state is None and self._fetch is not None:
            self._opt_state = dict(mu=self._fetch("mu"), nu=self._fetch("nu"), count=self.step)
        return self._opt_state

    def replace(self, **kw):
        new = ParamState(self._params, self.ema_params, self.step, self.version, self._opt_state, self._fetch)
        if "params" in kw:
            new.version = kw.pop("version", next(_versions))
            new._params = _as_flat(kw.pop("params"))
            new._fetch = None
            new._opt_state = None if "opt_state" not in kw else new._opt_state      # new parameters start a new optimiser state unless one is given
        if "ema_params" in kw:
            e = kw.pop("ema_params")
            new.ema_params = _as_flat(e) if e is not None else None
        if "opt_state" in kw:
            o = kw.pop("opt_state")
            new._opt_state = None if o is None else dict(mu=_as_flat(o["mu"]), nu=_as_flat(o["nu"]), count=int(o.get("count", new.step)))
            new.version = next(_versions) if new._fetch is None else new.version
        if "step" in kw:
            new.step = int(kw.pop("step"))
        if "version" in kw:
            new.version = kw.pop("version")
        if kw:
            raise AttributeError(f"ParamState has no field(s) {sorted(kw)}")
        return new


class DPState(ParamState):
    """flax_utils.TrainStateEMA (utils/flax_utils.py:18-27) as DPVAEAgent's callers see it: ParamState plus an EMA tree with a version
    token of its own (`ema_version`), so the engine's single sampling slot always knows which of the two weight sets it holds.  The EMA
    of a trained state lives in the engine's EMA arena and is fetched on first access, like its parameters."""

    def __init__(self, params=None, ema_params=None, step: int = 0, version: Optional[int] = None, opt_state=None, _fetch=None,
                 ema_version: Optional[int] = None, _ema_fetch=None, ema_is_params: bool = False):
        self._ema = None
        super().__init__(params, ema_params, step, version, opt_state, _fetch)
        self.ema_version = next(_versions) if ema_version is None else ema_version
        self._ema_fetch = _ema_fetch
        # the EMA equals the parameters (TrainStateEMA.create, load_snapshot): restoring the state re-seeds the engine's EMA arena from them
        self.ema_is_params = bool(ema_is_params)

    @property
    def ema_params(self):
        if self._ema is None and self._ema_fetch is not None:
            self._ema = self._ema_fetch()
        if self._ema is None and self.ema_is_params:
            return self.params
        return self._ema

    @ema_params.setter
    def ema_params(self, value):
        self._ema = value

    def replace(self, **kw):
        new = DPState(self._params, None, self.step, self.version, self._opt_state, self._fetch, self.ema_version, self._ema_fetch,
                      self.ema_is_params)
        new._ema = self._ema
        same = "params" in kw and "ema_params" in kw and kw["ema_params"] is kw["params"]
        if "params" in kw and "ema_params" not in kw and self.ema_is_params:
            new._ema = self.params                      # the EMA stays what it was: the OLD parameters
        if "params" in kw:
            new.version = kw.pop("version", next(_versions))
            new._params = _as_flat(kw.pop("params"))
            new._fetch = None
            new._opt_state = None if "opt_state" not in kw else new._opt_state
            new.ema_is_params = False
        if "ema_params" in kw:
            e = kw.pop("ema_params")
            new.ema_version = kw.pop("ema_version", next(_versions))
            new._ema_fetch = None
            new._ema = None if same or e is None else _as_flat(e)
            new.ema_is_params = same
        if "opt_state" in kw:
            o = kw.pop("opt_state")
            new._opt_state = None if o is None else dict(mu=_as_flat(o["mu"]), nu=_as_flat(o["nu"]), count=int(o.get("count", new.step)))
            new.version = next(_versions) if new._fetch is None else new.version
        for k in ("step", "version", "ema_version"):
            if k in kw:
                setattr(new, k, int(kw.pop(k)) if k == "step" else kw.pop(k))
        if kw:
            raise AttributeError(f"DPState has no field(s) {sorted(kw)}")
        return new


def _philox_normal(seed, elem0, step, stream_id, n, device):
    from .engine import philox_normal
    return philox_normal(seed, elem0, step, stream_id, n, device)


class _HostScalar:
    """A metric scalar that lives on the device until somebody looks at it: float()-able and np.asarray-able like the jnp 0-d arrays of the
    reference's metrics dict (eval_bc.py:152: `float(np.mean([m[k] for m in all_metrics]))`).  `fn` reads DeviceArrays (the first read is the
    call's completion point: fault poll, recompute) and does whatever scalar arithmetic is left on the host -- nothing of get_metrics is
    computed by torch."""

    def __init__(self, fn):
        self._fn = fn
        self.shape, self.ndim, self.dtype = (), 0, np.dtype(np.float32)

    def __float__(self):
        return float(self._fn())

    def __array__(self, dtype=None, copy=None):
        a = np.asarray(self._fn(), dtype=np.float32)
        return a.astype(dtype) if dtype is not None else a

    def __repr__(self):
        return "_HostScalar(...)"


def _Elem(vec, i):
    return _HostScalar(lambda: vec.numpy()[i])


def _need_nets(agent, what: str) -> None:
    if not (agent.use_planner and agent.use_idm):
        raise NotImplementedError(f"{what}() needs both the planner and the IDM (use_planner / use_idm)")


def _seed_of(rng) -> int:
    if rng is None:
        return 0
    if isinstance(rng, torch.Generator):
        # a stateful generator: every call consumes one draw, so successive policy calls see fresh noise
        return int(torch.randint(0, 2**62, (1,), generator=rng, device=rng.device).item())
    if isinstance(rng, (int, np.integer)):
        return int(rng)
    a = np.asarray(rng)
    if a.shape == (2,):                                   # a JAX-style uint32[2] key
        return (int(a[0]) << 32) | int(a[1])
    if a.shape == ():
        return int(a)
    raise TypeError(f"rng must be an int seed, a uint32[2] key or a torch.Generator, got {type(rng)}")


def _get(cfg, key, default=None):
    if cfg is None:
        return default
    if isinstance(cfg, Mapping):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def _norm_entry(entry) -> dict:
    """obs_normalization leaf: {'min','max'} (scalars or vectors) or {'clip_min','clip_max'}."""
    e = dict(entry)
    if "mean" in e:
        raise NotImplementedError                        # utils/data_utils.py:31-32
    if "min" in e or "clip_min" in e:
        return {k: (float(v) if np.ndim(v) == 0 else np.asarray(v, dtype=np.float32)) for k, v in e.items()}
    raise NotImplementedError                            # utils/data_utils.py:66-67


def load_pretrained_vae(vp: str):
    """`vae_pretrain_path` -> the VAE parameter tree.  The containers this package added are recognised by their
    suffix first (.safetensors, .npz -- also when they sit under a '....ckpt/' directory); anything else with 'ckpt' in
    its path follows the reference's rule (agent/ldp_agent.py:543-551: an orbax checkpoint written by train_vae.py)."""
    if vp.endswith(".safetensors"):
        loaded = W.load_safetensors(vp)
    elif vp.endswith(".npz"):
        loaded = W.load_npz(vp)
    elif "ckpt" in vp:
        from . import checkpoint
        loaded = checkpoint.param_trees(checkpoint.restore(vp))
        if "vae_params" not in loaded:
            raise KeyError(f"{vp}: no vae_params tree in this checkpoint (has {sorted(loaded)})")
    else:
        loaded = W.load_npz(vp)
    return loaded.get("vae_params") or loaded.get("vae") or next(iter(loaded.values()))


class _EngineCalls:
    """What every model class on a HipEngine shares (LDPAgent and its subclasses, vae_model.StableVAEModel): tensors onto the device, the
    normalise kernel behind postprocess_batch, and the fault protocol of a policy call (_record / _guarded).  Needs `self._engine` and
    `self._device`."""

    # ---- pre/post-processing (utils/data_utils.py:18-80) ----------------------------------------
    def _t(self, v) -> torch.Tensor:
        v = as_tensor(v)
        return v.to(device=self._device, dtype=torch.float32).contiguous()

    def _apply_norm(self, v: torch.Tensor, entry: dict, normalize: bool) -> torch.Tensor:
        if "min" in entry:
            lo, hi = entry["min"], entry["max"]
            if np.ndim(lo) != 0:
                lo, hi = np.asarray(lo), np.asarray(hi)
                diff = v.dim() - lo.ndim
                assert diff in (0, 1, 2, 3, 4, 5), "shape length mismatch in normalize_obs"
                assert tuple(v.shape[diff:]) == tuple(lo.shape), \
                    f"shape mismatch in normalize obs. {tuple(v.shape)}, {lo.shape}"
                lo, hi = lo.reshape(-1), hi.reshape(-1)
                return self._engine.normalize_bounds(v.reshape(-1, lo.size), lo, hi, normalize).reshape(v.shape)
            return self._engine.normalize_bounds(v, [lo], [hi], normalize)
        # clip_min / clip_max: plain clip in both directions (utils/data_utils.py:61-65)
        return self._engine.normalize_bounds(v, [entry["clip_min"]], [entry["clip_max"]], 2)

    def _normalize_dict(self, d, table, normalize=True):
        assert set(d.keys()).issubset(table), \
            f"obs_normalization keys {table.keys()} do not match batch keys {d.keys()}"
        return {k: self._apply_norm(self._t(v), table[k], normalize) for k, v in d.items()}

    # ---- completion hook of a policy call (fault protocol, include/ldp_hip.h) --------------------------
    def _engines(self):
        """Every engine handle a policy call of this agent enqueues on (LDPHierAgent has two)."""
        return [self._engine]

    def _seqs(self):
        return tuple(e.call_seq for e in self._engines())

    def _record(self, recompute):
        """recompute() -> list of replacement tensors (None for lazy arrays), in the order the call's
        DeviceArrays were created."""
        engines = self._engines()

        def on_complete(rec: CallRecord):
            # calls are asynchronous: a recorded fault may stem from any call enqueued so far, so the poll marks
            # them all suspect (engine.fault_upto) and each is recomputed when ITS results are first read
            for e in engines:
                e.poll_fault_kinds()
            if not any(s <= e.fault_upto for s, e in zip(rec.seqs, engines)):
                return
            kinds = 0
            for s_, e in zip(rec.seqs, engines):               # the kind(s) of the poll that made THIS call suspect, not every kind the handle ever saw
                if s_ <= e.fault_upto:
                    kinds |= e.last_fault_kinds
            if kinds & HipEngine.FAULT_RANGE:
                warnings.warn("libldp_hip: an operand left the range of the two-fp16-plane convolutions (|x| >= 65504); the call "
                              "is recomputed on three bf16 planes (fp32 range; the IDM on its exact-fp32 kernel), which this engine keeps from now on",
                              RuntimeWarning, stacklevel=3)
            if kinds & HipEngine.FAULT_EXCHANGE:
                warnings.warn("libldp_hip: a split work-group timed out on its peer (GPU shared with another "
                              "kernel?); the call is recomputed in safe mode, which this engine keeps from now on",
                              RuntimeWarning, stacklevel=3)
            # a recompute may meet the OTHER kind of fault for the first time (safe mode first, then the range guard): bounded retries
            for attempt in range(3):
                fresh = self._guarded(recompute)
                torch.cuda.current_stream(self._device).synchronize()
                again = 0
                for e in engines:
                    again |= e.poll_fault_kinds()
                if not again:
                    break
            else:
                raise RuntimeError("libldp_hip faulted again after switching to safe mode / bf16 planes")
            for arr, t in zip(rec.arrays, fresh):
                if arr is not None:
                    arr._swap(t)
        return CallRecord(on_complete)

    def _guarded(self, run):
        """Run the engine calls of one policy call; if an engine refuses because an earlier (unread) call
        faulted, acknowledge on every engine -- that marks the earlier calls suspect, they are recomputed when read -- and retry."""
        from ._lib import LDPHipFault
        for attempt in range(4):                     # in-flight pre-safe-mode launches may still fault after the first acknowledge
            try:
                return run()
            except LDPHipFault:
                if attempt == 3:
                    raise
                torch.cuda.current_stream(self._device).synchronize()
                for e in self._engines():
                    e.poll_fault_kinds()

    def _call(self, run, recompute=None):
        """One policy call under the fault protocol -> (run()'s tensors, the CallRecord its DeviceArrays carry).  recompute: what a later
        fault poll runs instead of `run` (a call with lazy arrays, or one that must not run twice)."""
        rec = self._record(run if recompute is None else recompute)
        res = self._guarded(run)
        rec.seqs = self._seqs()
        return res, rec

    # ---- the hand-off between a state (ParamState / DPState) and one module slot of an engine handle ---------------------------
    _ema_decay = None                     # decay of the parameter EMA a class trains with (DPVAEAgent, StableVAEModel); None: no EMA, ParamState

    def _slot_weights(self, eng, slot, state, shapes, use_ema=False):
        """Sampling side: the slot must hold this state's parameters (its EMA when use_ema; each set has its own token).  Nothing to do when
        the engine already holds the token; a state an update() left in the training arenas is published from there (master parameters ->
        packed sampling layouts on the device, no tree passes through Python); otherwise -> the checked host tree, for the caller to upload
        under that token (LDPAgent sends several slots in one load_params).  shapes: () -> {path: shape}, called only for a host tree."""
        want = state.ema_version if use_ema else state.version
        if eng.loaded[slot] == want:
            return None
        if getattr(eng, "train_ema_token" if use_ema else "train_token", {}).get(slot) == want:
            (eng.train_publish_ema if use_ema else eng.train_publish)([slot], versions={slot: want})
            return None
        tree = state.ema_params if use_ema else state.params
        W.check_params(tree, shapes())
        return tree

    def _train_sync(self, slot, state, shapes, eng=None, decay=None):
        """Training side: the arenas of `eng` (default: the first handle) must hold THIS state -- parameters, Adam moments (fresh when the
        state has none) and, for a class with an EMA, the EMA arena: enabled with the class's decay (`decay`: this slot's own, for a class
        whose states have different ones), re-seeded from the parameters by the (re)load, then overwritten with a distinct EMA tree.  Another
        model sharing the engine, a load_snapshot or a fresh create may have left something else there.  A (re)load synchronises the device:
        call it before anything of the step is in flight."""
        eng = self._engine if eng is None else eng
        decay = self._ema_decay if decay is None else decay
        if eng.train_token.get(slot) == state.version and (decay is None or eng.train_ema_token.get(slot) == state.ema_version):
            return
        W.check_params(state.params, shapes)
        ema = None if decay is None or state.ema_is_params else state.ema_params          # (read before the arenas are overwritten)
        o = state.opt_state
        eng.train_load(slot, state.params, mu=None if o is None else o["mu"], nu=None if o is None else o["nu"], step=state.step,
                       token=state.version)
        if decay is None:
            return
        if eng.ema_decay.get(slot) != decay:
            eng.train_ema(slot, decay)
        if ema is not None:
            W.check_params(ema, shapes)
            eng.train_write(slot, eng.TRAIN_EMA, ema)
        eng.train_ema_token[slot] = state.ema_version

    def _trained_state(self, slot, old, shapes, eng=None):
        """The state after a step: parameters, moments and EMA stay in the arenas and are fetched on demand, while it is the newest state."""
        eng = self._engine if eng is None else eng
        with_ema = self._ema_decay is not None
        token, etoken = next(_versions), next(_versions) if with_ema else None
        eng.train_token[slot] = token
        if with_ema:
            eng.train_ema_token[slot] = etoken
        which = {"params": eng.TRAIN_PARAMS, "mu": eng.TRAIN_MU, "nu": eng.TRAIN_NU, "ema": eng.TRAIN_EMA}

        def fetch(what):
            if eng.train_token.get(slot) != token or (what == "ema" and eng.train_ema_token.get(slot) != etoken):
                raise RuntimeError(f"this {slot} state was superseded by a later update(): its buffers were donated to the next step "
                                   "(keep what update() returned, as train_bc.py:107 and train_vae.py do)")
            return eng.train_read(slot, which[what], shapes)
        if with_ema:
            return DPState(None, None, old.step + 1, token, None, fetch, etoken, lambda: fetch("ema"))
        return ParamState(None, old.ema_params, old.step + 1, token, None, fetch)

    # ---- the statistics scalars of a metrics dict: 4-vectors (min, max, mean, std) on the device, a metric is one element of its vector ----
    @staticmethod
    def _stat_metrics(m, emb_key, arrs, obs_keys, n=2):
        """arrs: the reduce_stats vectors of [embedding / condition, actions, every obs key]; the first n of the four statistics per obs key."""
        tail = ("min", "max", "mean", "std")
        m.update({f"{emb_key}_{s}": _Elem(arrs[0], i) for i, s in enumerate(tail)})
        m["action_min"], m["action_max"] = _Elem(arrs[1], 0), _Elem(arrs[1], 1)
        for j, k in enumerate(obs_keys):
            m.update({f"{k}_{s}": _Elem(arrs[2 + j], i) for i, s in enumerate(tail[:n])})


class LDPAgent(_EngineCalls):
    # ---------------------------------------------------------------------------------------------
    def __init__(self, planner_state, idm_state, vae_params, obs_normalization, use_planner, use_idm,
                 alpha_planner, alpha_idm, config, engine: Optional[HipEngine], planner_spec, idm_spec,
                 vae_spec, device, lr_schedules=None):
        self.planner_state = planner_state
        self.idm_state = idm_state
        self.vae_params = vae_params
        self.obs_normalization = obs_normalization
        self.use_planner, self.use_idm = use_planner, use_idm
        self.alpha_planner, self.alpha_idm = alpha_planner, alpha_idm
        self.config = config
        self._engine = engine
        self._planner_spec, self._idm_spec, self._vae_spec = planner_spec, idm_spec, vae_spec
        self._device = device
        self._vae_version = next(_versions)
        # {"planner": f(count), "idm": f(count)}: optax.warmup_cosine_decay_schedule per network (agent/ldp_agent.py:583-589, 621-627); the
        # reference object also keeps `self.lr_schedule` -- whichever of the two `create` built LAST (:669) -- and reports THAT one's value for
        # both `planner_lr` and `idm_lr` (:257,266): kept as `lr_schedule` for the metrics only
        self._lr_schedules = lr_schedules or {}
        self.lr_schedule = self._lr_schedules.get("idm" if use_idm else "planner")

    # ---------------------------------------------------------------------------------------------
    @classmethod
    def create(cls, rng, batch, shape_meta,
               # Hydra config (agent/ldp_agent.yaml)
               name, planner, idm_net, preprocess_time, cond_encoder,
               vae_pretrain_path, vae_feature_dim,
               use_planner, use_idm,
               lowdim_obs, rgb_obs, obs_normalization, data_name,
               obs_horizon, pred_horizon, action_horizon,
               planner_n_diffusion_steps, idm_n_diffusion_steps,
               alpha_planner=1, alpha_idm=1,
               lr=None, end_lr=None, idm_lr=None, idm_end_lr=None,
               warmup_steps=None, decay_steps=None,
               update_planner_every=1, update_idm_every=1, update_idm_after=-1,
               update_planner_until=-1, update_planner_after=-1,
               grad_clip=None, device=None, vae_params=None, exclusive_gpu=True):
        """agent/ldp_agent.py:516-672.  `batch` is accepted for signature parity (the reference
        traces shapes from it); dims come from `shape_meta` exactly as there (:534-540).

        exclusive_gpu=False: another engine process computes on the same GPU.  Results are bit-stable either way
        (DESIGN.md 4.5), but the work-groups of the in-launch exchanges (column split, K split) then spin while the other
        process holds the CUs; this runs the handle without them (`safe_mode`, about half the speed at <= 256 plans)."""
        lowdim_obs, rgb_obs = list(lowdim_obs), list(rgb_obs)
        if len(rgb_obs) > 1:
            # get_obs_cond concatenates cameras on the time axis (:93-94): only defined for one
            raise NotImplementedError("more than one rgb_obs key: the reference's get_obs_cond "
                                      "concatenates cameras on axis 1 and is only well-defined for one")
        lowdim_dim = sum(int(np.prod(shape_meta["all_shapes"][k])) for k in lowdim_obs)
        # vae_feature_dim 16 (2x2x4 latent of 64x64 frames) is what every shipped config uses; agent/ldp_agent.py:69-80
        # also lists 32 / 36 / 64 (other latent shapes / image sizes: 64 / 96 / 128 pixel frames): all four are built
        if int(vae_feature_dim) not in LATENT_SHAPES:
            raise NotImplementedError(f"vae_feature_dim={vae_feature_dim}: the latent shapes of agent/ldp_agent.py:69-80 are "
                                      f"{sorted(LATENT_SHAPES)} (2x2x4, 2x2x8, 3x3x4, 4x4x4)")
        side, latent_ch = LATENT_SHAPES[int(vae_feature_dim)]
        image_size = 32 * side
        for k in rgb_obs:
            raw = k[len("latent_"):] if k.startswith("latent_") else k
            shp = shape_meta.get("all_shapes", {}).get(raw)
            if shp is not None and tuple(int(v) for v in shp) != (image_size, image_size, 3):
                raise NotImplementedError(f"image key {raw!r} has shape {tuple(shp)}: vae_feature_dim={vae_feature_dim} "
                                          f"means {image_size}x{image_size}x3 frames for the StableVAE")
        obs_dim = lowdim_dim + int(vae_feature_dim) * len(rgb_obs)
        if obs_dim > 128:
            raise NotImplementedError(f"obs_dim={obs_dim}: the planner's first conv is packed for observation "
                                      "embeddings of at most 128 features")
        action_dim = int(shape_meta["ac_dim"])
        seed = _seed_of(rng)

        down_dims = tuple(int(d) for d in _get(planner, "down_dims", (256, 512, 1024)))
        pspec = W.PlannerSpec(input_dim=obs_dim, global_cond_dim=obs_dim * int(obs_horizon),
                              diffusion_step_embed_dim=int(_get(planner, "diffusion_step_embed_dim", 256)),
                              down_dims=down_dims, kernel_size=int(_get(planner, "kernel_size", 5)),
                              n_groups=int(_get(planner, "n_groups", 8)),
                              downsample=bool(_get(planner, "downsample", True)))
        if not pspec.downsample:
            raise NotImplementedError("downsample=False planners are not built")
        if any(d < 256 or d % 128 for d in down_dims) or pspec.kernel_size != 5 or pspec.n_groups != 8:
            raise NotImplementedError(f"planner down_dims={down_dims} kernel_size={pspec.kernel_size} n_groups="
                                      f"{pspec.n_groups}: the MFMA conv tiles are built for kernel_size 5, 8 groups and "
                                      "levels that are multiples of 128 channels and at least 256 wide")
        if not bool(_get(idm_net, "use_layer_norm", True)) or _get(idm_net, "dropout_rate", None):
            raise NotImplementedError("IDM variants other than LayerNorm / no dropout are not built")
        if str(_get(cond_encoder, "activations", "mish")) != "mish" or bool(_get(cond_encoder, "activate_final", False)):
            raise NotImplementedError("cond_encoder must be MLP(mish, activate_final=False)")
        if bool(_get(preprocess_time, "learnable", False)):
            raise NotImplementedError("learnable FourierFeatures are not built")
        ispec = W.IDMSpec(obs_dim=obs_dim, action_dim=action_dim,
                          time_dim=int(_get(preprocess_time, "output_size", 256)),
                          cond_hidden=tuple(int(h) for h in _get(cond_encoder, "hidden_dims", (256, 256))),
                          hidden_dim=int(_get(idm_net, "hidden_dim", 256)),
                          n_blocks=int(_get(idm_net, "n_blocks", 3)))
        vspec = W.VAESpec(latent_channels=latent_ch)

        planner_state = idm_state = None
        if use_planner:
            planner_state = ParamState(W.init_planner_params(pspec, seed=seed * 3 + 1, perturb=False))
        if use_idm:
            idm_state = ParamState(W.init_idm_params(ispec, seed=seed * 3 + 2, perturb=False))
        if vae_params is None and vae_pretrain_path is not None:
            vae_params = load_pretrained_vae(str(vae_pretrain_path))
        vae_params = _as_flat(vae_params) if vae_params is not None else None

        config = dict(planner_n_diffusion_steps=int(planner_n_diffusion_steps),
                      idm_n_diffusion_steps=int(idm_n_diffusion_steps),
                      lowdim_obs=lowdim_obs, rgb_obs=rgb_obs, obs_horizon=int(obs_horizon),
                      name=name, action_dim=action_dim,
                      pred_horizon=int(pred_horizon), action_horizon=int(action_horizon),
                      obs_dim=obs_dim,
                      update_planner_every=update_planner_every, update_idm_every=update_idm_every,
                      update_planner_until=update_planner_until,
                      update_planner_after=update_planner_after,
                      update_idm_after=update_idm_after,
                      vae_feature_dim=int(vae_feature_dim), data_name=data_name)
        norm = {"obs": {k: _norm_entry(v) for k, v in dict(obs_normalization["obs"]).items()}}
        if "actions" in obs_normalization:
            norm["actions"] = _norm_entry(obs_normalization["actions"])

        if not torch.cuda.is_available():
            from ._lib import LDPHipUnavailable
            raise LDPHipUnavailable("no HIP device visible: LDPAgent has no CPU fallback")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        engine = HipEngine(obs_dim=obs_dim, action_dim=action_dim, global_cond_dim=pspec.global_cond_dim,
                           pred_horizon=int(pred_horizon), action_horizon=int(action_horizon),
                           down_dims=down_dims, kernel_size=pspec.kernel_size, n_groups=pspec.n_groups,
                           step_embed_dim=pspec.diffusion_step_embed_dim,
                           planner_train_steps=int(planner_n_diffusion_steps),
                           idm_train_steps=int(idm_n_diffusion_steps), idm_hidden=ispec.hidden_dim,
                           idm_blocks=ispec.n_blocks, idm_time_dim=ispec.time_dim, image_size=image_size,
                           vae_latent_channels=latent_ch, device=dev)
        if not exclusive_gpu:
            engine.set_option("safe_mode", 1)
        from .schedule import warmup_cosine_decay_schedule
        sched = {}
        if lr is not None and warmup_steps is not None and decay_steps is not None:
            if use_planner:
                sched["planner"] = warmup_cosine_decay_schedule(float(end_lr), float(lr), int(warmup_steps), int(decay_steps), float(end_lr))
            if use_idm:
                sched["idm"] = warmup_cosine_decay_schedule(float(idm_end_lr if idm_end_lr is not None else end_lr),
                                                            float(idm_lr if idm_lr is not None else lr), int(warmup_steps), int(decay_steps),
                                                            float(idm_end_lr if idm_end_lr is not None else end_lr))
        return cls(planner_state, idm_state, vae_params, norm, use_planner, use_idm, alpha_planner,
                   alpha_idm, config, engine, pspec, ispec, vspec, dev, lr_schedules=sched)

    # ---------------------------------------------------------------------------------------------
    def replace(self, **fields):
        """flax.struct `.replace`: a shallow copy sharing the engine (weights re-upload lazily)."""
        new = copy.copy(self)
        for k, v in fields.items():
            if not hasattr(new, k):
                raise AttributeError(f"LDPAgent has no field {k!r}")
            if k == "vae_params":
                v = _as_flat(v)
                new._vae_version = next(_versions)
            setattr(new, k, v)
        return new

    def get_params(self):
        """agent/ldp_agent.py:508-514."""
        params = {}
        if self.use_planner:
            params["planner_params"] = self.planner_state.params
        if self.use_idm:
            params["idm_params"] = self.idm_state.params
        return params

    def _sync_weights(self, need_vae=False):
        """Upload whatever the (possibly shared) engine does not hold for THIS agent: the engine keeps the
        version token of each module's tree, the agent compares it with its own."""
        use_ema, ups = self._sample_ema, []                   # ups: (handle, slot, tree, token) still to upload
        for net in self._nets():
            st = getattr(self, f"{net.key}_state")
            tree = self._slot_weights(net.eng, net.slot, st, net.shapes, use_ema)
            if tree is not None:
                ups.append((net.eng, net.slot, tree, st.ema_version if use_ema else st.version))
        if need_vae and self._engine.loaded["vae"] != self._vae_version:
            if self.vae_params is None:
                raise ValueError("raw image observations need VAE weights (vae_pretrain_path / vae_params)")
            ups.append((self._engine, "vae", self.vae_params, self._vae_version))
        for eng in self._engines():                           # one load_params per handle
            mine = [u for u in ups if u[0] is eng]
            if mine:
                eng.load_params(**{slot: tree for _, slot, tree, _ in mine}, versions={slot: token for _, slot, _, token in mine})

    _sample_ema = False                                       # sample with the EMA of the parameters (DPVAEAgent's use_ema)

    def _nets(self):
        """The diffusion networks of this agent, the planner first: `key` names the `<key>_state` attribute, the schedule, the alpha and
        the metric prefix; `eng` / `slot` say where the network lives (LDPHierAgent's IDM is a U-Net in a second handle's planner slot);
        `grad` is its tape, for the planner (x0, eps, t, cond, alpha) and for the IDM (s, a, eps, t, alpha); `stream` is the Philox stream
        of its training noise, `noise` the keys of its explicit timesteps / noise, `steps` its number of diffusion steps."""
        cfg, eng = self.config, self._engine
        nets = []
        if self.use_planner:
            nets.append(_Net("planner", eng, "planner", self._planner_shapes, eng.train_planner_grad, 7, ("t_plan", "noise_plan"),
                             cfg.get("planner_n_diffusion_steps")))
        if self.use_idm:
            nets.append(_Net("idm", eng, "idm", self._idm_shapes, eng.train_idm_grad, 8, ("t_idm", "noise_idm"), cfg.get("idm_n_diffusion_steps")))
        return nets

    def _planner_shapes(self):
        return W.planner_shapes(self._planner_spec)

    def _idm_shapes(self):
        return W.idm_shapes(self._idm_spec)

    # ---- pre/post-processing: _t / _apply_norm / _normalize_dict are _EngineCalls' (utils/data_utils.py:18-80) ----
    def _postprocess(self, batch):
        """postprocess_batch / postprocess_batch_obs selection of agent/ldp_agent.py:436-440."""
        if "actions" in batch.keys():
            out = {"obs": self._normalize_dict(batch["obs"], self.obs_normalization["obs"])}
            out["actions"] = self._apply_norm(self._t(batch["actions"]), self.obs_normalization["actions"], True)
            return out
        assert len(batch.keys()) == 1
        return {"obs": self._normalize_dict(batch["obs"], self.obs_normalization["obs"])}

    # ---- agent/ldp_agent.py:46-64 -----------------------------------------------------------------
    def vae_encode(self, batch):
        """agent/ldp_agent.py:46-64.  Called on its own (the reference's public method) the encode is a recorded, guarded call like vae_decode: the
        StableVAE's stride-2 / split convs sit behind the range guard, and a fault is recomputed and reported instead of leaving inf latents with
        the caller.  The agent's own policy calls use _vae_encode_t inside their recorded run."""
        keys = [k for k in batch.keys() if f"latent_{k}" in self.config["rgb_obs"]]
        if not keys:
            return {k: self._t(v) for k, v in batch.items()}

        def run():
            out = self._vae_encode_t(batch)
            return [out[k] for k in out]
        res, rec = self._call(run)
        order = [(f"latent_{k}" if k in keys else k) for k in batch.keys()]
        return {k: DeviceArray(t, record=rec) for k, t in zip(order, res)}

    def _vae_encode_t(self, batch):
        new_batch = {}
        for key in batch.keys():
            if f"latent_{key}" not in self.config["rgb_obs"]:
                new_batch[key] = self._t(batch[key])
                continue
            self._sync_weights(need_vae=True)
            init_obs = self._t(batch[key])
            B, H = init_obs.shape[:2]
            z = self._engine.vae_encode(init_obs.reshape(-1, *init_obs.shape[-3:]))   # NHWC in, NHWC mean out
            feats = z.reshape(B, H, -1)
            feats = self._apply_norm(feats, self.obs_normalization["obs"][f"latent_{key}"], True)
            new_batch[f"latent_{key}"] = feats
        return new_batch

    # ---- agent/ldp_agent.py:66-85 -----------------------------------------------------------------
    def _vae_decode_t(self, feats: torch.Tensor) -> torch.Tensor:
        B, H = feats.shape[:2]
        fd = self.config["vae_feature_dim"]
        side, latent_ch = LATENT_SHAPES[fd]
        if self.vae_params is None or "decoder/conv_in/kernel" not in self.vae_params:
            raise ValueError("plan_viz needs the StableVAE decoder weights (vae_pretrain_path / vae_params with "
                             "decoder/... and post_quant_conv/...)")
        self._sync_weights(need_vae=True)
        z = feats[:, :, :fd].reshape(B * H, side, side, latent_ch)        # agent/ldp_agent.py:69-80
        key = self.config["rgb_obs"][0]
        z = self._apply_norm(z.contiguous(), self.obs_normalization["obs"][key], False)
        img = self._engine.vae_decode(z)                      # (B*H, 3, S, S), like decode(...).sample
        return img.reshape(B, H, *img.shape[1:])

    def vae_decode(self, feats):
        t = self._t(feats)

        def run():
            return [self._vae_decode_t(t)]
        res, rec = self._call(run)                                # the decoder's split convs sit behind the range guard
        return DeviceArray(res[0], record=rec)

    # ---- agent/ldp_agent.py:88-97 -----------------------------------------------------------------
    def get_obs_cond(self, batch):
        lowdim = torch.cat([self._t(batch[k]) for k in self.config["lowdim_obs"]], dim=-1)
        B, H = lowdim.shape[:2]
        img = torch.cat([self._t(batch[k]) for k in self.config["rgb_obs"]], dim=1)
        return torch.cat([img.reshape(B, H, -1), lowdim.reshape(B, H, -1)], dim=-1)

    def _action_bounds(self):
        """(lo, hi, mode) of utils/data_utils.py:61-68 for the un-normalisation of actions."""
        e = self.obs_normalization["actions"]
        if "min" in e:
            return np.atleast_1d(np.asarray(e["min"], np.float32)), np.atleast_1d(np.asarray(e["max"], np.float32)), 0
        return np.asarray([e["clip_min"]], np.float32), np.asarray([e["clip_max"]], np.float32), 2

    # ---- IDM loop shared by the action samplers ---------------------------------------------------
    def _idm_actions(self, first, second, seed, B, noise=None, row_offset=0, sampler="ddpm", n_steps=None):
        trans = torch.cat([first, second], dim=-1)
        trans = trans.reshape(-1, trans.shape[-1]).contiguous()          # 'B H D -> (B H) D'
        a_init = a_noise = None
        if noise is not None:
            a_init, a_noise = noise.get("a_init"), noise.get("a_noise")
        rows_per = trans.shape[0] // B
        if sampler == "dpmpp":                                 # the solver is the planner's: the IDM loop of such a call is DDIM
            sampler = "ddim"
        a = self._engine.idm_sample(trans, a_init=a_init, step_noise=a_noise, seed=seed,
                                    row_offset=row_offset * rows_per, sampler=sampler, n_steps=n_steps)
        a = a.reshape(B, -1, a.shape[-1])
        return self._apply_norm(a, self.obs_normalization["actions"], False)

    # ---- agent/ldp_agent.py:350-389 ---------------------------------------------------------------
    def sample_action_from_plan(self, batch, next_plan, eval_rng, noise=None):
        seed = _seed_of(eval_rng)

        def run():
            self._sync_weights()
            nb = self._postprocess(batch)
            obs = self._vae_encode_t(nb["obs"])
            start = self.get_obs_cond(obs)
            return [self._idm_actions(start, self._t(next_plan), seed, start.shape[0], noise)]
        res, rec = self._call(run)
        return DeviceArray(res[0], record=rec)

    # ---- agent/ldp_agent.py:391-430 ---------------------------------------------------------------
    def sample_action(self, batch, eval_rng, noise=None):
        seed = _seed_of(eval_rng)

        def run():
            self._sync_weights()
            nb = self._postprocess(batch)
            obs = self._vae_encode_t(nb["obs"])
            plan = self.get_obs_cond(obs)
            return [self._idm_actions(plan[:, :-1], plan[:, 1:], seed, plan.shape[0], noise)]
        res, rec = self._call(run)
        return DeviceArray(res[0], record=rec)

    # ---- agent/ldp_agent.py:432-506 ---------------------------------------------------------------
    def sample(self, batch, eval_rng, **kw):
        """agent/ldp_agent.py:432-433.  Same return value as sample_viz; the only difference is that the
        image decode behind metrics['plan_viz'] is deferred until (unless) the caller reads it."""
        kw.setdefault("decode", False)
        return self.sample_viz(batch, eval_rng, **kw)

    def get_action(self, batch, eval_rng, **kw):
        """Alias named by BASELINE.json's north_star (the reference has no such method)."""
        return self.sample(batch, eval_rng, **kw)[0]

    def _solver_setup(self, sampler, n_steps, idm_steps, timesteps):
        """The host side of sampler="dpmpp" (DPM-Solver++(2M) over a timestep table: DESIGN.md 4.18), before any GPU work: the IDM loop
        of such a call is DDIM with idm_steps, which must divide idm_n_diffusion_steps; timesteps = "logsnr" / "uniform" / a sequence of
        n_steps integers is registered with every engine of this agent as the table of n_steps (None: the table the engine holds, or
        the log-SNR grid when it holds none)."""
        if sampler != "dpmpp":
            if timesteps is not None:
                raise ValueError('timesteps= belongs to sampler="dpmpp"')
            return
        from .schedule import solver_timesteps
        cfg = self.config
        ns = int(cfg["planner_n_diffusion_steps"] if n_steps is None else n_steps)
        if self.use_idm:
            idm_n = int(cfg["idm_n_diffusion_steps"])
            k = idm_n if idm_steps is None else int(idm_steps)
            if k < 1 or idm_n % k != 0:
                raise ValueError(f"idm_steps = {k} must divide idm_n_diffusion_steps = {idm_n} (the IDM loop of a \"dpmpp\" call is DDIM; "
                                 "idm_steps defaults to n_steps)")
        if timesteps is None:
            return
        if isinstance(timesteps, str):
            ts = solver_timesteps(int(cfg["planner_n_diffusion_steps"]), ns, timesteps)
        else:
            ts = np.asarray(timesteps, dtype=np.int64).reshape(-1)
            if len(ts) != ns:
                raise ValueError(f"timesteps must have n_steps = {ns} entries, got {len(ts)}")
        for e in self._engines():
            e.set_solver_timesteps(ts)

    # ---- what sample_viz, sample_warm, sample_constrained, sample_guided and plan share -----------------------------------------
    def _sample_setup(self, eval_rng, sampler, n_steps, idm_steps, noise):
        """-> (idm_steps, kw): idm_steps with its default, and the keywords every engine call of these methods takes as they are --
        the seed of eval_rng, sampler, idm_steps and the explicit-noise tensors of `noise` (None where it has none)."""
        seed = _seed_of(eval_rng)
        if idm_steps is None and n_steps is not None and sampler != "ddpm":
            idm_steps = n_steps                                # one schedule for both loops unless told otherwise
        nz = noise or {}
        kw = dict(seed=seed, sampler=sampler, idm_steps=idm_steps, x_init=nz.get("x_init"), x_noise=nz.get("x_noise"), a_init=nz.get("a_init"),
                  a_noise=nz.get("a_noise"))
        return idm_steps, kw

    def _sample_call(self, batch, call, keys=(), prev=None, decode=False):
        """One sampling call under the fault protocol -> (action, metrics): normalize -> vae_encode -> get_obs_cond -> ONE engine call
        (planner loop, plan assembly, IDM loop, action un-normalisation as one captured graph) -> _plan_metrics.
        call(obs_emb, bounds) makes the engine call -- bounds: its action_bounds / action_mode keywords -- and returns (x, plan, action)
        and, behind them, the tensors of keys[1:].  keys: what metrics holds between 'plan' and 'plan_mse' ('x' first, when at all).
        prev: a warm call's previous state (it may belong to the call that faulted: a recompute completes it first)."""
        oh = self.config["obs_horizon"]

        def run():
            self._sync_weights()
            obs_emb = self.get_obs_cond(self._vae_encode_t(self._postprocess(batch)["obs"])).contiguous()
            lo, hi, mode = self._action_bounds()
            x, plan, action, *more = call(obs_emb, dict(action_bounds=(lo, hi), action_mode=mode))
            out = [action, plan] + ([x] if keys else []) + more
            if obs_emb.shape[1] > oh:                          # from a training batch, not inference (:447-448)
                out.append(self._engine.mean_sq_diff(x, obs_emb[:, oh:]))
            return out

        def recompute():
            if isinstance(prev, DeviceArray):
                prev.complete()                                # the previous call may be the one that faulted: its x first
            return run() + [None]                              # plan_viz re-decodes itself from the new plan
        res, rec = self._call(run, recompute)
        return self._plan_metrics(res, rec, keys, decode)

    def _plan_metrics(self, res, rec, keys, decode):
        """res: the tensors [action, plan, *those named by keys, plan_mse when the batch has future frames] of a call recorded in rec
        -> (action, metrics) as DeviceArrays (created in that order: a recompute swaps them by position), with metrics['plan_viz']
        decoding itself from the plan when it is read (decode: enqueued now, no host sync)."""
        action, plan, *rest = (DeviceArray(t, record=rec) for t in res)
        metrics = {"plan": plan, **dict(zip(tuple(keys) + ("plan_mse",), rest))}
        S = self._engine.image_size
        viz = DeviceArray(thunk=lambda: self._vae_decode_t(plan.tensor), shape=tuple(plan.shape[:2]) + (3, S, S), record=rec)
        if decode:
            viz.tensor
        metrics["plan_viz"] = viz
        return action, metrics

    def sample_viz(self, batch, eval_rng, noise=None, decode=True, row_offset=0,
                   sampler="ddpm", n_steps=None, idm_steps=None, timesteps=None):
        """-> (action (B, ah, A), {'plan' (B, ah+1, D), 'plan_viz' (B, ah+1, 3, S, S)[, 'plan_mse']}), all
        DeviceArrays.
        noise: optional dict(x_init (B,T,D), x_noise (S,B,T,D), a_init (B*ah,A), a_noise (S,B*ah,A))
        for explicit-noise parity runs.  decode: True = enqueue the VAE decode of the plan now (the
        reference always does, agent/ldp_agent.py:483); False = leave metrics['plan_viz'] lazy (the
        decode is 5 x 24.9 GFLOP per plan and callers such as eval_bc.py:144 discard it).
        row_offset: global index of this batch's first plan (keeps the Philox stream independent of how
        candidates are sharded over GPUs).  n_steps / idm_steps: denoising steps (DDIM and DPM-Solver++; DDPM
        visits every training timestep).  sampler="dpmpp": the planner loop is DPM-Solver++(2M) over the timestep
        table `timesteps` (None / "logsnr" / "uniform" / n_steps integers: _solver_setup), the IDM loop DDIM."""
        _need_nets(self, "sample")
        idm_steps, kw = self._sample_setup(eval_rng, sampler, n_steps, idm_steps, noise)
        self._solver_setup(sampler, n_steps, idm_steps, timesteps)
        oh = self.config["obs_horizon"]

        def call(obs_emb, bounds):
            return self._engine.agent_sample(obs_emb, oh, row_offset=row_offset, planner_steps=n_steps, **kw, **bounds)
        return self._sample_call(batch, call, decode=decode)

    # ---- warm-started replanning (defined by this repository: DESIGN.md 4.16; csrc/replan.hip, replan.py) ---------------------
    def sample_warm(self, batch, eval_rng, prev, warm_steps, shift=None, sampler="ddim", n_steps=None, idm_steps=None, noise=None,
                    row_offset=0, decode=False):
        """sample() resumed from the previous call's plan -> (action, metrics): metrics is sample()'s plus 'x', the full planner state
        (B, T, D) as a DeviceArray -- the `prev` of the next call.
        prev: metrics['x'] of the previous call, or a (B, T, D) device tensor (it is not modified).  warm_steps = k runs the last k of the
        n_steps planner steps (1 <= k <= n_steps) from the warm initial state: prev shifted by `shift` positions (default action_horizon)
        with the edge held, noised to the level of step n_steps - k with the Philox draw a cold call would use as x_T.  The IDM loop, the
        plan assembly and the un-normalisation are sample()'s.  noise: optional dict(x_noise, a_init, a_noise) as in sample_viz (the
        initial state is the warm one: no x_init).
        prev=None, warm_steps=None is the cold call that also returns 'x' (the existing path)."""
        from .replan import check_warm_steps
        if sampler == "dpmpp":
            raise NotImplementedError('a warm start under sampler="dpmpp" is not built: its noise levels assume the uniform timestep grid')
        _need_nets(self, "sample_warm")
        if (prev is None) != (warm_steps is None):
            raise ValueError("prev and warm_steps go together: both None (a cold call that returns 'x') or both given")
        idm_steps, kw = self._sample_setup(eval_rng, sampler, n_steps, idm_steps, noise)
        cfg = self.config
        oh = cfg["obs_horizon"]
        ns = int(cfg["planner_n_diffusion_steps"] if n_steps is None else n_steps)
        if prev is None:
            def call(obs_emb, bounds):
                return self._engine.agent_sample(obs_emb, oh, row_offset=row_offset, planner_steps=n_steps, **kw, **bounds)
        else:
            step_begin = check_warm_steps(warm_steps, ns)
            if "x_init" in (noise or {}):
                raise ValueError("a warm call has no x_init: its initial state is the shifted, noised previous plan")
            sh = int(cfg["action_horizon"] if shift is None else shift)
            if sh < 0:
                raise ValueError(f"shift must be >= 0, got {shift}")
            del kw["x_init"]                                   # (agent_resample takes none)

            def call(obs_emb, bounds):
                store = self._t(prev).clone()                  # the engine writes the new state back in place: not into the caller's prev
                if tuple(store.shape) != (obs_emb.shape[0], cfg["pred_horizon"], cfg["obs_dim"]):
                    raise ValueError(f"prev must have shape {(obs_emb.shape[0], cfg['pred_horizon'], cfg['obs_dim'])}, got {tuple(store.shape)}")
                return self._engine.agent_resample(obs_emb, oh, store, step_begin, shift=sh, row_offset=row_offset, planner_steps=ns,
                                                   **kw, **bounds)
        return self._sample_call(batch, call, ("x",), prev=prev, decode=decode)

    def replanner(self, n_slots, warm_steps, sampler="ddim", n_steps=None, shift=None):
        """A Replanner (replan.py) for closed-loop control of up to n_slots environments: it keeps every environment's previous planner
        state on the device and runs a row warm -- the last warm_steps of n_steps planner steps -- whenever its slot holds one."""
        from .replan import Replanner
        if sampler == "dpmpp":
            raise NotImplementedError('a warm start under sampler="dpmpp" is not built: its noise levels assume the uniform timestep grid')
        if not (self.use_planner and self.use_idm):
            raise NotImplementedError("replanner() needs both the planner and the IDM (use_planner / use_idm)")
        return Replanner(self, n_slots, warm_steps, sampler=sampler, n_steps=n_steps, shift=shift)

    # ---- constrained planning (defined by this repository: DESIGN.md 4.17; csrc/constrain.hip, constrain.py) -------------------
    def sample_constrained(self, batch, eval_rng, target=None, mask=None, goal=None, t_goal=None, goal_dims=None, mode="repaint",
                           sampler="ddpm", n_steps=None, idm_steps=None, noise=None, row_offset=0, decode=False):
        """sample() with goals and waypoints inpainted in the planner loop -> (action, metrics): metrics is sample_warm()'s ('plan', 'x'
        the full planner state (B, T, D), lazy 'plan_viz', 'plan_mse' for a training batch).  After every denoising step the constrained
        entries of the trajectory are overwritten with the known values at that step's noise level (mode 'repaint'; 'clamp' writes the
        values themselves at every level): one planner loop, and metrics['x'] meets the constraint exactly.
        The constraint is constrain.build_constraint's: `target` (B, T, D) with `mask` broadcast from (D,), (T, D) or (B, T, D), and / or
        `goal` -- normalised embeddings (B, D) or an observation dict in batch['obs'] form -- written at step(s) `t_goal` (default
        action_horizon - 1) into the columns `goal_dims` (None / 'all', 'latent', 'lowdim', an index list, a bool (D,) array).  Values
        are in the normalised embedding units of the plan; they belong in [-1, 1], where the scheduler clips its own estimate.  With
        nothing given the call is sample()'s.  noise: optional dict(x_init, x_noise, a_init, a_noise) as in sample_viz.
        The control quality of inpainted plans has not been evaluated (the toy task of DESIGN.md 4.21 has no inpainting arm)."""
        from .constrain import MODES, build_constraint
        if sampler == "dpmpp":
            raise NotImplementedError('a constraint under sampler="dpmpp" is not built: its noise levels assume the uniform timestep grid')
        _need_nets(self, "sample_constrained")
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
        idm_steps, kw = self._sample_setup(eval_rng, sampler, n_steps, idm_steps, noise)
        cfg = self.config

        def call(obs_emb, bounds):
            B = obs_emb.shape[0]
            g = None if goal is None else self._goal_embedding(goal, B)
            tg, mk = build_constraint(cfg, B, target=None if target is None else self._t(target), mask=mask, goal=g, t_goal=t_goal,
                                      goal_dims=goal_dims)
            return self._engine.agent_sample_constrained(obs_emb, cfg["obs_horizon"], tg, mk, mode=mode, row_offset=row_offset,
                                                         planner_steps=n_steps, **kw, **bounds)
        return self._sample_call(batch, call, ("x",), decode=decode)

    # ---- guided planning (defined by this repository: DESIGN.md 4.19; csrc/guide.hip, guide.py) --------------------------------
    def build_guide(self, B, **kw):
        """guide.build_guide for this agent's config, bound to its engine: the result is sample_guided's `guide=` and, being a cost
        function on candidates, sample_best_of's `score=`."""
        from .guide import build_guide
        if not self.use_planner:
            raise NotImplementedError("a guide needs the planner (use_planner)")
        if isinstance(kw.get("goal"), Mapping):
            kw["goal"] = self._goal_embedding(kw["goal"], int(B))
        return build_guide(self.config, B, engine=self._engine, **kw)

    def sample_guided(self, batch, eval_rng, guide=None, target=None, weight=None, goal=None, t_goal=None, goal_dims=None, goal_weight=None,
                      smooth=None, anchor=None, lo=None, hi=None, bound_weight=None, scale=None, schedule="sigma2", sampler="ddim",
                      n_steps=None, idm_steps=None, noise=None, row_offset=0, decode=False):
        """sample() with the plan moved down the gradient of a cost inside every denoising step -> (action, metrics): metrics is
        sample_constrained()'s ('plan', 'x', lazy 'plan_viz', 'plan_mse' for a training batch) plus 'guide_cost' (B,), the cost J of the
        final planner state.  The cost is a guide.Guide -- `guide=`, or built here from guide.build_guide's arguments: soft goals and
        waypoints (target / weight, goal / t_goal / goal_dims / goal_weight, goal as embeddings (B, D) or an observation dict),
        smoothness (smooth, anchor=True: continuity with the batch's own last observation embedding, the state that precedes x[:, 0] in
        'plan') and box bounds (lo, hi, bound_weight).  scale / schedule: the step sizes (guide.Guide.step_sizes); a step size beyond the
        descent bound is a ValueError before the planner loop is enqueued.  The planner loop has one launch more per step than sample()'s; the IDM
        loop, the plan assembly and the un-normalisation are sample()'s.  noise: optional dict(x_init, x_noise, a_init, a_noise) as in
        sample_viz.  Not built (NotImplementedError): sampler="dpmpp".  The control quality of guided plans has been measured on a toy task only."""
        from .guide import Guide, build_guide
        if sampler == "dpmpp":
            raise NotImplementedError('guidance under sampler="dpmpp" is not built: the guided step is the DDPM / DDIM scheduler step')
        _need_nets(self, "sample_guided")
        built = dict(target=target, weight=weight, goal=goal, t_goal=t_goal, goal_dims=goal_dims, goal_weight=goal_weight, smooth=smooth,
                     anchor=anchor, lo=lo, hi=hi, bound_weight=bound_weight, scale=scale)
        if guide is not None:
            given = [k for k, v in built.items() if v is not None] + ([] if schedule == "sigma2" else ["schedule"])
            if given:
                raise ValueError(f"guide= already holds the cost and its step sizes: {', '.join(given)} cannot be given with it")
            if not isinstance(guide, Guide):
                raise ValueError(f"guide must be a guide.Guide (guide.build_guide / LDPAgent.build_guide), got {type(guide).__name__}")
        idm_steps, kw = self._sample_setup(eval_rng, sampler, n_steps, idm_steps, noise)
        cfg = self.config
        oh = cfg["obs_horizon"]
        ns = int(cfg["planner_n_diffusion_steps"] if n_steps is None else n_steps)
        rho = None if guide is None else guide.step_sizes(ns, sampler)      # (a given guide: every host check before any GPU work)

        def call(obs_emb, bounds):
            B = obs_emb.shape[0]
            gd, rh = guide, rho
            if gd is None:
                g = None if goal is None else self._goal_embedding(goal, B)
                gd = build_guide(cfg, B, **dict(built, target=None if target is None else self._t(target), goal=g,
                                                anchor=anchor if anchor is None or anchor is True else self._t(anchor)),
                                 schedule=schedule, engine=self._engine)
                rh = gd.step_sizes(ns, sampler)
            gd = self._batch_guide(gd, obs_emb)
            x, plan, action = self._engine.agent_sample_guided(obs_emb, oh, gd, rh, row_offset=row_offset, planner_steps=n_steps, **kw, **bounds)
            return x, plan, action, self._engine.plan_guide_cost(x, gd)
        return self._sample_call(batch, call, ("x", "guide_cost"), decode=decode)

    def _batch_guide(self, gd, obs_emb):
        """`gd` as the engine takes it for this batch: its B checked, anchor=True resolved to the batch's own current observation (in a
        copy of the guide, not the caller's)."""
        from .guide import Guide
        if gd.B != obs_emb.shape[0]:
            raise ValueError(f"the guide was built for B = {gd.B} plans, the batch holds {obs_emb.shape[0]}")
        if gd.anchor is True:
            gd = Guide(gd.cfg, gd.B, gd.target, gd.weight, obs_emb[:, self.config["obs_horizon"] - 1].contiguous(), gd.lam, gd.beta, gd.lo,
                       gd.hi, gd.scale, gd.schedule, self._engine, gd.wmax)
        return gd

    # ---- composed planning (defined by this repository: DESIGN.md 4.20; csrc/compose.hip) -----------------------------------
    def _guide_step_sizes(self, guide, sampler, n_steps):
        """The step sizes of `guide` for a loop of n_steps under `sampler`: Guide.step_sizes on the uniform grid, Guide.step_sizes_on at
        the entries of the timestep table under "dpmpp" (the table the engine holds for n_steps, else the log-SNR grid it would
        register).  The descent-bound refusal is theirs."""
        if sampler != "dpmpp":
            return guide.step_sizes(n_steps, sampler)
        from .schedule import solver_timesteps
        ts = self._engine.solver_tables.get(int(n_steps))
        if ts is None:
            ts = solver_timesteps(int(self.config["planner_n_diffusion_steps"]), int(n_steps), "logsnr")
        return guide.step_sizes_on(ts)

    def plan(self, batch, eval_rng, *, guide=None, target=None, mask=None, goal=None, t_goal=None, goal_dims=None, mode="repaint",
             prev=None, warm_steps=None, shift=None, sampler="ddim", n_steps=None, idm_steps=None, timesteps=None, noise=None,
             row_offset=0, decode=False):
        """sample() with any of a warm start, a constraint and a guide in ONE planner loop, under any sampler -> (action, metrics):
        metrics holds 'plan', 'x' (the full planner state (B, T, D): the `prev` of the next call), a lazy 'plan_viz', 'guide_cost' (B,)
        when guided, and 'plan_mse' for a training batch.
        guide: a guide.Guide (LDPAgent.build_guide).  target / mask / goal / t_goal / goal_dims / mode: sample_constrained's constraint.
        prev / warm_steps / shift: sample_warm's warm start.  sampler "dpmpp" runs over the timestep table `timesteps` (sample_viz); the
        guide's "sigma2" step sizes and the constraint's noise levels are then taken at the entries of that table.
        With a guide, or under "dpmpp", every denoising step is the U-Net evaluation plus one launch of the step kernel
        (csrc/compose.hip): data prediction, guide, scheduler or solver update, constraint, in that order.  A combination that a
        dedicated method also serves runs that method's loop and returns its bits.  Every refusal is raised before any GPU work.
        The control quality of such plans has been measured on a toy task only."""
        from .constrain import MODES, build_constraint
        from .guide import Guide
        from .replan import check_warm_steps
        _need_nets(self, "plan")
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
        if guide is not None and not isinstance(guide, Guide):
            raise ValueError(f"guide must be a guide.Guide (guide.build_guide / LDPAgent.build_guide), got {type(guide).__name__}")
        if (prev is None) != (warm_steps is None):
            raise ValueError("prev and warm_steps go together: both None (a cold call) or both given")
        if (target is None) != (mask is None):
            raise ValueError("target and mask go together: give both or neither")
        if goal is None and (t_goal is not None or goal_dims is not None):
            raise ValueError("t_goal and goal_dims describe `goal`: give goal too")
        idm_steps, kw = self._sample_setup(eval_rng, sampler, n_steps, idm_steps, noise)
        cfg = self.config
        ns = int(cfg["planner_n_diffusion_steps"] if n_steps is None else n_steps)
        step_begin, sh = 0, None
        if prev is not None:
            step_begin = check_warm_steps(warm_steps, ns)
            if "x_init" in (noise or {}):
                raise ValueError("a warm call has no x_init: its initial state is the shifted, noised previous plan")
            sh = int(cfg["action_horizon"] if shift is None else shift)
            if sh < 0:
                raise ValueError(f"shift must be >= 0, got {shift}")
        elif shift is not None:
            raise ValueError("shift describes a warm start: give prev and warm_steps too")
        self._solver_setup(sampler, n_steps, idm_steps, timesteps)
        rho = None if guide is None else self._guide_step_sizes(guide, sampler, ns)
        constrained = target is not None or goal is not None

        def call(obs_emb, bounds):
            B = obs_emb.shape[0]
            gd = None if guide is None else self._batch_guide(guide, obs_emb)
            tg = mk = None
            if constrained:
                g = None if goal is None else self._goal_embedding(goal, B)
                tg, mk = build_constraint(cfg, B, target=None if target is None else self._t(target), mask=mask, goal=g, t_goal=t_goal,
                                          goal_dims=goal_dims)
            store = None
            if prev is not None:
                store = self._t(prev).clone()                  # the engine writes the new state back in place: not into the caller's prev
                if tuple(store.shape) != (B, cfg["pred_horizon"], cfg["obs_dim"]):
                    raise ValueError(f"prev must have shape {(B, cfg['pred_horizon'], cfg['obs_dim'])}, got {tuple(store.shape)}")
            res = self._engine.agent_sample_composed(
                obs_emb, cfg["obs_horizon"], guide=gd, rho=rho, target=tg, mask=mk, mode=mode, x_store=store, shift=sh, step_begin=step_begin,
                row_offset=row_offset, planner_steps=ns, **kw, **bounds)
            return res if gd is None else (*res, self._engine.plan_guide_cost(res[0], gd))
        return self._sample_call(batch, call, ("x",) if guide is None else ("x", "guide_cost"), prev=prev, decode=decode)

    def controller(self, n_slots, warm_steps, sampler="ddim", n_steps=None, timesteps=None, shift=None):
        """A Controller (replan.py) for closed-loop control of up to n_slots environments: a Replanner whose act() also takes a guide and
        a constraint, under any sampler ("dpmpp": over the timestep table `timesteps`, as in sample_viz)."""
        from .replan import Controller
        if not (self.use_planner and self.use_idm):
            raise NotImplementedError("controller() needs both the planner and the IDM (use_planner / use_idm)")
        self._solver_setup(sampler, n_steps, n_steps, timesteps)
        return Controller(self, n_slots, warm_steps, sampler=sampler, n_steps=n_steps, shift=shift)

    # ---- best-of-N planning (defined by this repository: DESIGN.md 4.14; csrc/select.hip) ----------------------------------
    def _goal_embedding(self, goal, B):
        """`goal`: normalised embeddings (B, D), or an observation dict in batch['obs'] form (embedded like the batch, frame 0)."""
        if isinstance(goal, Mapping):
            obs = self._vae_encode_t(self._postprocess({"obs": goal})["obs"])
            g = self.get_obs_cond(obs)[:, 0]
        else:
            g = self._t(goal)
        if tuple(g.shape) != (B, self.config["obs_dim"]):
            raise ValueError(f"goal must embed to shape {(B, self.config['obs_dim'])}, got {tuple(g.shape)}")
        return g.contiguous()

    def _best_of(self, batch, seed, N, score, bandwidth, goal, goal_weight, t_goal, sampler, n_steps, idm_steps, noise, shard=None):
        """The steps of sample_best_of as device tensors -> [action, plan, best_index, best_cost, costs (B, N), candidates (B, N, T, D)].
        shard = (group, world, rank) (dist.sample_best_of_sharded): this rank draws and costs the candidates shard_bounds(N, world, rank);
        candidates and costs cross the ranks once each.  Whatever leaves the rank, and the redundant tail, is completed first (stream
        synchronised, fault word polled, recomputed on a fault): gathered copies could never be recalled."""
        from .dist import all_gather_rows, shard_bounds
        from .engine import check_candidate_range
        check_candidate_range(1, N, 1, bandwidth=bandwidth if score == "density" else None)
        cfg, eng = self.config, self._engine
        oh, ah, T, D = cfg["obs_horizon"], cfg["action_horizon"], cfg["pred_horizon"], cfg["obs_dim"]
        nz = noise or {}
        c0, c1 = (0, N) if shard is None else shard_bounds(N, shard[1], shard[2])

        def checked(fn):
            if shard is None:
                return fn()
            for _ in range(3):
                out = self._guarded(fn)
                torch.cuda.current_stream(self._device).synchronize()
                if not sum(e.poll_fault_kinds() for e in self._engines()):
                    return out
            raise RuntimeError("libldp_hip faulted again after switching to safe mode / bf16 planes")

        def gather(t):                                         # (n_loc, ...) of this rank's candidates -> (N, ...), in candidate order
            return t if shard is None or shard[1] == 1 else all_gather_rows(t.reshape(t.shape[0], -1).contiguous(), N, shard[0])

        self._sync_weights()
        obs_emb = checked(lambda: self.get_obs_cond(self._vae_encode_t(self._postprocess(batch)["obs"])).contiguous())
        B = obs_emb.shape[0]
        xi, xn = nz.get("x_init"), nz.get("x_noise")
        if xi is not None:
            xi = self._t(xi)[c0 * B:c1 * B]
        if xn is not None:
            xn = self._t(xn)[:, c0 * B:c1 * B]
        if c1 > c0:
            x_loc = checked(lambda: eng.plan_candidates(obs_emb, oh, N, c0=c0, n_loc=c1 - c0, x_init=xi, step_noise=xn, seed=seed,
                                                        sampler=sampler, n_steps=n_steps))
        else:                                                  # more ranks than candidates
            x_loc = torch.zeros((0, T, D), device=self._device)
        x_all = gather(x_loc.reshape(c1 - c0, B * T * D)).reshape(N * B, T, D)
        if callable(score):                                    # every rank scores all candidates: nothing to gather
            cand = x_all.reshape(N, B, T, D).transpose(0, 1).contiguous()
            costs = as_tensor(score(cand))
            if tuple(costs.shape) != (B, N) or not costs.is_cuda:
                raise ValueError(f"score(candidates) must return a device tensor of shape {(B, N)}, got {tuple(costs.shape)} on {costs.device}")
            cost_all = costs.to(dtype=torch.float32).t().contiguous()
        else:
            if score == "density":
                cost_loc = eng.plan_cost_density(x_all, B, bandwidth, c0=c0, n_loc=c1 - c0) if c1 > c0 else None
            elif score == "goal":
                if goal is None:
                    raise ValueError('score="goal" needs goal= (embeddings (B, D) or an observation dict)')
                g = checked(lambda: self._goal_embedding(goal, B))
                cost_loc = eng.plan_cost_goal(x_all[c0 * B:c1 * B], B, g, goal_weight, t_goal) if c1 > c0 else None
            else:
                raise ValueError(f'score must be "density", "goal" or a callable, got {score!r}')
            cost_all = gather(torch.zeros((0, B), device=self._device) if cost_loc is None else cost_loc).reshape(N, B)

        def tail():
            idx, best, x_best = eng.plan_select(cost_all, x_all, B)
            plan = torch.cat([obs_emb[:, oh - 1:oh], x_best[:, :ah]], dim=1)
            action = self._idm_actions(plan[:, :-1], plan[:, 1:], seed, B, nz, sampler=sampler, n_steps=idm_steps)
            return [action, plan, idx, best]
        return checked(tail) + [cost_all.t().contiguous(), x_all.reshape(N, B, T, D).transpose(0, 1).contiguous()]

    def sample_best_of(self, batch, eval_rng, n_candidates, score="density", bandwidth=0.5, goal=None, goal_weight=None, t_goal=None,
                       sampler="ddpm", n_steps=None, idm_steps=None, noise=None, decode=False, prev=None, warm_steps=None, timesteps=None):
        """Draw n_candidates plans per observation, score them on the GPU, act on the best one
        -> (action (B, ah, A), metrics): the action of the winning plan through the IDM, and
           metrics = {'plan' (B, ah+1, D), 'plan_viz' (lazy unless decode), 'best_index' (B,), 'best_cost' (B,), 'costs' (B, N),
                      'candidates' (B, N, T, D)}, all DeviceArrays of one call record, like sample_viz's.
        Candidate c of observation b is global planner row c * B + b (its Philox stream; with n_candidates = 1 row b is sample()'s row b).
        score: "density" -- cost_i = -sum_j exp(-|x_i - x_j|^2 / (2 h^2)), h^2 = bandwidth^2 x the mean squared distance over all pairs of
               the observation's candidates: the candidate in the densest region (mode seeking; lower cost is better everywhere);
               "goal" -- cost_i = sum_d goal_weight[d] (x_i[t_goal, d] - goal[b, d])^2 with goal = normalised embeddings (B, D) or an
               observation dict in batch['obs'] form, goal_weight (D,) >= 0 (default ones), t_goal default action_horizon - 1;
               a callable -- receives the candidates (B, N, T, D) as a device tensor and returns costs (B, N) as a device tensor.
        Ties go to the lowest candidate index, a NaN cost counts as +inf.
        noise: explicit-noise dict with x_init (N*B, T, D) / x_noise (S, N*B, T, D) in candidate-major rows and a_init (B*ah, A) /
        a_noise (S, B*ah, A) for the winners' IDM rows.  sampler="dpmpp" / timesteps: as in sample_viz."""
        if not (self.use_planner and self.use_idm):
            raise NotImplementedError("sample_best_of() needs both the planner and the IDM (use_planner / use_idm)")
        if prev is not None or warm_steps is not None:
            raise NotImplementedError("warm-started candidates are not built: a warm start (prev / warm_steps) is LDPAgent.sample_warm's "
                                      "and LDPAgent.replanner's, one plan per observation")
        N = int(n_candidates)
        seed = _seed_of(eval_rng)
        if idm_steps is None and n_steps is not None and sampler != "ddpm":
            idm_steps = n_steps
        self._solver_setup(sampler, n_steps, idm_steps, timesteps)

        def run():
            return self._best_of(batch, seed, N, score, bandwidth, goal, goal_weight, t_goal, sampler, n_steps, idm_steps, noise)
        res, rec = self._call(run, lambda: run() + [None])             # plan_viz re-decodes itself from the new plan
        return self._best_of_result(res, rec, decode)

    def _best_of_result(self, res, rec, decode):
        arrs = [DeviceArray(t, record=rec) for t in res]
        metrics = dict(zip(("plan", "best_index", "best_cost", "costs", "candidates"), arrs[1:]))
        plan, S = arrs[1], self._engine.image_size
        viz = DeviceArray(thunk=lambda: self._vae_decode_t(plan.tensor), shape=tuple(plan.shape[:2]) + (3, S, S), record=rec)
        if decode:
            viz.tensor
        metrics["plan_viz"] = viz
        return arrs[0], metrics

    # ---- agent/ldp_agent.py:223-323: the training step ----------------------------------------------------------------
    def _gates(self, step):
        """The python-side schedule gates of `update` / `update_mixed` (agent/ldp_agent.py:224-230, 275-281)."""
        cfg = self.config
        use_planner = bool(self.use_planner) and step % cfg["update_planner_every"] == 0
        use_idm = bool(self.use_idm) and step % cfg["update_idm_every"] == 0
        use_idm = use_idm and step >= cfg["update_idm_after"]
        update_planner = cfg["update_planner_until"] < 0 or step < cfg["update_planner_until"]
        update_planner = update_planner and step >= cfg["update_planner_after"]
        return use_planner and update_planner, use_idm

    def update(self, batch, rng, step, noise=None):
        """agent/ldp_agent.py:223-272 -> (new agent, metrics).  One jax.grad(loss) + optax.adam step per network, on the GPU (csrc/train.hip).
        rng: seed of the timesteps (host PCG64) and of the noise (device Philox), as in get_metrics; noise: optional explicit
        dict(t_plan, noise_plan, t_idm, noise_idm) for parity runs."""
        use_planner, use_idm = self._gates(int(step))
        return self._update_step(batch, None, rng, use_planner, use_idm, noise)

    def update_mixed(self, batch, mixed_batch, rng, step, noise=None):
        """agent/ldp_agent.py:274-323: the planner learns from `batch`, the IDM from `mixed_batch`."""
        use_planner, use_idm = self._gates(int(step))
        return self._update_step(batch, mixed_batch, rng, use_planner, use_idm, noise)

    def _update_step(self, batch, mixed_batch, rng, use_planner, use_idm, noise, shard=None):
        """One step of the networks `_nets` describes, on what `_planner_targets` / `_idm_pairs` read of the batch(es).
        shard (dist.update_sharded): dict(group, rows=(lo, n), mixed_rows=(lo, n)) -- `batch` / `mixed_batch` are rows [lo, lo + B) of a
        global batch of n rows split over the ranks of `group`.  Timesteps and noise are those of the global rows (so the step does not
        depend on the world size), each rank's loss is weighted B / n, the gradient arenas are summed over the ranks with one all-reduce per
        network, and everything after it (global norm, Adam) runs replicated."""
        cfg = self.config
        if not self._lr_schedules:
            raise ValueError(f"update() needs the optimiser settings of {type(self).__name__}.create (lr, end_lr, idm_lr, idm_end_lr, warmup_steps, decay_steps)")
        seed = _seed_of(rng)
        oh = cfg["obs_horizon"]
        nz = noise or {}
        nb = self._postprocess(batch)
        if "actions" not in nb:
            raise KeyError("update needs batch['actions'] (utils/data_utils.py:73)")
        obs_emb = self.get_obs_cond(nb["obs"]).contiguous()
        action = nb["actions"]
        emb_i, action_i = obs_emb, action
        if mixed_batch is not None:                                   # loss_mixed: the IDM learns from the mixed batch
            nbm = self._postprocess(mixed_batch)
            emb_i, action_i = self.get_obs_cond(nbm["obs"]).contiguous(), nbm["actions"]
        B, Bi = obs_emb.shape[0], emb_i.shape[0]
        rows_p = (0, B) if shard is None else shard["rows"]           # (first global row, global rows): the weights are 1 without shards
        rows_i = (0, Bi) if shard is None else shard.get("mixed_rows", shard["rows"]) if mixed_batch is not None else shard["rows"]
        trained = {n.key: n for n in self._nets() if (use_planner if n.key == "planner" else use_idm)}
        pn, im = trained.get("planner"), trained.get("idm")
        hg = np.random.Generator(np.random.PCG64(seed & (2**63 - 1)))

        def rows_of(x, rows, n_loc, per=1):
            """An explicit parity input given for the global batch -> this rank's rows."""
            lo, n_glob = rows
            return x[lo * per:(lo + n_loc) * per] if len(x) == n_glob * per and n_glob != n_loc else x

        def timesteps(net, rows, n_loc, per=1):
            """One per row of the network's x0, of the GLOBAL batch: given, or the generator's next draw."""
            t = nz.get(net.noise[0])
            return rows_of(np.asarray(hg.integers(0, int(net.steps), size=rows[1] * per) if t is None else t).reshape(-1), rows, n_loc, per)

        def noise_of(net, x0, rows, n_loc):
            eps = nz.get(net.noise[1])
            if eps is not None:
                return self._t(rows_of(eps, rows, n_loc, x0.shape[0] // n_loc))
            return _philox_normal(seed, rows[0] * (x0.numel() // n_loc), 0, net.stream, x0.numel(), self._device).reshape(x0.shape)

        def weight(net, rows, n_loc):
            return float(np.float32(getattr(self, f"alpha_{net.key}")) * (np.float32(n_loc) / np.float32(rows[1])))
        zero = torch.zeros((), dtype=torch.float32, device=self._device)
        plan_loss = idm_loss = zero
        # The two networks' gradients are independent: the IDM's tape (0.5 ms at 256 samples) is enqueued FIRST, on a second stream, and runs next to
        # the planner's (csrc/train.hip keeps one workspace lane per module); the statistics scalars read inputs only and go to a third.  The
        # main stream waits for both before anything reads a gradient or a scalar.
        for net in trained.values():                                  # (a (re)load of a training state synchronises the device: before anything is in flight)
            self._train_sync(net.slot, getattr(self, f"{net.key}_state"), net.shapes(), eng=net.eng)
        eng = self._engine
        side = eng.aux_streams() if eng.get_option("train_streams") else {}
        idm_stream = side.get("idm") if (pn and im) else None
        stats_stream = side.get("stats")
        main = torch.cuda.current_stream(self._device) if side else None     # (no side stream: the step touches no stream at all)

        def on(stream):
            """Enqueue on a side stream, behind what the main stream holds so far -- or on the main stream itself."""
            if stream is None:
                return contextlib.nullcontext()
            stream.wait_stream(main)
            return torch.cuda.stream(stream)
        with on(stats_stream):
            stats = [eng.reduce_stats(obs_emb), eng.reduce_stats(action)] + [eng.reduce_stats(nb["obs"][k]) for k in nb["obs"]]
        # host draws in the reference's order of use (planner, then IDM), whatever the enqueue order below
        t_plan = timesteps(pn, rows_p, B) if pn else None
        if im:                                                        # idm_loss
            s, a = self._idm_pairs(emb_i, action_i)
            t_idm = timesteps(im, rows_i, Bi, a.shape[0] // Bi)       # one per transition
            eps = noise_of(im, a, rows_i, Bi)
            with on(idm_stream):                                      # (its inputs were written on the main stream)
                idm_loss = im.grad(s, a, eps, t_idm, weight(im, rows_i, Bi))
        if pn:                                                        # plan_loss
            nxt = self._planner_targets(obs_emb)
            eps = noise_of(pn, nxt, rows_p, B)
            cond = obs_emb[:, :oh].reshape(B, -1).contiguous()
            plan_loss = pn.grad(nxt, eps, t_plan, cond, weight(pn, rows_p, B))
        for st in (idm_stream, stats_stream):
            if st is not None:
                main.wait_stream(st)
        if shard is not None:                                         # data parallel: sum of the B / n weighted shard gradients = the global batch's
            import torch.distributed as tdist
            for net in trained.values():
                tdist.all_reduce(net.eng.train_arena(net.slot, net.eng.TRAIN_GRADS), group=shard.get("group"))
            both = torch.stack([plan_loss.reshape(()), idm_loss.reshape(())])
            tdist.all_reduce(both, group=shard.get("group"))
            plan_loss, idm_loss = both[0], both[1]
        new, m = {}, {}
        for key, off in (("planner", dict(planner_lr=0, planner_step=0, noise_diff=0)), ("idm", dict(idm_lr=0, idm_step=0))):
            net = trained.get(key)
            if net is None:
                m.update(off)
                continue
            st = getattr(self, f"{key}_state")
            net.eng.train_apply(net.slot, float(np.float32(self._lr_schedules[key](st.step))))
            m[f"{key}_lr"], m[f"{key}_step"] = np.float32(self.lr_schedule(st.step)), st.step     # the OLD state's step, the LAST-built schedule (:257-258)
            new[f"{key}_state"] = self._trained_state(net.slot, st, net.shapes(), eng=net.eng)
        # linear_algebra.global_norm(grads), :253 -- a metric only (nothing is clipped), taken after the optimiser launches, which leave the
        # per-stripe sums of squares of the gradients they consumed behind (one small launch instead of a second pass over the arenas): one
        # call per engine handle over the slots it trained; two handles' norms (LDPHierAgent) combine as sqrt(a^2 + b^2)
        handles = {}
        for net in trained.values():
            handles.setdefault(id(net.eng), (net.eng, []))[1].append(net.slot)
        norms = [e.train_grad_norm(slots) for e, slots in handles.values()]
        g_norm = zero if not norms else norms[0] if len(norms) == 1 else torch.sqrt(norms[0].double() ** 2 + norms[1].double() ** 2).float()
        arrs = [DeviceArray(x) for x in [plan_loss, idm_loss, g_norm] + stats]
        # (alpha_planner / alpha_idm are already inside the two device scalars: the gradients are those of the weighted losses)
        m.update(plan_loss=_HostScalar(lambda: arrs[0].numpy()), idm_loss=_HostScalar(lambda: arrs[1].numpy()),
                 loss=_HostScalar(lambda: arrs[0].numpy() + arrs[1].numpy()), g_norm=_HostScalar(lambda: arrs[2].numpy()))
        self._stat_metrics(m, "emb", arrs[3:], nb["obs"])
        return self.replace(**new), m

    # ---- agent/ldp_agent.py:113-180, 328-349: the training losses, FORWARD ONLY ---------------------------
    def get_metrics(self, batch, rng, noise=None):
        """`get_metrics_step`: postprocess_batch -> get_obs_cond -> plan_loss / idm_loss (add_noise at a random timestep per sample, ONE
        network evaluation each, MSE against the noise) -> the statistics scalars.  No gradient anywhere: this is the call eval_bc.py:127
        makes before its sampling metrics.  Keys as the reference's `loss` (:141-180): plan_loss, idm_loss, loss, emb_min / max / mean /
        std, action_min / max, `<obs key>_min` / `_max` for every key of the (normalised) batch.

        rng: seed of the timesteps (host PCG64) and of the noise (the device Philox primitive); JAX's threefry stream is a non-goal.
        noise: optional dict(t_plan (B,), noise_plan (B, T, D), t_idm (R,), noise_idm (R, A)) -- explicit inputs for parity runs."""
        cfg, eng = self.config, self._engine
        seed = _seed_of(rng)
        oh = cfg["obs_horizon"]
        nz = noise or {}

        def run():
            self._sync_weights()
            nb = self._postprocess(batch)                           # needs 'actions' like postprocess_batch (utils/data_utils.py:70-74)
            if "actions" not in nb:
                raise KeyError("get_metrics needs batch['actions'] (utils/data_utils.py:73)")
            obs_emb = self.get_obs_cond(nb["obs"]).contiguous()     # (the reference's loss reads pre-encoded latents: no vae_encode here)
            action = nb["actions"]
            B = obs_emb.shape[0]
            hg = np.random.Generator(np.random.PCG64(seed & (2**63 - 1)))
            plan_loss = idm_loss = None
            if self.use_planner:                                    # :113-127
                nxt = self._planner_targets(obs_emb)
                npl = int(cfg["planner_n_diffusion_steps"])
                t = nz.get("t_plan")
                t = torch.as_tensor(hg.integers(0, npl, size=B) if t is None else np.asarray(t)).to(self._device)
                eps = nz.get("noise_plan")
                eps = (self._t(eps) if eps is not None else
                       _philox_normal(seed, 0, 0, 7, nxt.numel(), self._device).reshape(nxt.shape))
                noisy = eng.add_noise(nxt, eps, t, npl)
                cond = obs_emb[:, :oh].reshape(B, -1).contiguous()
                pred = eng.unet_forward(noisy, t, cond)
                plan_loss = eng.mean_sq_diff(pred, eps)
            if self.use_idm:                                        # :129-140
                s, a = self._idm_pairs(obs_emb, action)
                nid = int(cfg["idm_n_diffusion_steps"])
                t = nz.get("t_idm")
                t = torch.as_tensor(hg.integers(0, nid, size=a.shape[0]) if t is None else np.asarray(t).reshape(-1)).to(self._device)
                eps = nz.get("noise_idm")
                eps = (self._t(eps) if eps is not None else
                       _philox_normal(seed, 0, 0, 8, a.numel(), self._device).reshape(a.shape))
                noisy = eng.add_noise(a, eps, t, nid)
                pred = self._idm_eps(s, noisy, t)
                idm_loss = eng.mean_sq_diff(pred, eps)
            zero = torch.zeros((), dtype=torch.float32, device=self._device)
            out = [zero if plan_loss is None else plan_loss, zero if idm_loss is None else idm_loss,
                   eng.reduce_stats(obs_emb), eng.reduce_stats(action)]
            out += [eng.reduce_stats(nb["obs"][k]) for k in nb["obs"]]
            return out
        res, rec = self._call(run)
        keys = list(self._postprocess_keys(batch))
        arrs = [DeviceArray(t, record=rec) for t in res]
        # the two mean-squared errors are device scalars; alpha_planner / alpha_idm and the sum (agent/ldp_agent.py:146-158) are applied in
        # float32 when a value is read
        ap, ai = np.float32(self.alpha_planner if self.use_planner else 0), np.float32(self.alpha_idm if self.use_idm else 0)
        m = dict(plan_loss=_HostScalar(lambda: ap * arrs[0].numpy()), idm_loss=_HostScalar(lambda: ai * arrs[1].numpy()),
                 loss=_HostScalar(lambda: ap * arrs[0].numpy() + ai * arrs[1].numpy()))
        self._stat_metrics(m, "emb", arrs[2:], keys)
        return m

    # what the two losses read of a training batch (LDPHierAgent overrides the three: strided targets, a U-Net IDM)
    def _planner_targets(self, obs_emb):
        return obs_emb[:, self.config["obs_horizon"]:].contiguous()                                       # agent/ldp_agent.py:117

    def _idm_pairs(self, obs_emb, action):
        oh = self.config["obs_horizon"]
        s = torch.cat([obs_emb[:, oh - 1:-1], obs_emb[:, oh:]], dim=-1)
        s = s.reshape(-1, s.shape[-1]).contiguous()                                                       # 'B H D -> (B H) D'
        a = action[:, :-1].reshape(-1, action.shape[-1]).contiguous()
        if a.shape[0] != s.shape[0]:
            raise ValueError(f"idm_loss pairs {s.shape[0]} transitions with {a.shape[0]} actions: the batch needs "
                             "actions.shape[1] - 1 == obs.shape[1] - obs_horizon (agent/ldp_agent.py:130-131)")
        return s, a

    def _idm_eps(self, s, noisy, t):
        return self._engine.idm_forward(s, noisy, t)

    @staticmethod
    def _postprocess_keys(batch):
        return batch["obs"].keys()
