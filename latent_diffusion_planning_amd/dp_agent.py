"""DPAgent -- the reference's diffusion-policy baseline on raw pixels (agent/dp_agent.py, the agent train_bc.yaml selects by default) on the
HIP engine, for evaluation.

One ResNet-18 image encoder per camera key (or one 'shared'; networks/resnet_v1.py with agent/encoder/bridge_resnet.yaml: GroupNorm(4),
ReLU, spatial-softmax pooling -> 1024 features per frame) in front of the ConditionalUnet1D that DPVAEAgent runs: the U-Net denoises a
(B, pred_horizon, action_dim) action chunk given obs_cond = [image features | low-dim].  Everything heavy runs in libldp_hip.so: the
encoders (ldp_resnet_encode, csrc/resnet.hip; one weight module encoder<i> of the handle per encoder), the sampling loop
(ldp_plan_sample), the un-normalisation of the action rows (ldp_normalize_bounds).  The condition is assembled with torch.cat on the device.

Same names, argument meaning and return structure as the reference class: `create`, `.config`, `.replace`, `.planner_state`,
`.encoder_state_dict`, `get_obs_cond`, `sample`, `sample_action`, `get_action`, `get_metrics`, `get_params`.  rng / noise conventions are
DPVAEAgent's (int seed, uint32[2] key or torch.Generator; explicit noise for parity runs).

Not built: the backward pass of the encoder, so `update` raises -- a dp_agent is trained with the reference and evaluated here
(checkpoint.load_snapshot restores `planner_params` and `encoder_params`).
"""
from __future__ import annotations

import copy
from typing import Optional

import numpy as np
import torch

from . import weights as W
from ._lib import RESNET_FEATURES, RESNET_SLOTS
from .agent import DPState, LDPAgent, _Elem, _EngineCalls, _get, _HostScalar, _norm_entry, _philox_normal, _seed_of
from .arrays import DeviceArray
from .engine import HipEngine

MAX_COND = 8192                       # columns dense_launch takes (csrc/kernels_misc.hip): the FiLM projection reads the whole condition row

# agent/encoder/bridge_resnet.yaml: the fields that change the arithmetic, and the only values built
ENCODER_FIELDS = dict(stage_sizes=[2, 2, 2, 2], block_cls="ResNetBlock", feature_layers=[], n_filters=64, dtype="float32", act="relu",
                      norm="group", add_spatial_coordinates=False, pooling_method="spatial_softmax", softmax_temperature=1.0,
                      use_multiplicative_cond=False, use_film=False, use_tanh=False, use_simnorm=False, use_simnorm_rescale=False,
                      use_sigmoid=False)


def _check_encoder_cfg(encoder) -> None:
    """Refuse an encoder yaml that differs from bridge_resnet.yaml in a field that changes the arithmetic.  (conv, use_spatial_softmax,
    n_spatial_blocks and simnorm_dim are not read on this configuration's path.)"""
    for k, want in ENCODER_FIELDS.items():
        got = _get(encoder, k, want)
        if isinstance(want, list):
            got = [int(v) for v in got] if got is not None else None
        if got != want:
            raise NotImplementedError(f"encoder.{k}={got!r}: the ResNet encoder is built for agent/encoder/bridge_resnet.yaml "
                                      f"({k}: {want!r})")


def dp_image_cond(feats, lowdim: torch.Tensor) -> torch.Tensor:
    """get_obs_cond (agent/dp_agent.py:31-52) from the encoders' outputs: feats = one (B, frames * 1024) block per encoder call, in
    rgb_obs order (shared: the one block); lowdim (B, oh, L) -> (B, G) = [image features | low-dim]."""
    B = lowdim.shape[0]
    return torch.cat([f.reshape(B, -1) for f in feats] + [lowdim.reshape(B, -1)], dim=-1).contiguous()


class DPAgent(_EngineCalls):
    def __init__(self, planner_state, encoder_state_dict, obs_normalization, config, engine: Optional[HipEngine], planner_spec, device,
                 lr_schedule=None):
        self.planner_state = planner_state
        self.encoder_state_dict = dict(encoder_state_dict)
        self.obs_normalization = obs_normalization
        self.config = config
        self._engine = engine
        self._planner_spec = planner_spec
        self._device = device
        self.lr_schedule = lr_schedule

    # ---------------------------------------------------------------------------------------------
    @classmethod
    def create(cls, rng, batch, shape_meta,
               # Hydra config (agent/dp_agent.yaml)
               name, planner, encoder, lowdim_obs, rgb_obs, obs_normalization,
               obs_horizon, pred_horizon, action_horizon, n_diffusion_steps,
               lr, end_lr, warmup_steps, decay_steps, shared_encoder,
               planner_ema_decay, encoder_ema_decay,
               device=None, exclusive_gpu=True):
        """agent/dp_agent.py:213-310.  `batch` is accepted for signature parity (the reference traces shapes from it)."""
        lowdim_obs, rgb_obs = list(lowdim_obs), list(rgb_obs)
        shared = bool(shared_encoder)
        _check_encoder_cfg(encoder)
        if not rgb_obs:
            raise NotImplementedError("rgb_obs is empty: DPAgent conditions on at least one camera")
        for k in rgb_obs:
            shp = tuple(int(v) for v in shape_meta["all_shapes"][k])
            if shp != (64, 64, 3):
                raise NotImplementedError(f"{k} frames are {shp}: the ResNet encoder is built for 64x64x3 frames")
        keys = ["shared"] if shared else rgb_obs
        if len(keys) > RESNET_SLOTS:
            raise NotImplementedError(f"{len(keys)} encoders: an engine handle holds at most {RESNET_SLOTS}")
        lowdim_dim = sum(int(np.prod(shape_meta["all_shapes"][k])) for k in lowdim_obs)
        # (the reference's vision_feature_dim = 512 * len(rgb_obs), :226, is never used: the FiLM Dense infers its width from obs_cond)
        G = int(obs_horizon) * (RESNET_FEATURES * len(rgb_obs) + lowdim_dim)
        if G > MAX_COND:
            raise NotImplementedError(f"the condition has {G} columns: the FiLM projection takes at most {MAX_COND}")
        action_dim = int(shape_meta["ac_dim"])
        if action_dim > 128:
            raise NotImplementedError(f"action_dim={action_dim}: the U-Net's first conv is packed for inputs of at most 128 features")
        down_dims = tuple(int(d) for d in _get(planner, "down_dims", (256, 512, 1024)))
        pspec = W.PlannerSpec(input_dim=action_dim, global_cond_dim=G,
                              diffusion_step_embed_dim=int(_get(planner, "diffusion_step_embed_dim", 256)),
                              down_dims=down_dims, kernel_size=int(_get(planner, "kernel_size", 5)),
                              n_groups=int(_get(planner, "n_groups", 8)), downsample=bool(_get(planner, "downsample", True)))
        if not pspec.downsample:
            raise NotImplementedError("downsample=False U-Nets are not built")
        if any(d < 256 or d % 128 for d in down_dims) or pspec.kernel_size != 5 or pspec.n_groups != 8:
            raise NotImplementedError(f"planner down_dims={down_dims} kernel_size={pspec.kernel_size} n_groups="
                                      f"{pspec.n_groups}: the MFMA conv tiles are built for kernel_size 5, 8 groups and "
                                      "levels that are multiples of 128 channels and at least 256 wide")
        T = int(pred_horizon)
        if T % (1 << (len(down_dims) - 1)) != 0:
            raise ValueError(f"pred_horizon {T}: the {len(down_dims)}-level ConditionalUnet1D needs a multiple of {1 << (len(down_dims) - 1)}")
        if not 1 <= int(action_horizon) <= T:
            raise ValueError(f"action_horizon {action_horizon} must lie in 1..pred_horizon {T}")
        seed = _seed_of(rng)
        planner_state = DPState(W.init_planner_params(pspec, seed=seed * 3 + 1, perturb=False), None, ema_is_params=True)
        enc_states = {k: DPState(W.init_resnet_params(W.ResNetSpec(), seed=seed * 3 + 2 + i, perturb=False), None, ema_is_params=True)
                      for i, k in enumerate(keys)}                       # TrainStateEMA.create(..., ema_params=params), :262-268
        config = dict(n_diffusion_steps=int(n_diffusion_steps), lowdim_obs=lowdim_obs, rgb_obs=rgb_obs, obs_horizon=int(obs_horizon),
                      name=name, action_dim=action_dim, pred_horizon=T, action_horizon=int(action_horizon), shared_encoder=shared)
        norm = {"obs": {k: _norm_entry(v) for k, v in dict(obs_normalization["obs"]).items()}}
        if "actions" in obs_normalization:
            norm["actions"] = _norm_entry(obs_normalization["actions"])
        if not torch.cuda.is_available():
            from ._lib import LDPHipUnavailable
            raise LDPHipUnavailable("no HIP device visible: DPAgent has no CPU fallback")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        engine = HipEngine(obs_dim=action_dim, action_dim=action_dim, global_cond_dim=G, pred_horizon=T, action_horizon=int(action_horizon),
                           down_dims=down_dims, kernel_size=pspec.kernel_size, n_groups=pspec.n_groups,
                           step_embed_dim=pspec.diffusion_step_embed_dim, planner_train_steps=int(n_diffusion_steps),
                           idm_train_steps=int(n_diffusion_steps), image_size=0, device=dev)
        if not exclusive_gpu:
            engine.set_option("safe_mode", 1)
        from .schedule import warmup_cosine_decay_schedule
        sched = None
        if lr is not None and warmup_steps is not None and decay_steps is not None:
            sched = warmup_cosine_decay_schedule(float(end_lr), float(lr), int(warmup_steps), int(decay_steps), float(end_lr))
        return cls(planner_state, enc_states, norm, config, engine, pspec, dev, lr_schedule=sched)

    # ---------------------------------------------------------------------------------------------
    def _encoder_keys(self):
        return ["shared"] if self.config["shared_encoder"] else list(self.config["rgb_obs"])

    def replace(self, **fields):
        """flax.struct `.replace`: a shallow copy sharing the engine (weights re-upload lazily, only the trees whose token changed)."""
        new = copy.copy(self)
        for k, v in fields.items():
            if k not in ("planner_state", "encoder_state_dict", "obs_normalization"):
                raise AttributeError(f"DPAgent has no field {k!r}")
            if k == "encoder_state_dict":
                v = dict(v)
                missing = [e for e in self._encoder_keys() if e not in v]
                if missing:
                    raise KeyError(f"encoder_state_dict lacks {missing} (this agent's encoders: {self._encoder_keys()})")
            setattr(new, k, v)
        return new

    def get_params(self):
        """agent/dp_agent.py:207-211.  The reference returns the encoder PARAMETERS again under `encoder_ema_params` (it builds
        encoder_ema_params_dict and then does not use it): kept, so that a snapshot written here holds what one written there holds."""
        enc = {f"{k}_params": self.encoder_state_dict[k].params for k in self.encoder_state_dict}
        return dict(planner_params=self.planner_state.params, encoder_params=enc,
                    planner_ema_params=self.planner_state.ema_params, encoder_ema_params=enc)

    def _planner_shapes(self):
        return W.planner_shapes(self._planner_spec)

    def _sync_weights(self):
        """Upload what the engine does not hold for THIS agent: the U-Net, and every encoder whose version token changed (slot i = the
        i-th encoder key).  sample / get_metrics run on the PARAMETERS, never the EMA (:163-164, :201-202)."""
        eng = self._engine
        tree = self._slot_weights(eng, "planner", self.planner_state, self._planner_shapes)
        if tree is not None:
            eng.load_params(planner=tree, versions={"planner": self.planner_state.version})
        for i, k in enumerate(self._encoder_keys()):
            st = self.encoder_state_dict[k]
            if eng.loaded[f"encoder{i}"] != st.version:
                W.check_resnet_params(st.params)
                eng.load_encoder(i, st.params, version=st.version)

    _postprocess = LDPAgent._postprocess          # postprocess_batch / postprocess_batch_obs selection (:142-146)
    _action_bounds = LDPAgent._action_bounds

    # ---- agent/dp_agent.py:31-52 ------------------------------------------------------------------
    def _frames(self, v) -> torch.Tensor:
        x = self._t(v)[:, :self.config["obs_horizon"]]
        if tuple(x.shape[-3:]) != (64, 64, 3):
            raise ValueError(f"camera frames must be (B, H, 64, 64, 3), got {tuple(x.shape)}")
        return x

    def get_obs_cond(self, batch):
        """(B, G) = [image features | low-dim] from a NORMALISED observation dict (frames in [-1, 1]), on the device."""
        cfg, eng = self.config, self._engine
        oh = cfg["obs_horizon"]
        lowdim = torch.cat([self._t(batch[k])[:, :oh] for k in cfg["lowdim_obs"]], dim=-1)
        if cfg["shared_encoder"]:
            x = torch.cat([self._frames(batch[k]) for k in cfg["rgb_obs"]], dim=1)
            feats = [eng.resnet_encode(0, x.reshape(-1, 64, 64, 3))]
        else:
            feats = [eng.resnet_encode(i, self._frames(batch[k]).reshape(-1, 64, 64, 3)) for i, k in enumerate(cfg["rgb_obs"])]
        return dp_image_cond(feats, lowdim)

    # ---- agent/dp_agent.py:141-190 ----------------------------------------------------------------
    def sample(self, batch, eval_rng, noise=None, row_offset=0, sampler="ddpm", n_steps=None):
        """-> (action (B, action_horizon, A) un-normalised, metrics: obs_min / obs_max / obs_mean / obs_std of obs_cond and <key>_min /
        <key>_max of every normalised observation key).  noise: optional dict(x_init (B, T, A), x_noise (S, B, T, A)) for explicit-noise
        parity runs; row_offset: global index of the first row (the Philox stream of a row does not depend on sharding)."""
        seed = _seed_of(eval_rng)
        cfg, eng = self.config, self._engine
        nz = noise or {}
        keys = list(batch["obs"].keys())

        def run():
            self._sync_weights()
            nb = self._postprocess(batch)
            cond = self.get_obs_cond(nb["obs"])
            x = eng.plan_sample(cond, x_init=nz.get("x_init"), step_noise=nz.get("x_noise"), seed=seed, row_offset=row_offset,
                                sampler=sampler, n_steps=n_steps)
            lo, hi, mode = self._action_bounds()
            act = eng.normalize_bounds(x[:, :cfg["action_horizon"]].contiguous(), lo, hi, mode)
            return [act, eng.reduce_stats(cond)] + [eng.reduce_stats(nb["obs"][k]) for k in keys]
        res, rec = self._call(run)
        arrs = [DeviceArray(x, record=rec) for x in res]
        m = {f"obs_{s}": _Elem(arrs[1], i) for i, s in enumerate(("min", "max", "mean", "std"))}
        for j, k in enumerate(keys):
            m[f"{k}_min"], m[f"{k}_max"] = _Elem(arrs[2 + j], 0), _Elem(arrs[2 + j], 1)
        return arrs[0], m

    def sample_action(self, batch, rng, **kw):
        """agent/dp_agent.py:138-139."""
        return self.sample(batch, rng, **kw)

    def get_action(self, batch, eval_rng, **kw):
        return self.sample(batch, eval_rng, **kw)[0]

    # ---- agent/dp_agent.py:192-205 ----------------------------------------------------------------
    def get_metrics(self, batch, rng, noise=None):
        """loss's metrics, forward only: obs_min / obs_max / obs_mean / obs_std of obs_cond and
        loss = mean((unet(add_noise(a, noise, t), t, obs_cond) - noise)^2).  noise: optional dict(t (B,), noise (B, T, A))."""
        cfg, eng = self.config, self._engine
        seed = _seed_of(rng)
        nz = noise or {}

        def run():
            self._sync_weights()
            nb = self._postprocess(batch)
            if "actions" not in nb:
                raise KeyError("get_metrics needs batch['actions'] (utils/data_utils.py:73)")
            cond = self.get_obs_cond(nb["obs"])
            action = nb["actions"].contiguous()
            B = action.shape[0]
            if tuple(action.shape[1:]) != (cfg["pred_horizon"], cfg["action_dim"]):
                raise ValueError(f"batch['actions'] has shape {tuple(action.shape)}: the U-Net denoises (B, pred_horizon="
                                 f"{cfg['pred_horizon']}, action_dim={cfg['action_dim']}) chunks")
            hg = np.random.Generator(np.random.PCG64(seed & (2**63 - 1)))
            npl = int(cfg["n_diffusion_steps"])
            t = nz.get("t")
            t = torch.as_tensor(hg.integers(0, npl, size=B) if t is None else np.asarray(t)).to(self._device)
            eps = nz.get("noise")
            eps = self._t(eps) if eps is not None else _philox_normal(seed, 0, 0, 7, action.numel(), self._device).reshape(action.shape)
            pred = eng.unet_forward(eng.add_noise(action, eps, t, npl), t, cond)
            return [eng.mean_sq_diff(pred, eps), eng.reduce_stats(cond)]
        res, rec = self._call(run)
        arrs = [DeviceArray(x, record=rec) for x in res]
        m = {f"obs_{s}": _Elem(arrs[1], i) for i, s in enumerate(("min", "max", "mean", "std"))}
        m["loss"] = _HostScalar(lambda: arrs[0].numpy())
        return m

    # ---- what is not built / does not exist on the reference's class ---------------------------------
    def update(self, *a, **k):
        raise NotImplementedError("DPAgent.update: the backward pass of the ResNet encoder is not built; a dp_agent is trained with the "
                                  "reference and evaluated here (checkpoint.load_snapshot restores planner_params and encoder_params)")

    def sample_viz(self, *a, **k):
        raise NotImplementedError("DPAgent has no sample_viz (agent/dp_agent.py samples actions only)")

    def sample_warm(self, *a, **k):
        raise NotImplementedError("sample_warm is built for LDPAgent only (a DP agent denoises actions, which do not shift with the world like a latent plan)")

    def replanner(self, *a, **k):
        raise NotImplementedError("replanner is built for LDPAgent only (a DP agent denoises actions, which do not shift with the world like a latent plan)")

    def sample_guided(self, *a, **k):
        raise NotImplementedError("sample_guided is built for LDPAgent only (its costs are stated on latent plans; a DP agent denoises actions)")

    def build_guide(self, *a, **k):
        raise NotImplementedError("build_guide is built for LDPAgent only (its costs are stated on latent plans; a DP agent denoises actions)")

    def plan(self, *a, **k):
        raise NotImplementedError("plan is built for LDPAgent only (its parts are stated on latent plans; a DP agent denoises actions)")

    def controller(self, *a, **k):
        raise NotImplementedError("controller is built for LDPAgent only (its parts are stated on latent plans; a DP agent denoises actions)")

    def sample_action_from_plan(self, *a, **k):
        raise NotImplementedError("DPAgent has no sample_action_from_plan")

    def update_mixed(self, *a, **k):
        raise NotImplementedError("DPAgent has no update_mixed")
