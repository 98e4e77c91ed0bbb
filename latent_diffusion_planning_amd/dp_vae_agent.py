"""DPVAEAgent -- the reference's baseline (agent/dp_repr_agent.py, hydra target agent.dp_vae_agent.DPVAEAgent) on the HIP engine.

A diffusion policy over ACTIONS conditioned on frozen StableVAE latents: one ConditionalUnet1D (input_dim = action_dim) denoises a
(B, pred_horizon, A) action chunk given the observation condition of `get_obs_cond`.  Everything heavy runs in libldp_hip.so: the
StableVAE encoder (ldp_vae_encode), the sampling loop with its condition gather and action un-normalisation as one call / one captured
graph (ldp_policy_sample), the exact-fp32 training tape of the U-Net (ldp_train_planner_grad) and Adam with the parameter EMA fused into the
same launch (ldp_train_ema / ldp_train_apply).

Same names, argument meaning and return structure as the reference class: `create`, `.config`, `.replace`, `.planner_state` (`.params`,
`.ema_params`, `.step`, `.replace(params=, ema_params=)`), `vae_encode`, `vae_decode`, `get_obs_cond`, `sample`, `update`, `get_metrics`,
`get_params`.  rng / noise conventions are LDPAgent's (int seed, uint32[2] key or torch.Generator; explicit noise for parity runs).

Like LDPAgent, only the NEWEST trained state's parameters and EMA can be read back (both stay in the engine's arenas until fetched): keep
`agent = agent.update(...)[0]` as train_bc.py:107 does.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import weights as W
from .agent import (LATENT_SHAPES, DPState, LDPAgent, _HostScalar, _as_flat, _get, _norm_entry, _philox_normal, _seed_of,   # noqa: F401
                    load_pretrained_vae)                 # (DPState, this agent's state class, is defined next to ParamState)
from .arrays import DeviceArray
from .engine import HipEngine


def dp_obs_cond(frame_emb: torch.Tensor, obs_horizon: int, img_width: int) -> torch.Tensor:
    """get_obs_cond (agent/dp_repr_agent.py:76-85) from per-frame [image latent | low-dim] rows (B, H, E): the image features of frames
    0..oh-1 first, then their low-dim vectors -> (B, oh * E)."""
    x = frame_emb[:, :obs_horizon]
    B = x.shape[0]
    return torch.cat([x[..., :img_width].reshape(B, -1), x[..., img_width:].reshape(B, -1)], dim=-1).contiguous()


class DPVAEAgent(LDPAgent):
    """The fault protocol (_record / _guarded), pre/post-processing and the VAE calls are LDPAgent's; the planner slot of the engine holds
    the action U-Net."""

    def __init__(self, planner_state, vae_params, obs_normalization, config, engine: Optional[HipEngine], planner_spec, vae_spec, device,
                 lr_schedule=None):
        super().__init__(planner_state, None, vae_params, obs_normalization, True, False, 1, 0, config, engine, planner_spec, None,
                         vae_spec, device, lr_schedules={"planner": lr_schedule} if lr_schedule is not None else None)

    # ---------------------------------------------------------------------------------------------
    @classmethod
    def create(cls, rng, batch, shape_meta,
               # Hydra config (agent/dp_repr_agent.yaml)
               name, planner, lowdim_obs, rgb_obs, obs_normalization,
               obs_horizon, pred_horizon, action_horizon, n_diffusion_steps,
               lr, end_lr, warmup_steps, decay_steps,
               random_shift, use_ema, planner_ema_decay,
               vae_pretrain_path, vae_feature_dim,
               device=None, vae_params=None, exclusive_gpu=True):
        """agent/dp_repr_agent.py:225-307.  `batch` is accepted for signature parity (the reference traces shapes from it)."""
        lowdim_obs, rgb_obs = list(lowdim_obs), list(rgb_obs)
        if len(rgb_obs) != 1:
            raise NotImplementedError(f"rgb_obs={rgb_obs}: the DP condition is built for exactly one camera (multi-camera "
                                      "conditioning is not built)")
        if vae_feature_dim is None or int(vae_feature_dim) not in LATENT_SHAPES:
            raise NotImplementedError(f"vae_feature_dim={vae_feature_dim}: the latent shapes of agent/dp_repr_agent.py:56-69 are "
                                      f"{sorted(LATENT_SHAPES)} (2x2x4, 2x2x8, 3x3x4, 4x4x4)")
        side, latent_ch = LATENT_SHAPES[int(vae_feature_dim)]
        image_size = 32 * side
        lowdim_dim = sum(int(np.prod(shape_meta["all_shapes"][k])) for k in lowdim_obs)
        obs_dim = lowdim_dim + int(vae_feature_dim) * len(rgb_obs)         # per frame (:236-239)
        action_dim = int(shape_meta["ac_dim"])
        if action_dim > 128:
            raise NotImplementedError(f"action_dim={action_dim}: the U-Net's first conv is packed for inputs of at most 128 features")
        down_dims = tuple(int(d) for d in _get(planner, "down_dims", (256, 512, 1024)))
        pspec = W.PlannerSpec(input_dim=action_dim, global_cond_dim=int(obs_horizon) * obs_dim,   # Dense infers the width it is fed
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
        decay = float(planner_ema_decay)
        if not 0.0 <= decay <= 1.0:
            raise ValueError(f"planner_ema_decay={decay} must lie in [0, 1]")
        seed = _seed_of(rng)
        params = W.init_planner_params(pspec, seed=seed * 3 + 1, perturb=False)
        planner_state = DPState(params, None, ema_is_params=True)           # TrainStateEMA.create(..., ema_params=params)
        if vae_params is None and vae_pretrain_path is not None:
            vae_params = load_pretrained_vae(str(vae_pretrain_path))
        vae_params = _as_flat(vae_params) if vae_params is not None else None
        config = dict(n_diffusion_steps=int(n_diffusion_steps), lowdim_obs=lowdim_obs, rgb_obs=rgb_obs, obs_horizon=int(obs_horizon),
                      name=name, action_dim=action_dim, pred_horizon=T, action_horizon=int(action_horizon),
                      random_shift=random_shift, use_ema=bool(use_ema), vae_feature_dim=int(vae_feature_dim),
                      obs_dim=obs_dim, planner_ema_decay=decay)
        norm = {"obs": {k: _norm_entry(v) for k, v in dict(obs_normalization["obs"]).items()}}
        if "actions" in obs_normalization:
            norm["actions"] = _norm_entry(obs_normalization["actions"])
        if not torch.cuda.is_available():
            from ._lib import LDPHipUnavailable
            raise LDPHipUnavailable("no HIP device visible: DPVAEAgent has no CPU fallback")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        engine = HipEngine(obs_dim=action_dim, action_dim=action_dim, global_cond_dim=pspec.global_cond_dim, pred_horizon=T,
                           action_horizon=int(action_horizon), down_dims=down_dims, kernel_size=pspec.kernel_size, n_groups=pspec.n_groups,
                           step_embed_dim=pspec.diffusion_step_embed_dim, planner_train_steps=int(n_diffusion_steps),
                           idm_train_steps=int(n_diffusion_steps), image_size=image_size, vae_latent_channels=latent_ch, device=dev)
        if not exclusive_gpu:
            engine.set_option("safe_mode", 1)
        from .schedule import warmup_cosine_decay_schedule
        sched = None
        if lr is not None and warmup_steps is not None and decay_steps is not None:
            sched = warmup_cosine_decay_schedule(float(end_lr), float(lr), int(warmup_steps), int(decay_steps), float(end_lr))
        return cls(planner_state, vae_params, norm, config, engine, pspec, W.VAESpec(latent_channels=latent_ch), dev, lr_schedule=sched)

    # ---------------------------------------------------------------------------------------------
    def get_params(self):
        """agent/dp_repr_agent.py:220-223."""
        return dict(planner_params=self.planner_state.params, planner_ema_params=self.planner_state.ema_params)

    # the hand-off between planner_state and the engine is LDPAgent's: sampling with the EMA when use_ema (:176-179), training with one
    _sample_ema = property(lambda self: bool(self.config["use_ema"]))
    _ema_decay = property(lambda self: self.config["planner_ema_decay"])

    # ---- agent/dp_repr_agent.py:76-85 ---------------------------------------------------------------
    def _frame_emb(self, obs) -> torch.Tensor:
        """Per-frame [image latent | low-dim] rows (B, H, E): what LDPAgent.get_obs_cond builds for one camera."""
        return LDPAgent.get_obs_cond(self, obs).contiguous()

    def get_obs_cond(self, batch):
        """(B, obs_horizon * E) in the DP layout: the image latents of frames 0..oh-1, then their low-dim vectors."""
        return dp_obs_cond(self._frame_emb(batch), self.config["obs_horizon"], self.config["vae_feature_dim"])

    # ---- agent/dp_repr_agent.py:160-201 -------------------------------------------------------------
    def sample(self, batch, eval_rng, noise=None, row_offset=0, sampler="ddpm", n_steps=None):
        """-> (action (B, action_horizon, A) un-normalised, {}).  noise: optional dict(x_init (B, T, A), x_noise (S, B, T, A)) for
        explicit-noise parity runs; row_offset: global index of the first row (the Philox stream of a row does not depend on sharding)."""
        seed = _seed_of(eval_rng)
        cfg = self.config
        nz = noise or {}

        def run():
            self._sync_weights()
            nb = self._postprocess(batch)
            obs = self._vae_encode_t(nb["obs"])
            lo, hi, mode = self._action_bounds()
            return [self._engine.policy_sample(self._frame_emb(obs), cfg["obs_horizon"], cfg["vae_feature_dim"], x_init=nz.get("x_init"),
                                               x_noise=nz.get("x_noise"), seed=seed, row_offset=row_offset, sampler=sampler,
                                               n_steps=n_steps, action_bounds=(lo, hi), action_mode=mode)]
        res, rec = self._call(run)
        return DeviceArray(res[0], record=rec), {}

    def get_action(self, batch, eval_rng, **kw):
        return self.sample(batch, eval_rng, **kw)[0]

    # the LDP-only surface does not exist on the reference's DP class
    def sample_viz(self, *a, **k):
        raise NotImplementedError("DPVAEAgent has no sample_viz (agent/dp_repr_agent.py samples actions only)")

    def sample_action(self, *a, **k):
        raise NotImplementedError("DPVAEAgent has no sample_action (eval_bc.py:129-131 calls sample for dp agents)")

    def sample_action_from_plan(self, *a, **k):
        raise NotImplementedError("DPVAEAgent has no sample_action_from_plan")

    def sample_warm(self, *a, **k):
        raise NotImplementedError("sample_warm is built for LDPAgent only (a DP agent denoises actions, which do not shift with the world like a latent plan)")

    def replanner(self, *a, **k):
        raise NotImplementedError("replanner is built for LDPAgent only (a DP agent denoises actions, which do not shift with the world like a latent plan)")

    def sample_best_of(self, *a, **k):
        raise NotImplementedError("sample_best_of is built for LDPAgent only (it scores latent plans; a DP agent samples actions)")

    def sample_guided(self, *a, **k):
        raise NotImplementedError("sample_guided is built for LDPAgent only (its costs are stated on latent plans; a DP agent denoises actions)")

    def build_guide(self, *a, **k):
        raise NotImplementedError("build_guide is built for LDPAgent only (its costs are stated on latent plans; a DP agent denoises actions)")

    def plan(self, *a, **k):
        raise NotImplementedError("plan is built for LDPAgent only (its parts are stated on latent plans; a DP agent denoises actions)")

    def controller(self, *a, **k):
        raise NotImplementedError("controller is built for LDPAgent only (its parts are stated on latent plans; a DP agent denoises actions)")

    def update_mixed(self, *a, **k):
        raise NotImplementedError("DPVAEAgent has no update_mixed")

    # ---- agent/dp_repr_agent.py:101-158: the training step ------------------------------------------------------------------------------
    def _gates(self, step):
        """update() trains the U-Net on every step (no gating, :135-144): (use_planner, use_idm) for dist.update_sharded."""
        return True, False

    def update(self, batch, rng, step, noise=None):
        """-> (new agent, metrics): jax.grad(loss), one optax.adam step, then the EMA (:146-158) -- csrc/train.hip, one fused launch for
        Adam and the EMA.  rng: seed of the timesteps (host PCG64) and of the noise (device Philox); noise: optional explicit
        dict(t (B,), noise (B, T, A)) for parity runs."""
        if self.config.get("random_shift", 0) and float(self.config["random_shift"]) > 0:
            raise NotImplementedError("random_shift > 0 shifts the rgb keys as raw (B, T, H, W, C) images (agent/dp_repr_agent.py:135-144); "
                                      "a latent training batch holds none")
        return self._update_step(batch, None, rng, True, False, noise)

    def _update_step(self, batch, mixed_batch, rng, use_planner, use_idm, noise, shard=None):
        """shard (dist.update_sharded): dict(group, rows=(lo, n)) -- `batch` holds rows [lo, lo + B) of a global batch of n: global-row
        timesteps and noise, a B / n weighted loss, ONE all-reduce of the gradient arena, Adam and the EMA replicated."""
        if mixed_batch is not None or use_idm:
            raise NotImplementedError("DPVAEAgent trains one network on one batch")
        if self._lr_schedules.get("planner") is None:
            raise ValueError("update() needs the optimiser settings of DPVAEAgent.create (lr, end_lr, warmup_steps, decay_steps)")
        cfg, eng = self.config, self._engine
        seed = _seed_of(rng)
        nz = noise or {}
        nb = self._postprocess(batch)
        if "actions" not in nb:
            raise KeyError("update needs batch['actions'] (utils/data_utils.py:73)")
        cond = self.get_obs_cond(nb["obs"])
        action = nb["actions"].contiguous()
        B, T, A = action.shape
        if T != cfg["pred_horizon"] or A != cfg["action_dim"]:
            raise ValueError(f"batch['actions'] has shape {tuple(action.shape)}: the U-Net denoises (B, pred_horizon={cfg['pred_horizon']}, "
                             f"action_dim={cfg['action_dim']}) chunks (agent/dp_repr_agent.py:102-110)")
        lo, n = (0, B) if shard is None else shard["rows"]
        w = np.float32(B) / np.float32(n)
        st = self.planner_state
        self._train_sync("planner", st, self._planner_shapes())
        stats = [eng.reduce_stats(cond), eng.reduce_stats(action)] + [eng.reduce_stats(nb["obs"][k]) for k in nb["obs"]]
        hg = np.random.Generator(np.random.PCG64(seed & (2**63 - 1)))
        t = nz.get("t")
        t = np.asarray(hg.integers(0, int(cfg["n_diffusion_steps"]), size=n) if t is None else t).reshape(-1)
        if len(t) == n and n != B:
            t = t[lo:lo + B]
        eps = nz.get("noise")
        if eps is not None:
            eps = self._t(eps[lo:lo + B] if len(eps) == n and n != B else eps)
        else:
            eps = _philox_normal(seed, lo * T * A, 0, 7, action.numel(), self._device).reshape(action.shape)
        loss = eng.train_planner_grad(action, eps, t, cond, float(w))
        if shard is not None:
            import torch.distributed as tdist
            tdist.all_reduce(eng.train_arena("planner", eng.TRAIN_GRADS), group=shard.get("group"))
            loss = loss.reshape(1).clone()
            tdist.all_reduce(loss, group=shard.get("group"))
            loss = loss.reshape(())
        sched = self._lr_schedules["planner"]
        eng.train_apply("planner", float(np.float32(sched(st.step))))            # Adam + EMA, one launch
        new_state = self._trained_state("planner", st, self._planner_shapes())
        arrs = [DeviceArray(loss)] + [DeviceArray(x) for x in stats]
        m = dict(loss=_HostScalar(lambda: arrs[0].numpy()))
        self._stat_metrics(m, "obs", arrs[1:], nb["obs"], n=4)
        m["planner_lr"], m["planner_step"] = np.float32(sched(st.step)), st.step       # the OLD state's step (:156-157)
        return self.replace(planner_state=new_state), m

    # ---- agent/dp_repr_agent.py:203-218 -------------------------------------------------------------
    def get_metrics(self, batch, rng, noise=None):
        """The loss, forward only, with the parameters or (use_ema) their EMA, and the statistics scalars of `loss` (:101-133).
        noise: optional dict(t (B,), noise (B, T, A))."""
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
            hg = np.random.Generator(np.random.PCG64(seed & (2**63 - 1)))
            npl = int(cfg["n_diffusion_steps"])
            t = nz.get("t")
            t = torch.as_tensor(hg.integers(0, npl, size=B) if t is None else np.asarray(t)).to(self._device)
            eps = nz.get("noise")
            eps = self._t(eps) if eps is not None else _philox_normal(seed, 0, 0, 7, action.numel(), self._device).reshape(action.shape)
            pred = eng.unet_forward(eng.add_noise(action, eps, t, npl), t, cond)
            out = [eng.mean_sq_diff(pred, eps), eng.reduce_stats(cond), eng.reduce_stats(action)]
            return out + [eng.reduce_stats(nb["obs"][k]) for k in nb["obs"]]
        res, rec = self._call(run)
        arrs = [DeviceArray(x, record=rec) for x in res]
        m = dict(loss=_HostScalar(lambda: arrs[0].numpy()))
        self._stat_metrics(m, "obs", arrs[1:], batch["obs"].keys(), n=4)
        return m
