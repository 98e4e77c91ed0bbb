"""DPTrainAgent -- DPAgent (the reference's raw-pixel diffusion policy, agent/dp_agent.py) with its training step on the HIP engine.

`update` is agent/dp_agent.py:112-136: jax.grad(loss) w.r.t. the U-Net AND every image encoder, one optax.adam step per state at that
state's own schedule value, then the EMA of each.  On the GPU: the encoders' training forward (ldp_train_encoder_forward, every
activation kept), the U-Net tape with the gradient of the condition (ldp_train_planner_grad_cond), the inverse of the condition layout,
the encoders' backward (ldp_train_encoder_backward), and Adam + EMA in one launch per module (ldp_train_apply).  The encoders are the
engine's training modules "encoder<i>" (slot i = the i-th encoder key, "shared" = slot 0).

A subclass, not a change of DPAgent: the evaluation class stays byte for byte what it is (its `update` keeps raising, its nine config keys
stay), and everything it does -- sample, get_metrics, get_params, replace, snapshots -- works on trained states here.  `planner_ema_decay`
and `encoder_ema_decay` are attributes, not config keys.  Like every trainable class here, only the NEWEST trained state can be read back.
"""
from __future__ import annotations

import numpy as np
import torch

from . import weights as W
from .agent import _Elem, _HostScalar, _philox_normal, _seed_of
from .arrays import DeviceArray
from .dp_agent import DPAgent, dp_image_cond
from ._lib import RESNET_FEATURES, RESNET_TRAIN_MAX_FRAMES


def dp_image_cond_inverse(dcond: torch.Tensor, frames):
    """The inverse of dp_image_cond on a gradient: dcond (B, G) -> one (B * frames[i], 1024) block per encoder call, in the order the
    calls fed the condition; the low-dim columns behind them have no parameters and are dropped."""
    B, out, off = dcond.shape[0], [], 0
    for f in frames:
        w = int(f) * RESNET_FEATURES
        out.append(dcond[:, off:off + w].reshape(B * int(f), RESNET_FEATURES).contiguous())
        off += w
    return out


class DPTrainAgent(DPAgent):
    planner_ema_decay = None
    encoder_ema_decay = None
    _ema_decay = property(lambda self: self.planner_ema_decay)      # (_trained_state: every state of this class carries an EMA)

    @classmethod
    def create(cls, rng, batch, shape_meta, name, planner, encoder, lowdim_obs, rgb_obs, obs_normalization, obs_horizon, pred_horizon,
               action_horizon, n_diffusion_steps, lr, end_lr, warmup_steps, decay_steps, shared_encoder, planner_ema_decay,
               encoder_ema_decay, device=None, exclusive_gpu=True):
        """agent/dp_agent.py:213-310 -- DPAgent.create's signature; the two EMA decays are kept (TrainStateEMA.create, :262-268)."""
        decays = dict(planner_ema_decay=float(planner_ema_decay), encoder_ema_decay=float(encoder_ema_decay))
        for k, v in decays.items():
            if not 0.0 <= v <= 1.0:
                raise ValueError(f"{k}={v} must lie in [0, 1]")
        ag = super().create(rng, batch, shape_meta, name, planner, encoder, lowdim_obs, rgb_obs, obs_normalization, obs_horizon,
                            pred_horizon, action_horizon, n_diffusion_steps, lr, end_lr, warmup_steps, decay_steps, shared_encoder,
                            planner_ema_decay, encoder_ema_decay, device=device, exclusive_gpu=exclusive_gpu)
        ag.planner_ema_decay, ag.encoder_ema_decay = decays["planner_ema_decay"], decays["encoder_ema_decay"]
        return ag

    @property
    def _lr_schedules(self):
        """One warm-up-cosine schedule per state (agent/dp_agent.py:254-281): the same settings, each read at its own state's step."""
        return None if self.lr_schedule is None else {k: self.lr_schedule for k in ["planner"] + self._encoder_keys()}

    def _encoder_shapes(self):
        return W.resnet_shapes()

    def _sync_weights(self):
        """DPAgent's, except that an encoder an update() left in the training arenas is published on the device (_slot_weights) instead
        of passing through the host."""
        eng = self._engine
        tree = self._slot_weights(eng, "planner", self.planner_state, self._planner_shapes)
        if tree is not None:
            eng.load_params(planner=tree, versions={"planner": self.planner_state.version})
        for i, k in enumerate(self._encoder_keys()):
            st = self.encoder_state_dict[k]
            tree = self._slot_weights(eng, f"encoder{i}", st, self._encoder_shapes)
            if tree is not None:
                eng.load_encoder(i, tree, version=st.version)

    def _encoder_frames(self, obs):
        """What each encoder is applied to (agent/dp_agent.py:36-37, :43-44): one (B * frames, 64, 64, 3) block per encoder key."""
        cfg = self.config
        if cfg["shared_encoder"]:
            return [torch.cat([self._frames(obs[k]) for k in cfg["rgb_obs"]], dim=1).reshape(-1, 64, 64, 3)]
        return [self._frames(obs[k]).reshape(-1, 64, 64, 3) for k in cfg["rgb_obs"]]

    # ---- agent/dp_agent.py:112-136 ------------------------------------------------------------------
    def _gates(self, step):
        """update() trains the U-Net and the encoders on every step: (use_planner, use_idm) for dist.update_sharded."""
        return True, False

    def update(self, batch, rng, step, noise=None):
        """-> (new agent, metrics).  rng: seed of the timesteps (host PCG64) and of the noise (device Philox stream 7), as
        DPVAEAgent.update; noise: optional explicit dict(t (B,), noise (B, T, A)) for parity runs.  metrics: loss, obs_min / obs_max /
        obs_mean / obs_std of obs_cond, planner_lr / planner_step and enc_<key>_lr / enc_<key>_step (the OLD states' counts, :128-135)."""
        return self._update_step(batch, None, rng, True, False, noise)

    def _update_step(self, batch, mixed_batch, rng, use_planner, use_idm, noise, shard=None):
        """shard (dist.update_sharded): dict(group, rows=(lo, n)) -- `batch` holds rows [lo, lo + B) of a global batch of n: timesteps and
        noise of the global rows, the U-Net's loss weighted B / n (its condition gradient, and so the encoders' backward, carry the
        weight), ONE all-reduce of the gradient arena per trained module (the U-Net and every encoder slot) and of the loss, Adam and
        the EMAs replicated.  The obs_* statistics describe this rank's rows; the frame limit applies to this rank's frames."""
        if mixed_batch is not None or use_idm:
            raise NotImplementedError("DPTrainAgent trains one policy on one batch")
        if self._lr_schedules is None:
            raise ValueError("update() needs the optimiser settings of DPTrainAgent.create (lr, end_lr, warmup_steps, decay_steps)")
        cfg, eng = self.config, self._engine
        seed = _seed_of(rng)
        nz = noise or {}
        keys = self._encoder_keys()
        mods = ["planner"] + [f"encoder{i}" for i in range(len(keys))]
        states = [self.planner_state] + [self.encoder_state_dict[k] for k in keys]
        shapes = [self._planner_shapes()] + [self._encoder_shapes()] * len(keys)
        decays = [self.planner_ema_decay] + [self.encoder_ema_decay] * len(keys)
        for m, st, sh, d in zip(mods, states, shapes, decays):      # (a (re)load synchronises the device: before anything is in flight)
            self._train_sync(m, st, sh, decay=d)
        nb = self._postprocess(batch)
        if "actions" not in nb:
            raise KeyError("update needs batch['actions'] (utils/data_utils.py:73)")
        action = nb["actions"].contiguous()
        B = action.shape[0]
        if tuple(action.shape[1:]) != (cfg["pred_horizon"], cfg["action_dim"]):
            raise ValueError(f"batch['actions'] has shape {tuple(action.shape)}: the U-Net denoises (B, pred_horizon="
                             f"{cfg['pred_horizon']}, action_dim={cfg['action_dim']}) chunks")
        oh = cfg["obs_horizon"]
        lowdim = torch.cat([self._t(nb["obs"][k])[:, :oh] for k in cfg["lowdim_obs"]], dim=-1)
        frames = self._encoder_frames(nb["obs"])
        for x in frames:
            if x.shape[0] > RESNET_TRAIN_MAX_FRAMES:
                raise ValueError(f"{x.shape[0]} frames through one encoder: a training step takes at most {RESNET_TRAIN_MAX_FRAMES}")
        feats = [eng.train_encoder_forward(i, x) for i, x in enumerate(frames)]
        cond = dp_image_cond(feats, lowdim)
        stats = eng.reduce_stats(cond)
        hg = np.random.Generator(np.random.PCG64(seed & (2**63 - 1)))
        t = nz.get("t")
        lo, n = (0, B) if shard is None else shard["rows"]
        t = np.asarray(hg.integers(0, int(cfg["n_diffusion_steps"]), size=n) if t is None else t).reshape(-1)
        if len(t) == n and n != B:
            t = t[lo:lo + B]
        eps = nz.get("noise")
        if eps is not None:
            eps = self._t(eps[lo:lo + B] if len(eps) == n and n != B else eps)
        else:
            eps = _philox_normal(seed, lo * (action.numel() // B), 0, 7, action.numel(), self._device).reshape(action.shape)
        if shard is None:
            loss, dcond = eng.train_planner_grad_cond(action, eps, t, cond)
        else:
            loss, dcond = eng.train_planner_grad_cond(action, eps, t, cond, float(np.float32(B) / np.float32(n)))
        for i, d in enumerate(dp_image_cond_inverse(dcond, [x.shape[0] // B for x in frames])):
            eng.train_encoder_backward(i, d)
        if shard is not None:                                       # data parallel: the B / n weighted shard gradients sum to the global batch's
            import torch.distributed as tdist
            for mod in mods:
                tdist.all_reduce(eng.train_arena(mod, eng.TRAIN_GRADS), group=shard.get("group"))
            loss = loss.reshape(1).clone()
            tdist.all_reduce(loss, group=shard.get("group"))
            loss = loss.reshape(())
        m, new, scheds = {}, [], self._lr_schedules
        for mod, st, sh, name in zip(mods, states, shapes, ["planner"] + [f"enc_{k}" for k in keys]):
            lr = np.float32(scheds["planner" if mod == "planner" else keys[int(mod[-1])]](st.step))
            eng.train_apply(mod, float(lr))                         # Adam at optax defaults + the EMA, one launch
            new.append(self._trained_state(mod, st, sh))
            m[f"{name}_lr"], m[f"{name}_step"] = lr, st.step        # the OLD state's step
        arrs = [DeviceArray(loss), DeviceArray(stats)]
        m["loss"] = _HostScalar(lambda: arrs[0].numpy())
        m.update({f"obs_{s}": _Elem(arrs[1], i) for i, s in enumerate(("min", "max", "mean", "std"))})
        return self.replace(planner_state=new[0], encoder_state_dict=dict(zip(keys, new[1:]))), m

    def update_mixed(self, *a, **k):
        raise NotImplementedError("DPTrainAgent has no update_mixed")
