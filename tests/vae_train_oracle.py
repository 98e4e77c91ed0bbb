"""ORACLE (test infrastructure, NOT a product path) -- StableVAEModel.update_step (model/stable_vae_model.py:57-73) in float64 torch
autograd: the networks are oracle.torch32's VAE forward (`vae_encode_mean.__wrapped__` / `vae_decode.__wrapped__`, the undecorated functions
behind @torch.no_grad) over oracle.train.GradParams leaves; the posterior, KL and loss are tests/vae_model_oracle.py's, restated in torch;
Adam and the schedule are oracle/train.py's, the EMA tests/dp_oracle.ema_update.  `dtype=torch.float32` runs the same chain in float32:
the reference's own error, which the per-leaf bounds of the GPU tests come from.
PARITY UNPINNED like the other oracles: no executable reference here.
"""
from collections import OrderedDict

import numpy as np
import torch

from oracle import torch32
from oracle import train as OT
from tests import dp_oracle
from tests import vae_model_oracle as VO

LR, END_LR, WARMUP = 1e-4, 1e-6, 1000          # train_vae.yaml
EMA_DECAY = 0.99
BETA = 1e-5                                     # model/stable_vae_model.yaml


class GradParams32(torch32.TorchParams):
    """GradParams with float32 leaves."""

    def __init__(self, params):
        super().__init__(params, dtype=torch.float32)
        self.leaves = OrderedDict((k, torch.tensor(np.asarray(v, np.float32), requires_grad=True)) for k, v in params.items())

    def t(self, key):
        return self.leaves[key]

    def grads(self):
        return OrderedDict((k, (v.grad if v.grad is not None else torch.zeros_like(v)).double().numpy().copy()) for k, v in self.leaves.items())


def loss_and_grads(params, frames_nhwc, eps, use_kl=True, beta=BETA, dtype=torch.float64):
    """`loss` (:25-55) and jax.grad of it w.r.t. every leaf -> (metrics dict, grads {path: float64 array}, moments (N, h, w, 2 LC),
    reconstruction (N, 3, S, S))."""
    P = OT.GradParams(params) if dtype == torch.float64 else GradParams32(params)
    lc = VO.latent_channels(params)
    x = torch.tensor(np.asarray(frames_nhwc, np.float64), dtype=dtype)
    mom = torch32.vae_encode_mean.__wrapped__(P, x, latent_channels=2 * lc)
    mean, lv = mom[..., :lc], torch.clamp(mom[..., lc:], -30.0, 20.0)
    z = mean + torch.exp(0.5 * lv) * torch.tensor(np.asarray(eps, np.float64), dtype=dtype)
    kl = 0.5 * torch.sum(mean ** 2 + torch.exp(lv) - 1.0 - lv, dim=(1, 2, 3))
    rec = torch32.vae_decode.__wrapped__(P, z)
    mse = torch.mean((x.permute(0, 3, 1, 2) - rec) ** 2)
    loss = mse + beta * torch.mean(kl) if use_kl else mse
    loss.backward()
    metrics = VO.metrics_from(frames_nhwc, z.detach().double().numpy(), kl.detach().double().numpy(), rec.detach().double().numpy(), use_kl, beta)
    return metrics, P.grads(), mom.detach().double().numpy(), rec.detach().double().numpy()


def schedule():
    """warmup_cosine_decay_schedule(end_lr -> lr -> end_lr) as StableVAEModel.create builds it (decay_steps = n_grad_steps)."""
    return OT.warmup_cosine_decay_schedule(END_LR, LR, WARMUP, 300000, END_LR)


def train(params, steps, use_kl=True, beta=BETA, decay=EMA_DECAY, dtype=torch.float64):
    """`steps` = [(frames, eps)]: update_step per entry -> list of dict(metrics, grads, params, ema, lr) after each step (metrics / grads of the
    pre-update parameters, lr = schedule(old count))."""
    sched = schedule()
    p = OrderedDict((k, np.asarray(v, np.float64)) for k, v in params.items())
    ema = OrderedDict(p)
    opt = OT.adam_init(p)
    out = []
    for frames, eps in steps:
        lr = sched(opt["count"])
        m, g, mom, _ = loss_and_grads(p, frames, eps, use_kl, beta, dtype)
        p, opt = OT.adam_apply(p, g, opt, sched)
        ema = dp_oracle.ema_update(ema, p, decay)
        out.append(dict(metrics=m, grads=g, params=p, ema=ema, lr=lr, moments=mom))
    return out
