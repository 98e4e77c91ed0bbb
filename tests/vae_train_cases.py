"""Fixtures of the whole-leaf StableVAE gradient tests (tests/test_hip_vae_train_full.py on the GPU, the conditions they rest on in
tests/test_vae_train_cpu.py): the cases, their inputs, the float64 / float32 oracle runs and the project's per-entry gradient rule.
Test infrastructure, NOT a product path."""
from collections import OrderedDict

import numpy as np
import torch

from latent_diffusion_planning_amd import weights as W
from tests import vae_model_oracle as VO
from tests import vae_train_oracle as VT
from tests.golden.make_golden_vae_update import eps_of, normalised, raw_frames

CLAMP_SHIFT = 45.0            # case d: quant_conv/bias[LC] += 45 and [LC + 1] -= 45 put log-variance channels 0 / 1 beyond the clamp (-30, 20)

#            params seed, B, use_kl, beta, clamp fixture
CASES = OrderedDict(a=(5, 1, True, 1e-5, False),       # 31 of 32 rows are padding; 4 attention rows; K = 32 wgrad with one live row
                    b=(5, 3, True, 1.0, False),        # the KL backward dominates the encoder's gradients
                    c=(7, 2, False, 1.0, False),       # use_kl = 0 ignores beta
                    d=(5, 3, True, 1.0, True))         # log-variance channel 0 above the clamp, channel 1 below it, 2 and 3 inside


def clamp_params(params):
    """`params` with the log-variance bias of channels 0 and 1 moved far outside the clamp."""
    lc = VO.latent_channels(params)
    p = OrderedDict(params)
    b = np.array(params["quant_conv/bias"], np.float32)
    b[lc] += np.float32(CLAMP_SHIFT)
    b[lc + 1] -= np.float32(CLAMP_SHIFT)
    p["quant_conv/bias"] = b
    return p


def frames_and_eps(B):
    """The seeding of tests/golden/make_golden_vae_update.case for a batch of B."""
    return normalised(raw_frames(5100 + 7 * B, B)), eps_of(5200 + 7 * B, B)


def case_inputs(name):
    """-> (params, frames (B, 64, 64, 3) float64 normalised, eps (B, 2, 2, LC) float32, use_kl, beta)."""
    pseed, B, use_kl, beta, clamp = CASES[name]
    p = W.init_vae_params(seed=pseed)
    frames, eps = frames_and_eps(B)
    return (clamp_params(p) if clamp else p), frames, eps, use_kl, beta


def oracle_run(params, frames, eps, use_kl, beta, with32=True):
    """The float64 chain and (with32) the same chain in float32 -> dict(metrics, grads, moments, err32 {path: max |g32 - g64|})."""
    torch.set_num_threads(16)
    m, g, mom, _ = VT.loss_and_grads(params, frames, eps, use_kl, beta, torch.float64)
    out = dict(metrics=m, grads=g, moments=mom)
    if with32:
        _, g32, _, _ = VT.loss_and_grads(params, frames, eps, use_kl, beta, torch.float32)
        out["err32"] = OrderedDict((k, float(np.abs(g32[k] - g[k]).max())) for k in g)
    return out


def leaf_bound(ref64, err32):
    """The project's gradient rule for one leaf (tests/test_hip_stress.py; the 1e-12 floor of tests/test_hip_dp_vae.py)."""
    return max(1e-4 * float(np.abs(ref64).max()), 3.0 * err32) + 1e-12


def combine(chunks):
    """sum_c (|c| / B) G_c in float64 of [(frames in the chunk, gradient tree)]: the gradient of the mean loss over all the frames."""
    total = float(sum(n for n, _ in chunks))
    out = OrderedDict((k, np.zeros(np.shape(v), np.float64)) for k, v in chunks[0][1].items())
    for n, g in chunks:
        for k, v in g.items():
            out[k] += (n / total) * np.asarray(v, np.float64)
    return out
