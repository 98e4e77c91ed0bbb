"""ORACLE (test infrastructure, NOT a product path) -- float64 restatement of StableVAEModel's forward side
(model/stable_vae_model.py:25-55 `loss`, :94-101 `reconstruct_step`, :118-123 `sample_step`) and of diffusers'
FlaxDiagonalGaussianDistribution (models/vae_flax.py: `__init__` split / clip(-30, 20) / exp, `sample`, `kl`, `mode`).
The two networks are oracle.np64's; `vae_encode_mean(..., latent_channels=2 * LC)` returns every quant_conv channel.
PARITY UNPINNED like the other oracles: no executable reference here.
"""
import numpy as np

from oracle import np64, philox

METRIC_KEYS = ("img_min", "img_max", "img_mean", "img_std", "loss", "loss_mse", "loss_kl", "z_min", "z_max", "z_mean", "z_std")
STREAM_VAE_EPS = 9            # include/ldp_hip.h LDP_PHILOX_STREAM_VAE_EPS
STREAM_VAE_SAMPLE = 10        # LDP_PHILOX_STREAM_VAE_SAMPLE


def latent_channels(params) -> int:
    return int(np.asarray(params["post_quant_conv/bias"]).shape[0])


def moments(params, frames_nhwc):
    """encode(x).latent_dist.parameters, channels-last: (N, h, w, 2 LC)."""
    return np64.vae_encode_mean(params, frames_nhwc, latent_channels=2 * latent_channels(params))


def posterior(mom, eps):
    """FlaxDiagonalGaussianDistribution on channels-last moments -> (z, per-image kl, std)."""
    mom = np.asarray(mom, np.float64)
    lc = mom.shape[-1] // 2
    mean, logvar = mom[..., :lc], np.clip(mom[..., lc:], -30.0, 20.0)       # jnp.split(parameters, 2, axis=-1); jnp.clip
    std, var = np.exp(0.5 * logvar), np.exp(logvar)
    z = mean + std * np.asarray(eps, np.float64)                             # sample
    kl = 0.5 * np.sum(mean ** 2 + var - 1.0 - logvar, axis=(1, 2, 3))        # kl(other=None)
    return z, kl, std


def metrics_from(frames_nhwc, z, kl, rec_nchw, use_kl, beta):
    """The eleven scalars of `loss` (:34-53) from its tensors."""
    img = np.transpose(np.asarray(frames_nhwc, np.float64), (0, 3, 1, 2))
    mse = float(np.mean((img - np.asarray(rec_nchw, np.float64)) ** 2))
    klm = float(np.mean(kl)) if use_kl else 0.0
    z = np.asarray(z, np.float64)
    return dict(img_min=float(img.min()), img_max=float(img.max()), img_mean=float(img.mean()), img_std=float(img.std()),
                loss=mse + float(beta) * klm, loss_mse=mse, loss_kl=klm,
                z_min=float(z.min()), z_max=float(z.max()), z_mean=float(z.mean()), z_std=float(z.std()))


def loss(params, frames_nhwc, eps, use_kl, beta):
    """-> (metrics dict, z (N, h, w, LC), rec (N, 3, S, S), moments (N, h, w, 2 LC)).  frames: normalised NHWC, cameras already
    concatenated on the batch axis (:28)."""
    mom = moments(params, frames_nhwc)
    z, kl, _ = posterior(mom, eps)
    rec = np64.vae_decode(params, z)
    return metrics_from(frames_nhwc, z, kl, rec, use_kl, beta), z, rec, mom


def reconstruct(params, frames_nhwc):
    """decode(encode(x).latent_dist.mode()).sample (:94-101); mode() is the mean."""
    lc = latent_channels(params)
    return np64.vae_decode(params, np64.vae_encode_mean(params, frames_nhwc, latent_channels=lc))


def sample(params, latents):
    return np64.vae_decode(params, latents)


def float32_chain(params, frames_nhwc, eps, use_kl, beta):
    """The same chain in float32 through oracle.torch32 (an independent restatement of the two networks) and float32 numpy: the
    reference's own error, which the bounds of the trained-like case are derived from.  -> like `loss`."""
    import torch
    from oracle import torch32
    P = torch32.TorchParams(params, dtype=torch.float32)
    lc = latent_channels(params)
    mom = torch32.vae_encode_mean(P, torch.tensor(np.asarray(frames_nhwc), dtype=torch.float32), latent_channels=2 * lc).numpy()
    mean, lv = mom[..., :lc], np.clip(mom[..., lc:], np.float32(-30), np.float32(20))
    z = (mean + np.exp(np.float32(0.5) * lv) * np.asarray(eps, np.float32)).astype(np.float32)
    kl = np.float32(0.5) * np.sum(mean * mean + np.exp(lv) - np.float32(1) - lv, axis=(1, 2, 3), dtype=np.float32)
    rec = torch32.vae_decode(P, torch.tensor(z)).numpy()
    return metrics_from(frames_nhwc, z, kl, rec, use_kl, beta), z, rec, mom


def trained_like_params(seed=2, frames=None):
    """A heavy-tailed VAE set that meets the fixture condition: tests.util.trained_like on the seeded init (as vae_params_heavy), then
    quant_conv's log-variance columns scaled until |logvar| <= 2 on `frames` (trained_like was tuned for the mean channels only and
    leaves the log-variance head saturating both clamps)."""
    from latent_diffusion_planning_amd import weights as W
    from tests.util import VAE_STREAM, rng, trained_like
    base = trained_like(W.init_vae_params(seed=seed), 1000 + seed, heads=("quant_conv", "decoder/conv_out"), out_scale=1.0 / 100.0,
                        keep=VAE_STREAM)
    if frames is None:
        frames = rng(4244).uniform(-1, 1, (2, 64, 64, 3))
    lc = latent_channels(base)
    lv = moments(base, frames)[..., lc:]
    scale = 2.0 / float(np.abs(lv).max())
    k, b = np.array(base["quant_conv/kernel"], np.float64), np.array(base["quant_conv/bias"], np.float64)
    k[..., lc:] *= scale
    b[lc:] *= scale
    fit = dict(base)
    fit["quant_conv/kernel"], fit["quant_conv/bias"] = k.astype(np.float32), b.astype(np.float32)
    return fit, base


def philox_eps(seed, n_frames, per_frame, row_offset=0, stream=STREAM_VAE_EPS):
    """The eps libldp_hip draws for frames row_offset .. row_offset + n_frames - 1: element (row_offset + n) * per_frame + e."""
    return philox.normal(seed, row_offset * per_frame, 0, stream, n_frames * per_frame).reshape(n_frames, per_frame)
