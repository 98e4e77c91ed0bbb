"""ORACLE (test infrastructure, NOT a product path) -- independent float32 torch-CPU
restatement of the same hot path as oracle/np64.py, written against torch.nn.functional
primitives with the Flax->torch layout / padding / flip mappings derived in SURVEY.md
Appendix A.  It exists (i) to catch transcription errors in np64.py (the two must agree to
float32 round-off) and (ii) as the timed "CPU port" baseline in bench.py (`cpu_baseline`,
kind "port": proxy for the unavailable JAX-CPU reference path).

PARITY UNPINNED (see oracle/np64.py header): no executable reference, no golden vectors.

Mappings used (each has a KAT in tests/test_oracle_kats.py):
  * flax Conv kernel (k, Cin, Cout)           -> F.conv1d weight (Cout, Cin, k) = permute(2,1,0)
  * flax Conv stride-2 'SAME' (k=3, even T)   -> F.pad(x, (0, 1)) + conv1d(stride=2)
  * flax ConvTranspose(k=4, s=2, SAME, transpose_kernel=False)
        -> F.conv_transpose1d(x, weight[ci, co, j] = kernel[3-j, ci, co], stride=2, padding=1)
  * flax GroupNorm / LayerNorm eps = 1e-6
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F


class TorchParams:
    """Flat flax-path dict -> torch tensors, with the layout conversions cached."""

    def __init__(self, params, dtype=torch.float32, device="cpu"):
        self.raw = params
        self.dtype, self.device = dtype, device
        self._cache = {}

    def t(self, key):
        v = self._cache.get(key)
        if v is None:
            v = torch.as_tensor(np.asarray(self.raw[key]), dtype=self.dtype, device=self.device)
            self._cache[key] = v
        return v

    def conv1d_w(self, key):            # (k, Cin, Cout) -> (Cout, Cin, k)
        ck = ("c1", key)
        if ck not in self._cache:
            self._cache[ck] = self.t(key).permute(2, 1, 0).contiguous()
        return self._cache[ck]

    def convT_w(self, key):             # (k, Cin, Cout) -> (Cin, Cout, k) flipped along k
        ck = ("ct", key)
        if ck not in self._cache:
            self._cache[ck] = self.t(key).flip(0).permute(1, 2, 0).contiguous()
        return self._cache[ck]

    def conv2d_w(self, key):            # (kh, kw, Cin, Cout) -> (Cout, Cin, kh, kw)
        ck = ("c2", key)
        if ck not in self._cache:
            self._cache[ck] = self.t(key).permute(3, 2, 0, 1).contiguous()
        return self._cache[ck]

    def has(self, key):
        return key in self.raw


def _freqs(dim, device, exact=False):
    """exact: exp itself in float64, rounded to float32 once.  A float32 exp is that value or an ulp off, by library and machine: NumPy's
    vectorised one differs from it in up to 59 of 128 entries, libm's expf -- which fills the device's table (csrc/engine.hip
    sinusoid_table) -- in none, and an ulp of f moves the argument k f by up to 7.6e-6.  The default stays the float32 exp the committed goldens
    were made with; a test that bounds the device's error by float32 round-off asks for the device's own frequencies."""
    half = dim // 2
    step = np.float32(np.log(np.float32(10000.0))) / np.float32(half - 1)
    x = np.arange(half, dtype=np.float32) * -step
    f = np.exp(x.astype(np.float64)).astype(np.float32) if exact else np.exp(x).astype(np.float32)
    return torch.as_tensor(f, device=device)


def _ksteps(k, n, device):
    if torch.is_tensor(k):
        return k.to(device=device, dtype=torch.float32).reshape(-1).expand(n) if k.numel() == 1 \
            else k.to(device=device, dtype=torch.float32).reshape(n)
    k = np.asarray(k)
    return torch.as_tensor(np.broadcast_to(k.reshape(-1) if k.ndim else k, (n,)).astype(np.float32),
                           device=device)


# ------------------------------------------------------------------------------ planner
def _conv_block(P: TorchParams, x, prefix, groups, k):
    y = F.conv1d(x, P.conv1d_w(f"{prefix}/Conv_0/kernel"), P.t(f"{prefix}/Conv_0/bias"),
                 padding=k // 2)
    y = F.group_norm(y, groups, P.t(f"{prefix}/GroupNorm_0/scale"),
                     P.t(f"{prefix}/GroupNorm_0/bias"), eps=1e-6)
    return F.mish(y)


def _res_block(P, x, cond_mish, prefix, groups, k, proj):
    out = _conv_block(P, x, f"{prefix}/Conv1dBlock_0", groups, k)
    emb = F.linear(cond_mish, P.t(f"{prefix}/Dense_0/kernel").t(), P.t(f"{prefix}/Dense_0/bias"))
    c = out.shape[1]
    out = emb[:, :c, None] * out + emb[:, c:, None]
    out = _conv_block(P, out, f"{prefix}/Conv1dBlock_1", groups, k)
    res = x
    if proj:
        res = F.conv1d(x, P.conv1d_w(f"{prefix}/Conv_0/kernel"), P.t(f"{prefix}/Conv_0/bias"))
    return out + res


def unet_forward(P: TorchParams, x_btc, k, global_cond, down_dims=(256, 512, 1024),
                 kernel_size=5, n_groups=8, embed_dim=256, downsample=True):
    """Channels-first inside; takes / returns (B, T, D) like the reference."""
    dev = x_btc.device
    b = x_btc.shape[0]
    kk = _ksteps(k, b, dev)
    arg = kk[:, None] * _freqs(embed_dim, dev)[None, :]
    e = torch.cat([torch.sin(arg), torch.cos(arg)], dim=-1).to(P.dtype)
    e = F.mish(F.linear(e, P.t("Dense_0/kernel").t(), P.t("Dense_0/bias")))
    e = F.linear(e, P.t("Dense_1/kernel").t(), P.t("Dense_1/bias"))
    g = torch.cat([e, global_cond.to(P.dtype)], dim=-1) if global_cond is not None else e
    gm = F.mish(g)
    x = x_btc.to(P.dtype).transpose(1, 2)
    h = []
    idx = 0
    nl = len(down_dims)
    for lvl in range(nl):
        for proj in (True, False):
            x = _res_block(P, x, gm, f"ConditionalResidualBlock1D_{idx}", n_groups, kernel_size, proj)
            idx += 1
        h.append(x)
        if downsample and lvl < nl - 1:
            t = x.shape[-1]
            if t % 2 == 0:
                xp = F.pad(x, (0, 1))
            else:
                xp = F.pad(x, (1, 1))
            x = F.conv1d(xp, P.conv1d_w(f"Downsample1d_{lvl}/Conv_0/kernel"),
                         P.t(f"Downsample1d_{lvl}/Conv_0/bias"), stride=2)
    for _ in range(2):
        x = _res_block(P, x, gm, f"ConditionalResidualBlock1D_{idx}", n_groups, kernel_size, False)
        idx += 1
    for lvl in range(nl - 1):
        x = torch.cat([x, h.pop()], dim=1)
        for proj in (True, False):
            x = _res_block(P, x, gm, f"ConditionalResidualBlock1D_{idx}", n_groups, kernel_size, proj)
            idx += 1
        if downsample:
            x = F.conv_transpose1d(x, P.convT_w(f"Upsample1d_{lvl}/ConvTranspose_0/kernel"),
                                   P.t(f"Upsample1d_{lvl}/ConvTranspose_0/bias"),
                                   stride=2, padding=1)
    x = _conv_block(P, x, "Conv1dBlock_0", 8, kernel_size)
    x = F.conv1d(x, P.conv1d_w("Conv_0/kernel"), P.t("Conv_0/bias"))
    return x.transpose(1, 2).contiguous()


# The same computation as an ordered list of stages (tests/test_hip_planner_stages.py checks every launch of the engine on its own):
# (kind, name, inputs, fn) with `inputs` the indices of the stages whose outputs `fn(P, *inputs)` takes -- UNET_IN_X / UNET_IN_K /
# UNET_IN_COND: the call's x (channels first), timesteps and global condition -- and every activation (B, C, T) in P.dtype.  The FiLM
# vectors of all blocks are one stage, (B, F) with block i's (scale|bias) slice at column sum_{j<i} 2 Cout_j, and an input of every block's
# first half.  Built from the functions above, so chaining the stages IS unet_forward (tests/test_oracle_planner_stages.py).  Kinds: the
# engine's (include/ldp_hip.h LDP_UNET_STAGE_*), with its two FiLM parts as the one stage "film" and the residual projection a first
# half also writes as the stage "proj" of its own.
UNET_IN_X, UNET_IN_K, UNET_IN_COND = -1, -2, -3


def _time_embed(P, k, b, embed_dim, dev):
    kk = _ksteps(k, b, dev)
    arg = kk[:, None] * _freqs(embed_dim, dev)[None, :]
    e = torch.cat([torch.sin(arg), torch.cos(arg)], dim=-1).to(P.dtype)
    e = F.mish(F.linear(e, P.t("Dense_0/kernel").t(), P.t("Dense_0/bias")))
    return F.linear(e, P.t("Dense_1/kernel").t(), P.t("Dense_1/bias"))


def unet_film(P, k, global_cond, n_blocks, embed_dim=256):
    """(B, F): Dense_0(Mish([temb(k), cond])) of every residual block, side by side."""
    b = global_cond.shape[0] if global_cond is not None else int(torch.as_tensor(k).numel())
    e = _time_embed(P, k, b, embed_dim, global_cond.device if global_cond is not None else "cpu")
    g = torch.cat([e, global_cond.to(P.dtype)], dim=-1) if global_cond is not None else e
    gm = F.mish(g)
    return torch.cat([F.linear(gm, P.t(f"ConditionalResidualBlock1D_{i}/Dense_0/kernel").t(), P.t(f"ConditionalResidualBlock1D_{i}/Dense_0/bias"))
                      for i in range(n_blocks)], dim=-1)


def unet_film_parts(P, k, global_cond, n_blocks, embed_dim=256):
    """The two addends the engine keeps apart: (Mish(temb(k)) @ W[:E] + b, Mish(cond) @ W[E:]), each (B, F)."""
    b = global_cond.shape[0]
    em = F.mish(_time_embed(P, k, b, embed_dim, global_cond.device))
    cm = F.mish(global_cond.to(P.dtype))
    ws = [P.t(f"ConditionalResidualBlock1D_{i}/Dense_0/kernel") for i in range(n_blocks)]
    bs = [P.t(f"ConditionalResidualBlock1D_{i}/Dense_0/bias") for i in range(n_blocks)]
    E = em.shape[1]
    return (torch.cat([em @ w[:E] + c for w, c in zip(ws, bs)], dim=-1), torch.cat([cm @ w[E:] for w in ws], dim=-1))


def _unet_res_first(P, x, film, prefix, off, groups, k):
    """FiLM(Conv1dBlock_0(x)) with the block's slice of the FiLM stage"""
    out = _conv_block(P, x, f"{prefix}/Conv1dBlock_0", groups, k)
    c = out.shape[1]
    emb = film[:, off:off + 2 * c]
    return emb[:, :c, None] * out + emb[:, c:, None]


def _unet_res_proj(P, x, prefix):
    return F.conv1d(x, P.conv1d_w(f"{prefix}/Conv_0/kernel"), P.t(f"{prefix}/Conv_0/bias"))


def _unet_res_second(P, h, res, prefix, groups, k):
    return _conv_block(P, h, f"{prefix}/Conv1dBlock_1", groups, k) + res


def _unet_down(P, x, lvl):
    xp = F.pad(x, (0, 1)) if x.shape[-1] % 2 == 0 else F.pad(x, (1, 1))
    return F.conv1d(xp, P.conv1d_w(f"Downsample1d_{lvl}/Conv_0/kernel"), P.t(f"Downsample1d_{lvl}/Conv_0/bias"), stride=2)


def _unet_up(P, x, lvl):
    return F.conv_transpose1d(x, P.convT_w(f"Upsample1d_{lvl}/ConvTranspose_0/kernel"), P.t(f"Upsample1d_{lvl}/ConvTranspose_0/bias"),
                              stride=2, padding=1)


def unet_stages(P, down_dims=(256, 512, 1024), kernel_size=5, n_groups=8, embed_dim=256):
    nl = len(down_dims)
    n_blocks = 2 * nl + 2 + 2 * (nl - 1)
    st = [("input", "x", (UNET_IN_X,), lambda P, x: x),
          ("film", "film", (UNET_IN_K, UNET_IN_COND), lambda P, k, c: unet_film(P, k, c, n_blocks, embed_dim))]
    FILM = 1
    off = [0]

    def block(idx, xs, cout, proj):
        """xs: the stage(s) whose outputs, concatenated over channels, the block reads -> the stage of its output"""
        p = f"ConditionalResidualBlock1D_{idx}"
        cat = (lambda *t: t[0]) if len(xs) == 1 else (lambda *t: torch.cat(t, dim=1))
        st.append(("res1", f"{p}/Conv1dBlock_0", tuple(xs) + (FILM,),
                   lambda P, *t, p=p, o=off[0]: _unet_res_first(P, cat(*t[:-1]), t[-1], p, o, n_groups, kernel_size)))
        h = len(st) - 1
        off[0] += 2 * cout
        if proj:
            st.append(("proj", f"{p}/Conv_0", tuple(xs), lambda P, *t, p=p: _unet_res_proj(P, cat(*t), p)))
        res = len(st) - 1 if proj else xs[0]
        st.append(("res2", f"{p}/Conv1dBlock_1", (h, res), lambda P, h, r, p=p: _unet_res_second(P, h, r, p, n_groups, kernel_size)))
        return len(st) - 1

    cur, idx, skips = 0, 0, []
    for lvl in range(nl):
        for proj in (True, False):
            cur = block(idx, [cur], down_dims[lvl], proj)
            idx += 1
        skips.append(cur)
        if lvl < nl - 1:
            st.append(("down", f"Downsample1d_{lvl}", (cur,), lambda P, x, l=lvl: _unet_down(P, x, l)))
            cur = len(st) - 1
    for _ in range(2):
        cur = block(idx, [cur], down_dims[-1], False)
        idx += 1
    for lvl in range(nl - 1):
        cur = block(idx, [cur, skips.pop()], down_dims[nl - 2 - lvl], True)
        idx += 1
        cur = block(idx, [cur], down_dims[nl - 2 - lvl], False)
        idx += 1
        st.append(("up", f"Upsample1d_{lvl}", (cur,), lambda P, x, l=lvl: _unet_up(P, x, l)))
        cur = len(st) - 1
    st.append(("fin_block", "Conv1dBlock_0", (cur,), lambda P, x: _conv_block(P, x, "Conv1dBlock_0", 8, kernel_size)))
    st.append(("head", "Conv_0", (len(st) - 1,), lambda P, x: F.conv1d(x, P.conv1d_w("Conv_0/kernel"), P.t("Conv_0/bias"))))
    return st


@torch.no_grad()
def run_unet_stages(P, stages, x_btc, k, global_cond):
    """Every stage's output, chained from the call's inputs; the last one transposed back is unet_forward's result."""
    ext = {UNET_IN_X: x_btc.to(P.dtype).transpose(1, 2), UNET_IN_K: k, UNET_IN_COND: global_cond}
    outs = []
    for kind, name, inputs, fn in stages:
        outs.append(fn(P, *[ext[i] if i < 0 else outs[i] for i in inputs]))
    return outs


# ------------------------------------------------------------------------------ IDM
def idm_forward(P: TorchParams, s, a, k, time_dim=256, n_blocks=3, exact_freqs=False):
    dev = s.device
    r = s.shape[0]
    kk = _ksteps(k, r, dev)
    arg = kk[:, None] * _freqs(time_dim, dev, exact_freqs)[None, :]
    tff = torch.cat([torch.cos(arg), torch.sin(arg)], dim=-1).to(P.dtype)
    c = F.mish(F.linear(tff, P.t("MLP_0/Dense_0/kernel").t(), P.t("MLP_0/Dense_0/bias")))
    c = F.linear(c, P.t("MLP_0/Dense_1/kernel").t(), P.t("MLP_0/Dense_1/bias"))
    h = F.linear(torch.cat([a.to(P.dtype), s.to(P.dtype), c], dim=-1),
                 P.t("MLPResNet_0/Dense_0/kernel").t(), P.t("MLPResNet_0/Dense_0/bias"))
    for i in range(n_blocks):
        p = f"MLPResNet_0/MLPResNetBlock_{i}"
        y = F.layer_norm(h, (h.shape[-1],), P.t(f"{p}/LayerNorm_0/scale"),
                         P.t(f"{p}/LayerNorm_0/bias"), eps=1e-6)
        y = F.relu(F.linear(y, P.t(f"{p}/Dense_0/kernel").t(), P.t(f"{p}/Dense_0/bias")))
        h = h + F.linear(y, P.t(f"{p}/Dense_1/kernel").t(), P.t(f"{p}/Dense_1/bias"))
    return F.linear(F.relu(h), P.t("MLPResNet_0/Dense_1/kernel").t(), P.t("MLPResNet_0/Dense_1/bias"))


# ------------------------------------------------------------------------------ schedulers
def _tables(n):
    def abar(t):
        return math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2
    betas = torch.tensor([min(1 - abar((i + 1) / n) / abar(i / n), 0.999) for i in range(n)],
                         dtype=torch.float32)
    alphas = 1.0 - betas
    return betas, alphas, torch.cumprod(alphas, 0)


def ddpm_step(eps, t, x, noise, tables):
    """float32 arithmetic throughout, like the reference's traced step."""
    betas, alphas, acp = tables
    a_t = acp[t]
    a_prev = acp[t - 1] if t > 0 else torch.tensor(1.0)
    x0 = ((x - (1 - a_t).sqrt() * eps) / a_t.sqrt()).clamp(-1.0, 1.0)
    c0 = a_prev.sqrt() * betas[t] / (1 - a_t)
    cx = alphas[t].sqrt() * (1 - a_prev) / (1 - a_t)
    out = c0 * x0 + cx * x
    if t > 0:
        var = ((1 - a_prev) / (1 - a_t) * betas[t]).clamp(min=1e-20)
        out = out + var.sqrt() * noise
    return out


def ddim_step(eps, t, t_prev, x, tables):
    _, _, acp = tables
    a_t = acp[t]
    a_prev = acp[t_prev] if t_prev >= 0 else torch.tensor(1.0)
    x0 = ((x - (1 - a_t).sqrt() * eps) / a_t.sqrt()).clamp(-1.0, 1.0)
    return a_prev.sqrt() * x0 + (1 - a_prev).sqrt() * eps


@torch.no_grad()
def planner_sample(P, obs_cond, x_init, step_noise=None, n_train=100, n_steps=100,
                   sampler="ddpm", stop_after=None, **kw):
    """stop_after: run only the first `stop_after` of the n_steps steps (bench.py's bounded CPU
    timing; every step costs the same).  None = the whole loop."""
    tables = _tables(n_train)
    x = x_init.to(P.dtype)
    stride = n_train // n_steps
    for i in range(n_steps if stop_after is None else min(stop_after, n_steps)):
        k = (n_steps - 1 - i) * stride
        eps = unet_forward(P, x, k, obs_cond, **kw)
        if sampler == "ddpm":
            x = ddpm_step(eps, k, x, step_noise[i] if k > 0 else None, tables)
        else:
            x = ddim_step(eps, k, k - stride, x, tables)
    return x


@torch.no_grad()
def idm_sample(P, transition, a_init, step_noise=None, n_train=100, n_steps=100, sampler="ddpm",
               stop_after=None, exact_freqs=False):
    tables = _tables(n_train)
    a = a_init.to(P.dtype)
    stride = n_train // n_steps
    for i in range(n_steps if stop_after is None else min(stop_after, n_steps)):
        k = (n_steps - 1 - i) * stride
        eps = idm_forward(P, transition, a, k, exact_freqs=exact_freqs)
        if sampler == "ddpm":
            a = ddpm_step(eps, k, a, step_noise[i] if k > 0 else None, tables)
        else:
            a = ddim_step(eps, k, k - stride, a, tables)
    return a


# ------------------------------------------------------------------------------ StableVAE
def _gn2(P, x, prefix, groups=32):
    return F.group_norm(x, groups, P.t(f"{prefix}/scale"), P.t(f"{prefix}/bias"), eps=1e-6)


def _conv3(P, x, prefix):
    return F.conv2d(x, P.conv2d_w(f"{prefix}/kernel"), P.t(f"{prefix}/bias"), padding=1)


def _conv1(P, x, prefix):
    return F.conv2d(x, P.conv2d_w(f"{prefix}/kernel"), P.t(f"{prefix}/bias"))


def _res_first(P, x, prefix):
    """conv1(swish(norm1 x))"""
    return _conv3(P, F.silu(_gn2(P, x, f"{prefix}/norm1")), f"{prefix}/conv1")


def _res_shortcut(P, x, prefix):
    return _conv1(P, x, f"{prefix}/conv_shortcut")


def _res_second(P, h, skip, prefix):
    """conv2(swish(norm2 h)) + skip"""
    return _conv3(P, F.silu(_gn2(P, h, f"{prefix}/norm2")), f"{prefix}/conv2") + skip


def _resnet2d(P, x, prefix):
    h = _res_first(P, x, prefix)
    if P.has(f"{prefix}/conv_shortcut/kernel"):
        x = _res_shortcut(P, x, prefix)
    return _res_second(P, h, x, prefix)


def _attn(P, x, prefix):
    n, c, hh, ww = x.shape
    r = _gn2(P, x, f"{prefix}/group_norm").reshape(n, c, hh * ww).transpose(1, 2)
    lin = lambda t, nm: F.linear(t, P.t(f"{prefix}/{nm}/kernel").t(), P.t(f"{prefix}/{nm}/bias"))
    q, k, v = lin(r, "query"), lin(r, "key"), lin(r, "value")
    sc = c ** -0.25
    w = torch.softmax((q * sc) @ (k * sc).transpose(1, 2), dim=-1)
    o = lin(w @ v, "proj_attn")
    return o.transpose(1, 2).reshape(n, c, hh, ww) + x


def _mid(P, x, prefix):
    x = _resnet2d(P, x, f"{prefix}/resnets_0")
    x = _attn(P, x, f"{prefix}/attentions_0")
    return _resnet2d(P, x, f"{prefix}/resnets_1")


def _downsample(P, x, prefix):
    return F.conv2d(F.pad(x, (0, 1, 0, 1)), P.conv2d_w(f"{prefix}/kernel"), P.t(f"{prefix}/bias"), stride=2)


def _upsample(x):
    return F.interpolate(x, scale_factor=2.0, mode="nearest")


def _up_conv(P, x, prefix):
    return _conv3(P, _upsample(x), prefix)


def _norm_out_conv(P, x, side):
    return _conv3(P, F.silu(_gn2(P, x, f"{side}/conv_norm_out")), f"{side}/conv_out")


@torch.no_grad()
def vae_encode_mean(P, img_nhwc, n_blocks=6, layers=2, latent_channels=4):
    x = img_nhwc.to(P.dtype).permute(0, 3, 1, 2)
    x = _conv3(P, x, "encoder/conv_in")
    for i in range(n_blocks):
        for j in range(layers):
            x = _resnet2d(P, x, f"encoder/down_blocks_{i}/resnets_{j}")
        if i != n_blocks - 1:
            x = _downsample(P, x, f"encoder/down_blocks_{i}/downsamplers_0/conv")
    x = _mid(P, x, "encoder/mid_block")
    x = _norm_out_conv(P, x, "encoder")
    x = _conv1(P, x, "quant_conv")
    return x[:, :latent_channels].permute(0, 2, 3, 1).contiguous()


@torch.no_grad()
def vae_decode(P, z_nhwc, n_blocks=6, layers=2):
    x = z_nhwc.to(P.dtype).permute(0, 3, 1, 2)
    x = _conv1(P, x, "post_quant_conv")
    x = _conv3(P, x, "decoder/conv_in")
    x = _mid(P, x, "decoder/mid_block")
    for i in range(n_blocks):
        for j in range(layers + 1):
            x = _resnet2d(P, x, f"decoder/up_blocks_{i}/resnets_{j}")
        if i != n_blocks - 1:
            x = _up_conv(P, x, f"decoder/up_blocks_{i}/upsamplers_0/conv")
    return _norm_out_conv(P, x, "decoder")


# The same two computations as ordered lists of stages (tests/test_hip_vae_stages.py checks every stage of the engine on its own):
# (kind, name, inputs, fn) with `inputs` the indices of the stages whose outputs `fn(P, *inputs)` takes (-1: the call's input, NCHW)
# and every tensor NCHW in P.dtype.  Built from the functions above, so chaining them IS vae_encode_mean / vae_decode
# (tests/test_oracle_vae_stages.py).  The kinds are the engine's (include/ldp_hip.h LDP_VAE_STAGE_*).
def _resnet_stages(P, st, prefix, x_idx):
    st.append(("res1", f"{prefix}/conv1", (x_idx,), lambda P, x, p=prefix: _res_first(P, x, p)))
    h_idx, skip = len(st) - 1, x_idx
    if P.has(f"{prefix}/conv_shortcut/kernel"):
        st.append(("shortcut", f"{prefix}/conv_shortcut", (x_idx,), lambda P, x, p=prefix: _res_shortcut(P, x, p)))
        skip = len(st) - 1
    st.append(("res2", f"{prefix}/conv2", (h_idx, skip), lambda P, h, s, p=prefix: _res_second(P, h, s, p)))
    return len(st) - 1


def _mid_stages(P, st, prefix, x_idx):
    x_idx = _resnet_stages(P, st, f"{prefix}/resnets_0", x_idx)
    st.append(("attn", f"{prefix}/attentions_0", (x_idx,), lambda P, x, p=prefix: _attn(P, x, f"{p}/attentions_0")))
    return _resnet_stages(P, st, f"{prefix}/resnets_1", len(st) - 1)


def vae_encode_stages(P, n_blocks=6, layers=2):
    """Input: frames NCHW.  The last stage is quant_conv with all 2 * latent_channels moments (vae_encode_mean keeps the first half)."""
    st = [("conv_in", "encoder/conv_in", (-1,), lambda P, x: _conv3(P, x, "encoder/conv_in"))]
    cur = 0
    for i in range(n_blocks):
        for j in range(layers):
            cur = _resnet_stages(P, st, f"encoder/down_blocks_{i}/resnets_{j}", cur)
        if i != n_blocks - 1:
            p = f"encoder/down_blocks_{i}/downsamplers_0/conv"
            st.append(("down", p, (cur,), lambda P, x, p=p: _downsample(P, x, p)))
            cur = len(st) - 1
    cur = _mid_stages(P, st, "encoder/mid_block", cur)
    st.append(("conv_out", "encoder/conv_out", (cur,), lambda P, x: _norm_out_conv(P, x, "encoder")))
    st.append(("quant", "quant_conv", (len(st) - 1,), lambda P, x: _conv1(P, x, "quant_conv")))
    return st


def vae_decode_stages(P, n_blocks=6, layers=2):
    """Input: z NCHW.  The last stage is the engine's NCHW transpose: the identity here."""
    st = [("post_quant", "post_quant_conv", (-1,), lambda P, x: _conv1(P, x, "post_quant_conv")),
          ("conv_in", "decoder/conv_in", (0,), lambda P, x: _conv3(P, x, "decoder/conv_in"))]
    cur = _mid_stages(P, st, "decoder/mid_block", 1)
    for i in range(n_blocks):
        for j in range(layers + 1):
            cur = _resnet_stages(P, st, f"decoder/up_blocks_{i}/resnets_{j}", cur)
        if i != n_blocks - 1:
            p = f"decoder/up_blocks_{i}/upsamplers_0/conv"
            st.append(("up", p, (cur,), lambda P, x, p=p: _up_conv(P, x, p)))
            cur = len(st) - 1
    st.append(("conv_out", "decoder/conv_out", (cur,), lambda P, x: _norm_out_conv(P, x, "decoder")))
    st.append(("nchw", "sample", (len(st) - 1,), lambda P, x: x))
    return st


@torch.no_grad()
def run_stages(P, stages, x_nchw):
    """Every stage's output, chained from the call's input."""
    outs = []
    for kind, name, inputs, fn in stages:
        outs.append(fn(P, *[x_nchw.to(P.dtype) if i < 0 else outs[i] for i in inputs]))
    return outs
