"""Algorithmic work of the hot path: 2*MACs of *non-padding* taps only, so a
kernel that multiplies zero padding is not credited.  Used by bench.py for `roofline.achieved`.
Reference shapes: networks/diffusion_nets_v2.py:113-169, networks/mlp_diffusion_nets.py:32-68,
model/stable_vae_model.yaml:4-16."""
from __future__ import annotations

from .weights import IDMSpec, PlannerSpec, VAESpec

FP32_MFMA_PEAK_TFLOPS = 157.3     # MI355X, v_mfma_f32_16x16x4_f32 / 32x32x2 (MI355X_MICROARCH.md)
HBM_PEAK_GBS = 8000.0


def _valid_taps_same(t: int, k: int) -> int:
    """sum over output positions of the taps of a k-wide, stride-1, pad k//2 conv that hit data."""
    p = k // 2
    return sum(1 for to in range(t) for j in range(k) if 0 <= to + j - p < t)


def _valid_taps_down(t_in: int) -> int:
    """k=3 stride-2 conv with XLA SAME pads (0,1) for even t_in."""
    return sum(1 for q in range(t_in // 2) for j in range(3) if 2 * q + j < t_in)


def _valid_taps_up(t_in: int) -> int:
    """transposed k=4 stride-2: out[2q]=x[q-1]K0+x[q]K2, out[2q+1]=x[q]K1+x[q+1]K3."""
    n = 0
    for q in range(t_in):
        n += (q - 1 >= 0) + 1 + 1 + (q + 1 < t_in)
    return n


def planner_forward_flops(spec: PlannerSpec, T: int, hoisted: bool = False) -> float:
    """FLOPs of one ConditionalUnet1D evaluation for one sample.  hoisted=True leaves out the
    k-only / plan-only work this build moves out of the loop (time MLP + FiLM Dense)."""
    k = spec.kernel_size
    macs = 0.0
    film = 0.0
    t = T
    blocks = spec.blocks()
    L = len(spec.down_dims)
    bi = 0

    def block(cin, cout, proj, t):
        m = _valid_taps_same(t, k) * (cin * cout + cout * cout)
        if proj:
            m += t * cin * cout
        return m

    for lvl in range(L):
        for _ in range(2):
            cin, cout, proj = blocks[bi]
            macs += block(cin, cout, proj, t)
            film += spec.cond_dim * 2 * cout
            bi += 1
        if lvl < L - 1:
            c = spec.down_dims[lvl]
            macs += _valid_taps_down(t) * c * c
            t //= 2
    for _ in range(2):
        cin, cout, proj = blocks[bi]
        macs += block(cin, cout, proj, t)
        film += spec.cond_dim * 2 * cout
        bi += 1
    for lvl in range(L - 1):
        for _ in range(2):
            cin, cout, proj = blocks[bi]
            macs += block(cin, cout, proj, t)
            film += spec.cond_dim * 2 * cout
            bi += 1
        c = list(reversed(spec.down_dims[:-1]))[lvl]
        macs += _valid_taps_up(t) * c * c
        t *= 2
    c0 = spec.down_dims[0]
    macs += _valid_taps_same(t, k) * c0 * c0 + t * c0 * spec.input_dim
    e = spec.diffusion_step_embed_dim
    time_mlp = 2 * e * 4 * e
    total = macs if hoisted else macs + film + time_mlp
    return 2.0 * total


def idm_forward_flops(spec: IDMSpec) -> float:
    """FLOPs of one MLPDiffusion evaluation for one row."""
    h = spec.hidden_dim
    macs = spec.time_dim * spec.cond_hidden[0] + spec.cond_hidden[0] * spec.cond_hidden[1]
    macs += spec.in_dim * h + spec.n_blocks * (h * 4 * h * 2) + h * spec.action_dim
    return 2.0 * macs


def plan_flops(pspec: PlannerSpec, T: int, n_steps: int, ispec: IDMSpec = None, idm_rows: int = 0,
               idm_steps: int = 0) -> float:
    f = n_steps * planner_forward_flops(pspec, T)
    if ispec is not None:
        f += idm_steps * idm_rows * idm_forward_flops(ispec)
    return f


def _taps_same_2d(s: int) -> int:
    """live taps of a 3x3, stride-1, pad-1 conv summed over the output pixels of an s x s image."""
    return _valid_taps_same(s, 3) ** 2


def _taps_down_2d(s_in: int) -> int:
    """3x3 stride 2 with XLA SAME pads (0, 1) on an even side: live taps over the output pixels."""
    return _valid_taps_down(s_in) ** 2


def vae_forward_flops(spec: VAESpec, image_size: int) -> dict:
    """FLOPs of one StableVAE forward pass for one frame, non-padding taps only (like planner_forward_flops) ->
    {"encoder": .., "decoder": .., "total": ..}.  The nearest x2 upsample is folded into its 3x3 (the taps of the upsampled image that
    hit data); the attention counts its four Dense layers and the two (tokens x tokens x C) products; GroupNorm / SiLU are not counted."""
    ch, lc, layers = spec.block_out_channels, spec.latent_channels, spec.layers_per_block

    def res(s, ci, co):
        m = _taps_same_2d(s) * (ci * co + co * co)
        return m + (s * s * ci * co if ci != co else 0)

    def mid(s, c):
        t = s * s
        return 2 * res(s, c, c) + 4 * t * c * c + 2 * t * t * c

    s, c = image_size, ch[0]
    enc = _taps_same_2d(s) * spec.in_channels * c
    for i, co in enumerate(ch):
        for _ in range(layers):
            enc += res(s, c, co)
            c = co
        if i != len(ch) - 1:
            enc += _taps_down_2d(s) * c * c
            s //= 2
    enc += mid(s, c) + _taps_same_2d(s) * c * 2 * lc + s * s * (2 * lc) ** 2
    dec = s * s * lc * lc + _taps_same_2d(s) * lc * ch[-1]
    c = ch[-1]
    dec += mid(s, c)
    for i, co in enumerate(reversed(ch)):
        for _ in range(layers + 1):
            dec += res(s, c, co)
            c = co
        if i != len(ch) - 1:
            s *= 2
            dec += _taps_same_2d(s) * c * c
    dec += _taps_same_2d(s) * c * spec.out_channels
    return {"encoder": 2.0 * enc, "decoder": 2.0 * dec, "total": 2.0 * (enc + dec)}
