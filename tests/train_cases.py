"""Fixtures of the training-GEMM launch-shape tests (tests/test_hip_train_shapes.py and tests/test_hip_resnet_train_shapes.py on the GPU, the
conditions they rest on in tests/test_train_cpu.py): the option sets that reach each of the 15 instantiations of csrc/train.hip's kernel
family, the `gemm_shape` and `fused_part_bytes` rules restated, the launches of the ResNet-18 encoder's tape restated from its convolution
tables, the batches, the IDM row selection and the per-entry gradient rule.  Test infrastructure, NOT a product path."""
from collections import OrderedDict

import numpy as np
import torch

from oracle import torch32
from oracle import train as OT
from tests.util import rng

D, A, T = 25, 7, 8

# name -> the options it sets (every other option of DEFAULTS keeps its default)
CONFIGS = OrderedDict(
    t32={},
    t64=dict(train_small_wg=0),
    t128=dict(train_big=1),
    t128_64=dict(train_big=1, train_small_wg=0),
    ki2_32=dict(train_intra_split=1),
    ki2_64=dict(train_intra_split=1, train_small_wg=0),
    nosplit=dict(train_split=0),
    deep=dict(train_wg_target=1536),
    shallow=dict(train_wg_target=48),
    gn_generic=dict(train_gn4=0),
    ungrouped=dict(train_group_proj=0),
    reduce=dict(train_fuse_reduce=0),          # (not a launch shape: the separate reduce launch, so that it too meets the oracle)
)
# csrc/engine.hpp Options: the defaults of every option a test of the module touches
DEFAULTS = dict(train_small_wg=1 << 20, train_big=0, train_intra_split=0, train_split=1, train_wg_target=384, train_gn4=1, train_group_proj=1,
                train_fuse_reduce=1, train_streams=1, train_sides=1)

FORMS = ("nn", "nt", "tn")
TILES = ("32", "32_ki2", "64", "64_ki2", "128")
KERNELS = tuple(f"{f}_{t}" for f in FORMS for t in TILES)                     # the 15 instantiations
COUNTERS = tuple(f"stat_train_gemm_{k}" for k in KERNELS + ("fused", "reduce"))


def options(name):
    return dict(DEFAULTS, **CONFIGS[name])


# ---- csrc/train.hip gemm_shape, restated ----------------------------------------------------------------------------------------------------
def gemm_shape(M, N, nbatch, min_steps, opt, can_split=True):
    """One launch -> (tile rows 32 / 64 / 128, K split over work-groups, 1 or 2 wave quartets per work-group).  128 x 128 tiles where train_big
    and both M and N reach 128; else 64 columns by 32 rows where the 64-row tiling has fewer than train_small_wg work-groups (and M is a
    multiple of 32), else by 64 rows.  K is split in factors of two while the launch has fewer than train_wg_target work-groups, at most 32
    ways, and every split keeps at least two K steps; train_intra_split takes the first factor of two into the work-group (never for the 128-row
    tile)."""
    cdiv = lambda a, b: -(-a // b)          # noqa: E731
    if opt["train_big"] and M >= 128 and N >= 128:
        tile, tiles = 128, cdiv(N, 128) * cdiv(M, 128) * nbatch
    else:
        small = cdiv(N, 64) * cdiv(M, 64) * nbatch < opt["train_small_wg"] and M % 32 == 0
        tile = 32 if small else 64
        tiles = cdiv(N, 64) * cdiv(M, tile) * nbatch
    ks, ki = 1, 1
    if can_split and opt["train_split"]:
        while ks < 32 and tiles * ks < opt["train_wg_target"] and min_steps // (ks * 2) >= 2:
            ks *= 2
    if opt["train_intra_split"] and tile != 128 and ks >= 2:
        ki, ks = 2, ks // 2
    return tile, ks, ki


def kernel_of(form, tile, ki):
    return f"{form}_{tile}" + ("_ki2" if ki == 2 else "")


CNT_TILES = 1 << 16                        # csrc/train.hip: tickets of one launch


def fused_part_bytes(M, N, nbatch, tile, ks):
    """csrc/train.hip fused_part_bytes, restated: the workspace of the in-launch split-K finish (ks blocks of one tile per output tile), or 0
    where the launch cannot use it (more tiles than tickets, offsets beyond 2^31) and falls back to the separate reduce launch."""
    cdiv = lambda a, b: -(-a // b)          # noqa: E731
    tiles = cdiv(N, 128) * cdiv(M, 128) * nbatch if tile == 128 else cdiv(N, 64) * cdiv(M, tile) * nbatch
    size = tiles * ks * (128 * 128 if tile == 128 else tile * 64) * 4
    return size if tiles <= CNT_TILES and size < 1 << 31 else 0


# ---- csrc/train_tables.hpp tap_1d / tap_2d / plan_taps, restated ----------------------------------------------------------------------------------
MODE_K5, MODE_DOWN, MODE_UP, MODE_P1 = 0, 1, 2, 3   # 1-D: k = 5 pad 2, k = 3 stride 2 pad (0, 1), transposed k = 4 stride 2, 1x1
VC_S1, VC_S2, VC_UP, VC_P1, VC_P2 = 0, 1, 2, 3, 4   # 2-D: 3x3 pad 1, 3x3 stride 2 pad (0, 1), nearest x2 then 3x3, 1x1, 1x1 stride 2


def tap_in_1d(mode, Tin, to, j):
    """Input position that tap j of output position `to` reads, or -1 (padding, or a tap of the transposed convolution's other phase)."""
    if mode == MODE_K5:
        ti = to + j - 2
    elif mode == MODE_DOWN:
        ti = 2 * to + j
    elif mode == MODE_UP:                  # out[2q] = x[q-1] K0 + x[q] K2; out[2q+1] = x[q] K1 + x[q+1] K3
        q = to >> 1
        ti = {0: q - 1, 2: q}.get(j, -1) if to % 2 == 0 else {1: q, 3: q + 1}.get(j, -1)
    elif mode == MODE_P1:
        ti = to
    else:
        raise ValueError(mode)
    return ti if 0 <= ti < Tin else -1


def tap_in(mode, Sin, Sout, po, j):
    """Input pixel that tap j of output pixel po reads, or -1 (padding)."""
    y, x, dy, dx = po // Sout, po % Sout, j // 3, j % 3
    if mode == VC_S1:
        iy, ix = y + dy - 1, x + dx - 1
    elif mode == VC_S2:
        iy, ix = 2 * y + dy, 2 * x + dx
    elif mode == VC_UP:                    # the 3x3 reads the upsampled image (side Sout) at (uy, ux): input pixel (uy >> 1, ux >> 1)
        uy, ux = y + dy - 1, x + dx - 1
        if uy < 0 or ux < 0 or uy >= Sout or ux >= Sout:
            return -1
        iy, ix = uy >> 1, ux >> 1
    elif mode == VC_P2:
        return 2 * y * Sin + 2 * x if j == 0 else -1
    elif mode == VC_P1:
        return po if j == 0 else -1
    else:
        raise ValueError(mode)
    return -1 if iy < 0 or ix < 0 or iy >= Sin or ix >= Sin else iy * Sin + ix


def ntaps_of(family, mode):
    return {MODE_K5: 5, MODE_DOWN: 3, MODE_UP: 4, MODE_P1: 1}[mode] if family == "1d" else (1 if mode in (VC_P1, VC_P2) else 9)


def conv_tables(family, mode, Sin, Sout, cin, cout):
    """The three launch tables of one convolution, appended to empty tables -> dict(segs=[(a_off, b_off)], batches=[(c_off, seg_begin, seg_end)],
    plan=dict(Tin, Tout, ntaps, f_b0, f_nb, f_minseg, d_b0, ...)).  family "1d": Sin / Sout positions; "2d": square images of side Sin / Sout.
    Written loop for loop as the two builders this header replaced walked them, so it states their order: forward = a batch per output with a
    segment per live tap; data gradient = a batch per input whose segments run output-major and tap-minor (the summation order of its split
    K); weight gradient = a batch per tap with a segment per output it is live at, and no batch for a tap that is live nowhere."""
    if family == "1d":
        Tin, Tout = Sin, Sout
        tap = lambda to, j: tap_in_1d(mode, Tin, to, j)                  # noqa: E731
    else:
        Tin, Tout = Sin * Sin, Sout * Sout
        tap = lambda to, j: tap_in(mode, Sin, Sout, to, j)               # noqa: E731
    ntaps, wtap = ntaps_of(family, mode), cin * cout
    segs, batches, plan = [], [], dict(Tin=Tin, Tout=Tout, ntaps=ntaps)

    def close(kind, c_off, s0, keep_empty=True):
        n = len(segs) - s0
        if n == 0 and not keep_empty:
            return
        batches.append((c_off, s0, len(segs)))
        plan[kind + "_minseg"] = n if plan[kind + "_nb"] == 0 else min(plan[kind + "_minseg"], n)
        plan[kind + "_nb"] += 1

    plan.update(f_b0=len(batches), f_nb=0, f_minseg=0)
    for to in range(Tout):
        s0 = len(segs)
        for j in range(ntaps):
            ti = tap(to, j)
            if ti >= 0:
                segs.append((ti * cin, j * wtap))
        close("f", to * cout, s0)
    plan.update(d_b0=len(batches), d_nb=0, d_minseg=0)
    for ti in range(Tin):
        s0 = len(segs)
        for to in range(Tout):
            for j in range(ntaps):
                if tap(to, j) == ti:
                    segs.append((to * cout, j * wtap))
        close("d", ti * cin, s0)
    plan.update(w_b0=len(batches), w_nb=0, w_minseg=0)
    for j in range(ntaps):
        s0 = len(segs)
        for to in range(Tout):
            ti = tap(to, j)
            if ti >= 0:
                segs.append((ti * cin, to * cout))
        close("w", j * wtap, s0, keep_empty=False)
    return dict(segs=segs, batches=batches, plan=plan)


def conv_plan(mode, Sin, Sout):
    """-> dict(f_nb, f_minseg, d_nb, d_minseg, w_nb, w_minseg): batches of the forward / data-gradient / weight-gradient launch of one 2-D
    convolution and the fewest segments any of them has.  Forward: one batch per output pixel, a segment per live tap; data gradient: one
    batch per input pixel, a segment per (output pixel, tap) that reads it -- none at the pixels a stride-2 1x1 skips; weight gradient: one
    batch per tap that is live somewhere, a segment per output pixel it is live at."""
    ntaps = 1 if mode in (VC_P1, VC_P2) else 9
    Tin, Tout = Sin * Sin, Sout * Sout
    live = [[tap_in(mode, Sin, Sout, to, j) for j in range(ntaps)] for to in range(Tout)]
    hits = [0] * Tin
    for row in live:
        for ti in row:
            if ti >= 0:
                hits[ti] += 1
    per_tap = [sum(1 for to in range(Tout) if live[to][j] >= 0) for j in range(ntaps)]
    per_tap = [n for n in per_tap if n > 0]
    return dict(f_nb=Tout, f_minseg=min(sum(1 for ti in row if ti >= 0) for row in live), d_nb=Tin, d_minseg=min(hits),
                w_nb=len(per_tap), w_minseg=min(per_tap))


def encoder_convs():
    """The 20 convolutions of csrc/resnet_train.hpp's tape as (mode, Sin, Sout, cin, cout, has a data gradient): the stem as a 1x1 over gathered
    patches (K = 147 padded to 160; the image is no parameter) and, per ResNetBlock (rnt_block), Conv_0, Conv_1 and the projection."""
    out = [(VC_P1, 32, 32, 160, 64, False)]
    S = 16
    for b in range(8):
        stage = b // 2
        cout, cin = 64 << stage, 64 if b == 0 else 64 << ((b - 1) // 2)
        stride = 2 if stage > 0 and b % 2 == 0 else 1
        So = S // stride
        out.append((VC_S1 if stride == 1 else VC_S2, S, So, cin, cout, True))
        out.append((VC_S1, So, So, cout, cout, True))
        if stride != 1 or cin != cout:
            out.append((VC_P2, S, So, cin, cout, True))
        S = So
    return out


def encoder_launches(rows):
    """The 59 GEMM launches of one encoder forward + backward over `rows` padded frames (conv_fwd / conv_dgrad / conv_wgrad): 20 forward,
    19 data-gradient, 20 weight-gradient, as (form, M, N, batches, fewest K steps of a batch)."""
    fwd, dgrad, wgrad = [], [], []
    for mode, Sin, Sout, cin, cout, has_d in encoder_convs():
        p = conv_plan(mode, Sin, Sout)
        fwd.append(("nn", rows, cout, p["f_nb"], p["f_minseg"] * (cin // 32)))
        if has_d:
            dgrad.append(("nt", rows, cin, p["d_nb"], p["d_minseg"] * (cout // 32)))
        wgrad.append(("tn", cin, cout, p["w_nb"], p["w_minseg"] * (rows // 32)))
    return fwd + dgrad + wgrad


def known_launches(model, rows):
    """Launches every gradient call of `model` over `rows` (padded) rows makes, as (form, M, N, batches, fewest K steps of a batch): the Dense
    layers 256 -> 1024 -> 256 both tapes have (the planner's step encoder, the IDM's residual blocks: csrc/train.hip dense_fwd / dense_dgrad /
    dense_wgrad) and, for the planner, the 256 -> 256 k = 5 convolution at 8 positions (three live taps at the ends; taps +-2 meet 6 positions).
    "encoder": every GEMM launch of the ResNet-18 tape (encoder_launches), forward and backward call together."""
    if model == "encoder":
        return encoder_launches(rows)
    out = [("nn", rows, 1024, 1, 8), ("nn", rows, 256, 1, 32), ("nt", rows, 1024, 1, 8), ("tn", 1024, 256, 1, rows // 32), ("tn", 256, 1024, 1, rows // 32)]
    if model == "planner":
        out += [("nn", rows, 256, 8, 3 * 8), ("nt", rows, 256, 8, 3 * 8), ("tn", 256, 256, 5, 6 * (rows // 32))]
    return out


def expected(model, rows, name):
    """-> (counters that must rise, counters that must stay) for one gradient call under configuration `name`: the table of the module's
    docstring where the batch allows it, else what the restated rule gives for the launches known_launches lists.  A launch that splits K
    finishes inside the launch where train_fuse_reduce is set and fused_part_bytes allows it, else through the reduce launch."""
    opt = options(name)
    must, finishes = set(), set()
    for form, M, N, nb, steps in known_launches(model, rows):
        tile, ks, ki = gemm_shape(M, N, nb, steps, opt)
        must.add(kernel_of(form, tile, ki))
        if ks > 1:
            finishes.add("fused" if opt["train_fuse_reduce"] and fused_part_bytes(M, N, nb, tile, ks) > 0 else "reduce")
    must |= finishes
    never = set()
    if not opt["train_big"]:
        never |= {k for k in KERNELS if k.endswith("_128")}
    if not opt["train_intra_split"]:
        never |= {k for k in KERNELS if k.endswith("_ki2")}
    if opt["train_small_wg"] == 0:
        never |= {k for k in KERNELS if "_32" in k}
    elif opt["train_small_wg"] == 1 << 20:                  # every M of the tapes is a multiple of 32
        never |= {k for k in KERNELS if "_64" in k}
    if not opt["train_split"]:
        never |= {"fused", "reduce"}
    if model == "encoder":                                  # known_launches lists every launch of this tape
        never |= (set(KERNELS) | {"fused", "reduce"}) - must
    elif not opt["train_fuse_reduce"]:
        never.add("fused")
    elif "reduce" not in finishes:
        never.add("reduce")
    assert not (must & never), (model, rows, name, must & never)
    return must, never


def read_counters(eng):
    return {c[len("stat_train_gemm_"):]: eng.get_option(c) for c in COUNTERS}


def check_counters(before, after, must, never, what):
    diff = {k: after[k] - before[k] for k in after}
    missing = sorted(k for k in must if diff[k] <= 0)
    extra = sorted(k for k in never if diff[k] != 0)
    assert not missing and not extra, f"{what}: did not run: {missing}; ran and must not: {extra}; launches: { {k: v for k, v in diff.items() if v} }"
    return diff


# ---- batches ------------------------------------------------------------------------------------------------------------------------------------
def planner_batch(B, seed):
    """-> dict(obs_emb (B, T + 1, D), t (B,), noise (B, T, D)) float32, as tests/test_hip_train.py draws them."""
    g = rng(seed)
    obs_emb = g.uniform(-1, 1, (B, T + 1, D)).astype(np.float32)
    return dict(obs_emb=obs_emb, t=g.integers(0, 100, B), noise=g.standard_normal((B, T, D)).astype(np.float32))


def idm_pool(rows, seed):
    """-> dict(s (rows, 2 D), a0 (rows, A), noise (rows, A), t (rows,)): IDM rows are independent of each other."""
    g = rng(seed)
    return dict(s=g.uniform(-1, 1, (rows, 2 * D)).astype(np.float32), a0=g.uniform(-1, 1, (rows, A)).astype(np.float32),
                noise=g.standard_normal((rows, A)).astype(np.float32), t=g.integers(0, 100, rows))


def take_rows(c, idx):
    return {k: v[idx] for k, v in c.items()}


def idm_preacts(ip, c, dtype):
    """Every ReLU input of the IDM for the rows of `c` (the three blocks' Dense_0 outputs and the final residual stream, as _relu_margins of
    tests/test_hip_train.py walks them), computed in `dtype` from the float64 noisy actions -> (rows, 3 * 1024 + 256) float64."""
    import torch.nn.functional as F
    P = torch32.TorchParams(ip, dtype=dtype)
    a = OT._add_noise(torch.tensor(c["a0"], dtype=torch.float64), torch.tensor(c["noise"], dtype=torch.float64), c["t"], 100).to(dtype)
    s = torch.tensor(c["s"], dtype=dtype)
    arg = torch.tensor(c["t"])[:, None].float() * torch32._freqs(256, "cpu")[None, :]
    e = F.mish(F.linear(torch.cat([torch.cos(arg), torch.sin(arg)], -1).to(dtype), P.t("MLP_0/Dense_0/kernel").t(), P.t("MLP_0/Dense_0/bias")))
    e = F.linear(e, P.t("MLP_0/Dense_1/kernel").t(), P.t("MLP_0/Dense_1/bias"))
    h = F.linear(torch.cat([a, s, e], -1), P.t("MLPResNet_0/Dense_0/kernel").t(), P.t("MLPResNet_0/Dense_0/bias"))
    pre = []
    for i in range(3):
        p = f"MLPResNet_0/MLPResNetBlock_{i}"
        y = F.layer_norm(h, (256,), P.t(f"{p}/LayerNorm_0/scale"), P.t(f"{p}/LayerNorm_0/bias"), eps=1e-6)
        u = F.linear(y, P.t(f"{p}/Dense_0/kernel").t(), P.t(f"{p}/Dense_0/bias"))
        pre.append(u)
        h = h + F.linear(F.relu(u), P.t(f"{p}/Dense_1/kernel").t(), P.t(f"{p}/Dense_1/bias"))
    pre.append(h)
    return torch.cat(pre, dim=1).double().numpy()


MARGIN_OVER_ROUNDOFF = 16.0


def idm_rows(ip, rows, seed):
    """`rows` IDM rows whose ReLU inputs stay clear of zero: a pool of 1.5 x rows, of which the rows with the largest margins (the smallest
    |ReLU input| of the row in float64) are kept -- never more than a third dropped.  A ReLU input within float32 round-off of zero gates
    differently in float32 than in float64 and moves the row's whole contribution to the gradient: no error of a kernel, and not comparable at
    1e-4.  -> (the rows, dict(kept_min, roundoff, ratio)); ratio = smallest kept margin / largest |float32 - float64| ReLU input of the pool,
    which the callers hold against MARGIN_OVER_ROUNDOFF."""
    assert rows % 2 == 0
    pool = idm_pool(rows * 3 // 2, seed)
    p64, p32 = idm_preacts(ip, pool, torch.float64), idm_preacts(ip, pool, torch.float32)
    margin = np.abs(p64).min(axis=1)
    keep = np.sort(np.argsort(-margin, kind="stable")[:rows])
    info = dict(kept_min=float(margin[keep].min()), roundoff=float(np.abs(p32 - p64).max()))
    info["ratio"] = info["kept_min"] / info["roundoff"]
    return take_rows(pool, keep), info


def idm_as_samples(c):
    """The rows as one-transition samples for oracle/train.py: obs_emb (rows, 2, D), actions (rows, 2, A)."""
    n = len(c["t"])
    return c["s"].reshape(n, 2, D), np.concatenate([c["a0"][:, None], np.zeros((n, 1, A), np.float32)], axis=1)


def oracle_planner(pp, c, alpha=1.0):
    r = OT.loss_and_grads(pp, None, c["obs_emb"], np.zeros((len(c["t"]), T + 1, A)), t_plan=c["t"], noise_plan=c["noise"], alpha_planner=alpha)
    return dict(loss=r["plan_loss"], grads=r["grads_planner"], g_norm=r["g_norm"])


def oracle_idm(ip, c, alpha=1.0):
    emb, act = idm_as_samples(c)
    r = OT.loss_and_grads(None, ip, emb, act, t_idm=c["t"], noise_idm=c["noise"], alpha_idm=alpha)
    return dict(loss=r["idm_loss"], grads=r["grads_idm"], g_norm=r["g_norm"])


# ---- the per-entry rule ----------------------------------------------------------------------------------------------------------------------
def every_entry(got, ref, factor=1e-4, scale=None, floor=None):
    """|got - ref| <= factor max|scale leaf| + 1e-12 on every entry of every leaf (scale = ref unless given) -> (report of the worst entry, the
    leaves over the bound as text).  floor = {leaf: figure}: the rule of DESIGN 4.11, max(factor max|scale leaf|, floor[leaf]) + 1e-12, whose
    callers pass three times the leaf's float32-against-float64 error."""
    worst, bad = dict(err_over_bound=0.0, leaf=None, at=None), []
    for k, r in ref.items():
        g, r = np.asarray(got[k], np.float64), np.asarray(r, np.float64)
        assert g.shape == r.shape, (k, g.shape, r.shape)
        bound = max(factor * float(np.abs(r if scale is None else scale[k]).max()), 0.0 if floor is None else float(floor[k])) + 1e-12
        err = np.abs(g - r)
        i = int(np.argmax(np.where(np.isnan(err), np.inf, err)))
        ratio = float(err.flat[i]) / bound
        if not ratio <= worst["err_over_bound"]:                 # (a NaN is the worst)
            worst = dict(err_over_bound=ratio, leaf=k, at=[int(x) for x in np.unravel_index(i, r.shape)])
        if not ratio <= 1.0:
            bad.append(f"{k}{tuple(worst['at'])}: got {g.flat[i]:.9e}, want {r.flat[i]:.9e}, |diff| / bound = {ratio:.3g}; "
                       f"{int((~(err <= bound)).sum())} of {err.size} entries over the bound")
    return worst, bad


def combine(chunks):
    """sum_c (|c| / B) G_c in float64 of [(samples in the chunk, gradient tree)]: the gradient of the mean loss over all the samples."""
    total = float(sum(n for n, _ in chunks))
    out = OrderedDict((k, np.zeros(np.shape(v), np.float64)) for k, v in chunks[0][1].items())
    for n, g in chunks:
        for k, v in g.items():
            out[k] += (n / total) * np.asarray(v, np.float64)
    return out
