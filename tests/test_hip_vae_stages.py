"""Every stage of the StableVAE forward path on its own against float64, on the tiles the engine really runs.  -m gpu.

`HipEngine.vae_trace` (ldp_vae_trace) runs the encode_chunk / decode_chunk of vae_moments / vae_decode and copies every stage's output out
behind the stage.  For stage k the float64 stage function of oracle/torch32.py is applied to the GPU's OWN tapped input(s) of that stage, so no
error is inherited from earlier stages, and the bound is the project's rule:

    |got - ref64| <= max(1e-5, 3 * err32) * max(1, max|ref64|)

with err32 the error of the float32 evaluation of the same stage function on the same input, in the same units.  The trace table says which
kernel family ran each stage and where its GroupNorm took its statistics from; `_expected_path` states what the dispatch is meant to pick
 and every table is held against it, under the default options and under each option that moves a stage to another kernel.

Measured on the MI355X (worst err / bound per arithmetic form): DESIGN.md 4.7.1.
"""
import numpy as np
import pytest
import torch

from latent_diffusion_planning_amd import weights as W
from oracle import torch32
from tests.util import rng

pytestmark = pytest.mark.gpu

DEFAULTS = dict(vae_split=1, vae_split_f16=1, vae_split_s2=1, no_mb2=0, vae_split_gn_only=0, vae_no_conv_stats=0, vae_no_conv_in_stats=0)
_engines, _params = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


def _engine(S, LC):
    if (S, LC) not in _engines:
        from latent_diffusion_planning_amd.engine import HipEngine
        e = HipEngine(obs_dim=25, action_dim=7, global_cond_dim=25, pred_horizon=8, action_horizon=4, image_size=S, vae_latent_channels=LC)
        e.load_params(vae=_vae_params(LC)[0])
        _engines[(S, LC)] = e
    return _engines[(S, LC)]


def _vae_params(LC):
    if LC not in _params:
        vp = W.init_vae_params(W.VAESpec(latent_channels=LC), seed=2)
        _params[LC] = (vp, torch32.TorchParams(vp, dtype=torch.float64), torch32.TorchParams(vp, dtype=torch.float32))
    return _params[LC]


def _inputs(decode, N, S, LC, first=0, seed=0):
    """Rows of three kinds, row n of kind (first + n) % 3: 0 a smooth field (low-frequency gradient + 1e-2 noise), 1 nearly constant
    (0.3 + 1e-3 noise), 2 uniform noise over the whole input range ([-1, 1] for frames, [-3, 3] for latents).  Row n depends on (seed, n) only."""
    side, ch, amp = (S // 32, LC, 3.0) if decode else (S, 3, 1.0)
    out = np.empty((N, side, side, ch), np.float32)
    yy, xx = np.meshgrid(np.linspace(-1, 1, side), np.linspace(-1, 1, side), indexing="ij")
    for n in range(N):
        g = rng(7000 + 100 * seed + n + (50 if decode else 0))
        kind = (first + n) % 3
        if kind == 0:
            c = g.uniform(-0.5, 0.5, (ch, 3))
            f = np.stack([c[i, 0] * yy + c[i, 1] * xx + c[i, 2] * np.sin(2.0 * (xx + yy)) for i in range(ch)], -1)
            out[n] = amp * f + 1e-2 * g.standard_normal(f.shape)
        elif kind == 1:
            out[n] = 0.3 + 1e-3 * g.standard_normal((side, side, ch))
        else:
            out[n] = g.uniform(-amp, amp, (side, side, ch))
    return torch.tensor(out)


def _nchw(row, dtype):
    t = row["t"] if row["nchw"] else row["t"][..., :row["channels"]].permute(0, 3, 1, 2)
    return t.to("cpu", dtype).contiguous()


# ---- what the dispatch is meant to pick --------------------------------------------------------------------------------------------------
def _expected_path(rows, k, opts, decode):
    """(family, tile, fused_out, stats route) of stage k.  3x3 convs, stride 1: at 64 / 32 / 16 pixels with 128 | Cout on split operands
    (sconv3: two fp16 planes, or three bf16 planes with vae_split_f16 = 0) -- the upsamplers' convs only without vae_split_gn_only --, else an
    exact-fp32 tconv tile: four-wave 64 columns (4, 1, 2) when the row tiles by 8 pixels and 64 | Cin, Cout; (4, 1, 4) / stride 2 (4, 1, 2) on
    3-pixel rows; (2, 4, 1) otherwise.  The (4, 1, 2) tile runs on two fp16 planes for stride 2 and at 8 pixels (vae_split, vae_split_f16 and
    vae_split_s2 all on); stride 2 keeps (2, 4, 1) under no_mb2.  A conv leaves column sums when it is sconv3, or a stride-1 four-wave tile
    whose image has a multiple of 16 row tiles.  A GroupNorm reads its producer's sums when the producer left some (conv_in: its row sums)."""
    r = rows[k]
    N, Wd, ld, kind = r["t"].shape[0], r["t"].shape[2], r["t"].shape[-1], r["kind"]
    f16 = bool(opts["vae_split"] and opts["vae_split_f16"])
    fam, tile, fused = "none", (0, 0, 0), False
    if kind == "shortcut":
        fam, tile = "tconv_f32", (2, 4, 1)
    elif kind == "attn":
        fam, tile = "tconv_f32", (2, 4, 1)
    elif kind == "down":
        if Wd % 8 == 0 and not opts["no_mb2"]:
            fam, tile = ("tconv_f16x3" if f16 and opts["vae_split_s2"] else "tconv_f32"), (4, 1, 2)
        else:
            fam, tile = "tconv_f32", ((4, 1, 2) if Wd == 3 else (2, 4, 1))
    elif kind in ("res1", "res2", "up", "conv_out") or (kind == "conv_in" and decode):
        if Wd in (64, 32, 16) and ld % 128 == 0 and opts["vae_split"] and not (kind == "up" and opts["vae_split_gn_only"]):
            fam, fused = ("sconv_f16x3" if f16 else "sconv_bf16x6"), True
        else:
            to = 8 if Wd % 8 == 0 else 4 if Wd % 4 == 0 else 2 if Wd % 2 == 0 else 3
            tile = (4, 1, 4) if to == 3 else (4, 1, 2) if to == 8 and ld % 64 == 0 else (2, 4, 1)
            fused = tile[0] == 4 and (Wd * Wd // to) % 16 == 0
            fam = "tconv_f16x3" if Wd == 8 and tile == (4, 1, 2) and f16 and opts["vae_split_s2"] else "tconv_f32"
    route = "none"
    if kind in ("res1", "res2", "attn", "conv_out"):
        src = rows[r["inputs"][0]]
        if src["kind"] == "conv_in" and not decode:
            route = "gn_part" if opts["vae_no_conv_in_stats"] else "conv_in"
        else:
            route = "conv" if src["fused_out"] and not opts["vae_no_conv_stats"] else "gn_part"
    return fam, tile, fused, route


def _path(r):
    return r["family"], tuple(r["tile"]) if r["family"].startswith("tconv") else (0, 0, 0), r["fused_out"], r["stats"]


# ---- one traced run, checked ---------------------------------------------------------------------------------------------------------------
def _check_run(tag, eng, LC, x, decode, opts=DEFAULTS):
    """Traces x, checks every stage against float64 on its own tapped inputs, the table against `_expected_path`, the exact properties and the
    bitwise invariants.  -> (rows, out).  Misses are collected and reported together."""
    _, P64, P32 = _vae_params(LC)
    out, rows = eng.vae_trace(x.cuda(), decode=decode)
    out2, rows2 = eng.vae_trace(x.cuda(), decode=decode)
    plain = eng.vae_decode(x.cuda()) if decode else eng.vae_moments(x.cuda())
    eng.check_fault()
    bad = []
    if eng.get_option("range_fallback") != 0:
        bad.append("range_fallback set")
    if not torch.equal(rows[-1]["t"], out):
        bad.append("the last tap is not the returned output")
    if not torch.equal(out, plain):
        bad.append("the traced call's output differs from the untraced call's")
    if not (torch.equal(out, out2) and len(rows) == len(rows2) and all(torch.equal(a["t"], b["t"]) for a, b in zip(rows, rows2))):
        bad.append("a second traced call gave other bits")
    if not all(bool(torch.isfinite(r["t"]).all()) for r in rows):
        bad.append("non-finite tap")

    stages = torch32.vae_decode_stages(P64) if decode else torch32.vae_encode_stages(P64)
    main = [k for k, r in enumerate(rows) if r["kind"] != "upsampled"]          # table row of each oracle stage
    assert [rows[k]["kind"] for k in main] == [s[0] for s in stages], "the trace's stages are not the oracle's"
    x_nchw = x.permute(0, 3, 1, 2)
    for j, (k, (kind, name, inputs, fn)) in enumerate(zip(main, stages)):
        r = rows[k]
        want_in = tuple(-1 if i < 0 else main[i] for i in inputs)
        got_in = r["inputs"][:1] if kind == "up" else r["inputs"]               # (an upsampler's second input is its auxiliary row)
        if got_in != want_in:
            bad.append(f"stage {k} {name}: read stages {r['inputs']}, expected {want_in}")
            continue
        ins = [x_nchw if i < 0 else rows[i] for i in want_in]
        ref64 = fn(P64, *[(t if torch.is_tensor(t) else _nchw(t, torch.float64)).double() for t in ins])
        ref32 = fn(P32, *[(t if torch.is_tensor(t) else _nchw(t, torch.float32)).float() for t in ins]).double()
        got = _nchw(r, torch.float64)
        if got.shape != ref64.shape:
            bad.append(f"stage {k} {name}: shape {tuple(got.shape)} vs {tuple(ref64.shape)}")
            continue
        scale = max(1.0, float(ref64.abs().max()))
        err, err32 = float((got - ref64).abs().max()) / scale, float((ref32 - ref64).abs().max()) / scale
        bound = max(1e-5, 3.0 * err32)
        worst = int((got - ref64).abs().flatten(1).max(1).values.argmax())      # the batch row of the largest error
        path = _path(r)
        print(f"{tag} stage {k:2d} {kind:10s} {name:45s} {r['t'].shape[2]:3d}px {path[0]:12s} {path[1]} stats {path[3]:7s} fused_out {int(path[2])}"
              f"  err {err:.3e} err32 {err32:.3e} bound {bound:.3e} ratio {err / bound:.3f} row {worst}")
        if not (np.isfinite(err) and err <= bound):
            bad.append(f"stage {k} {name} [{path[0]} {path[1]}, stats {path[3]}]: err {err:.3e} > bound {bound:.3e} (err32 {err32:.3e})")
        want = _expected_path(rows, k, opts, decode)
        if path != want:
            bad.append(f"stage {k} {name}: ran {path}, expected {want}")
        # exact properties
        if not r["nchw"] and r["t"].shape[-1] > r["channels"] and bool((r["t"][..., r["channels"]:] != 0).any()):
            bad.append(f"stage {k} {name}: padded channels are not zero")
        if kind == "up":
            aux, src = rows[r["inputs"][1]], rows[r["inputs"][0]]
            if aux["kind"] != "upsampled" or aux["inputs"] != (r["inputs"][0],) or \
                    not torch.equal(aux["t"], src["t"].repeat_interleave(2, 1).repeat_interleave(2, 2)):
                bad.append(f"stage {k} {name}: the upsampled tensor is not the pixel replication of stage {r['inputs'][0]}")
        if kind == "nchw" and not torch.equal(r["t"], rows[r["inputs"][0]]["t"][..., :3].permute(0, 3, 1, 2)):
            bad.append(f"stage {k}: the NCHW transpose is not exact")
    assert not bad, f"{tag}: {len(bad)} miss(es):\n  " + "\n  ".join(bad)
    return rows, out


def _run(S, LC, N, decode, first=0, opts=None):
    eng = _engine(S, LC)
    o = dict(DEFAULTS, **(opts or {}))
    tag = f"{S}px LC{LC} N{N} {'dec' if decode else 'enc'}" + "".join(f" {k}={v}" for k, v in (opts or {}).items())
    try:
        for k, v in (opts or {}).items():
            eng.set_option(k, v)
        return _check_run(tag, eng, LC, _inputs(decode, N, S, LC, first), decode, o)
    finally:
        for k in (opts or {}):
            eng.set_option(k, DEFAULTS[k])


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decode", [False, True], ids=["encode", "decode"])
@pytest.mark.parametrize("N", [1, 2, 3])
def test_stages_64px(N, decode):
    """The attention's q|k|v as one MFMA 1x1 conv with row stride 3 C: N = 2 fills its 8-row group, N = 1 and 3 (N * T no multiple of 8)
    leave the last one ragged.  The 2- and 4-pixel levels' row tiles are ragged inside a 16-row block."""
    rows, _ = _run(64, 4, N, decode)
    assert [(r["family"], tuple(r["tile"])) for r in rows if r["kind"] == "attn"] == [("tconv_f32", (2, 4, 1))]
    fams = {r["family"] for r in rows}
    assert {"sconv_f16x3", "tconv_f16x3", "tconv_f32"} <= fams and "sconv_bf16x6" not in fams
    assert {r["stats"] for r in rows} >= ({"conv", "gn_part"} | (set() if decode else {"conv_in"}))


@pytest.mark.parametrize("decode", [False, True], ids=["encode", "decode"])
def test_stages_96px(decode):
    """Levels of 96 / 48 / 24 / 12 / 6 / 3 pixels: 8-, 4-, 2- and 3-pixel row tiles, T = 9 attention (18 rows: a ragged 8-row group)."""
    rows, _ = _run(96, 4, 2, decode, first=2)
    tiles = {(r["t"].shape[2], tuple(r["tile"])) for r in rows if r["family"].startswith("tconv") and r["kind"] not in ("shortcut", "attn")}
    assert {(3, (4, 1, 4)), (12, (2, 4, 1)), (6, (2, 4, 1))} <= tiles and ((3, (4, 1, 2)) in tiles or decode)
    assert [r["family"] for r in rows if r["kind"] == "attn"] == ["tconv_f32"]


def test_stages_128px_encode():
    """T = 16 attention at N = 1; the 128-pixel level on the exact-fp32 four-wave tile with fused column sums."""
    rows, _ = _run(128, 4, 1, False, first=1)
    assert [r["family"] for r in rows if r["kind"] == "attn"] == ["tconv_f32"]
    assert all(r["family"] == "tconv_f32" and tuple(r["tile"]) == (4, 1, 2) and r["fused_out"] for r in rows if r["t"].shape[2] == 128 and r["kind"] in ("res1", "res2"))


@pytest.mark.parametrize("decode", [False, True], ids=["encode", "decode"])
def test_stages_8_latent_channels(decode):
    """tiny_dense (quant_conv / post_quant_conv) at the other width."""
    rows, out = _run(64, 8, 2, decode, first=1)
    assert rows[0 if decode else -1]["channels"] == (8 if decode else 16)


OPTION_SETS = [("vae_split", 0, (False, True)), ("vae_split_f16", 0, (False, True)), ("vae_split_s2", 0, (False, True)), ("no_mb2", 1, (False,)),
               ("vae_split_gn_only", 1, (True,)), ("vae_no_conv_stats", 1, (False, True)), ("vae_no_conv_in_stats", 1, (False,))]


@pytest.mark.parametrize("name,value,decode", [(n, v, d) for n, v, sides in OPTION_SETS for d in sides],
                         ids=[f"{n}={v}-{'decode' if d else 'encode'}" for n, v, sides in OPTION_SETS for d in sides])
def test_stages_under_option(name, value, decode):
    """Each option that moves stages to another kernel or another statistics route: every stage still meets the bound, the stages the
    option is about changed path as `_expected_path` says, and no other stage changed."""
    eng = _engine(64, 4)
    x = _inputs(decode, 2, 64, 4)
    _, base = eng.vae_trace(x.cuda(), decode=decode)
    rows, _ = _run(64, 4, 2, decode, opts={name: value})
    opts = dict(DEFAULTS, **{name: value})
    moved = [k for k in range(len(rows)) if _path(rows[k]) != _path(base[k])]
    want = [k for k in range(len(rows)) if _expected_path(rows, k, opts, decode) != _expected_path(base, k, DEFAULTS, decode)]
    print(f"{name}={value}: stages moved {moved}")
    assert moved == want and moved, (moved, want)
    about = {"vae_split": ("sconv_f16x3", "tconv_f16x3"), "vae_split_f16": ("sconv_f16x3", "tconv_f16x3"), "vae_split_s2": ("tconv_f16x3",)}
    if name in about:                  # every stage of the families the option is about left them, for the family the option names
        assert all((base[k]["family"] in about[name]) == (k in moved) for k in range(len(rows)))
        assert all(rows[k]["family"] == ("sconv_bf16x6" if name == "vae_split_f16" and base[k]["family"] == "sconv_f16x3" else "tconv_f32")
                   for k in moved)
    elif name == "no_mb2":
        assert all(base[k]["kind"] == "down" and tuple(rows[k]["tile"]) == (2, 4, 1) and rows[k]["family"] == "tconv_f32" for k in moved)
    elif name == "vae_split_gn_only":
        assert all(base[k]["kind"] == "up" and rows[k]["family"] == "tconv_f32" and tuple(rows[k]["tile"]) == (4, 1, 2) for k in moved)
    elif name == "vae_no_conv_stats":
        assert all(base[k]["stats"] == "conv" and rows[k]["stats"] == "gn_part" for k in moved) and not any(r["stats"] == "conv" for r in rows)
    else:
        assert [(base[k]["stats"], rows[k]["stats"]) for k in moved] == [("conv_in", "gn_part")]


@pytest.mark.parametrize("decode", [False, True], ids=["encode", "decode"])
def test_rows_do_not_depend_on_the_batch(decode):
    """The same two frames traced alone and as rows 0-1 of an N = 3 batch: the same bits for those rows in every tap.  (Until this test the
    attention ran its four Dense layers on a VALU kernel whenever N * T was no multiple of 8: stages from the attention on differed by up to
    2.4e-6 between the two batches.)"""
    eng = _engine(64, 4)
    x3 = _inputs(decode, 3, 64, 4)
    _, r2 = eng.vae_trace(x3[:2].contiguous().cuda(), decode=decode)
    _, r3 = eng.vae_trace(x3.cuda(), decode=decode)
    eng.check_fault()
    assert len(r2) == len(r3)
    bad = []
    for k, (a, b) in enumerate(zip(r2, r3)):
        if not torch.equal(a["t"], b["t"][:2]):
            d = float((a["t"] - b["t"][:2]).abs().max())
            bad.append(f"stage {k} {a['kind']} [{a['family']} / {b['family']}]: max |diff| {d:.3e}")
    assert not bad, f"{len(bad)} tap(s) differ:\n  " + "\n  ".join(bad)
