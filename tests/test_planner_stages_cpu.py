"""The checker of tests/test_hip_planner_stages.py must be able to fail (CPU, runs anywhere).

`planner_stage_cases.stage_error` -- the rule |got - ref64| <= max(1e-5, 3 err32) max(1, max|ref64|) -- is fed "device" outputs of one planner
stage (conv k = 5 + GroupNorm(8) + Mish + FiLM) computed on the planes of tests/split_emulate.py with fp32 accumulation: the correct two-fp16-
plane / three-product and three-bf16-plane / six-product arithmetic, and four defects a split-operand tile could have.  Shapes: the three
levels of the pred_horizon 8 U-Net.  Inputs: N(0, 1), and a heavy variant with every 7th input channel x 30 and one output channel x 100.

Measured here, 4 rows per case (err relative to max(1, max|ref64|); the bound is its 1e-5 floor in every case, err32 1.3e-7 .. 3.3e-7):
    fp16 planes x 3 (correct)                                   1.6e-7 .. 4.0e-7
    bf16 planes x 6 (correct)                                   1.4e-7 .. 3.4e-7
    low plane of one 32-channel K step never multiplied         5.0e-5 .. 8.2e-5   (N(0, 1) inputs; asserted there only)
    low-plane accumulator added with 2^-10 instead of 2^-11     2.1e-4 .. 3.7e-4
    the h l' product missing                                    1.2e-4 .. 3.3e-4
    one of the six bf16 products (m m) missing                  2.2e-6 .. 4.3e-6   -- UNDER the floor: the sensitivity limit of this check
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.planner_stage_cases import stage_error
from tests.split_emulate import H16_SCALE, PAIRS, planes, planes_f16
from tests.util import rng

SHAPES = [(2, 1024, 1024), (4, 1024, 512), (8, 512, 256)]
B = 4


def _problem(T, cin, cout, heavy):
    g = rng(50_000 + T * 7 + cin + cout + (1 if heavy else 0))
    x = g.standard_normal((B, cin, T))
    w = g.standard_normal((cout, cin, 5)) / np.sqrt(5 * cin)
    if heavy:
        x[:, ::7] *= 30.0
        w[int(g.integers(0, cout))] *= 100.0
    p = dict(x=x, w=w, b=0.1 * g.standard_normal(cout), gs=1 + 0.1 * g.standard_normal(cout), gb=0.1 * g.standard_normal(cout),
             film=g.standard_normal((B, 2 * cout)))
    return {k: torch.tensor(np.asarray(v, np.float32)) for k, v in p.items()}          # fp32 values: what a kernel is handed


def _stage(p, dtype, conv=None):
    """conv + bias, GroupNorm(8), Mish, FiLM in `dtype`; `conv(x, w)`: the contraction alone (default F.conv1d)"""
    q = {k: v.to(dtype) for k, v in p.items()}
    y = (F.conv1d(q["x"], q["w"], padding=2) if conv is None else conv(p["x"], p["w"]).to(dtype)) + q["b"][None, :, None]
    y = F.mish(F.group_norm(y, 8, q["gs"], q["gb"], eps=1e-6))
    c = y.shape[1]
    return q["film"][:, :c, None] * y + q["film"][:, c:, None]


def _c(a, b):
    return F.conv1d(a, b, padding=2)


def conv_f16(x, w, scale=1.0 / H16_SCALE, drop_hl=False, skip_step=None):
    """two fp16 planes, hh in one fp32 accumulator, h l' + l' h in a second one added with `scale`"""
    (xh, xl), (wh, wl) = planes_f16(x), planes_f16(w)
    if skip_step is not None:                      # the low planes of one 32-channel K step never reach the matrix pipe
        xl, wl = xl.clone(), wl.clone()
        xl[:, skip_step:skip_step + 32] = 0
        wl[:, skip_step:skip_step + 32] = 0
    low = _c(xl, wh) if drop_hl else _c(xh, wl) + _c(xl, wh)
    return _c(xh, wh) + low * scale


def conv_bf16(x, w, pairs=PAIRS[6]):
    xp, wp = planes(x), planes(w)
    tot = None
    for i, j in pairs:                             # small to large, fp32 accumulate
        t = _c(xp[i], wp[j])
        tot = t if tot is None else tot + t
    return tot


def _judge(p, conv):
    ref64, ref32 = _stage(p, torch.float64), _stage(p, torch.float32)
    e = stage_error(_stage(p, torch.float32, conv), ref64, ref32)
    assert e["bound"] == 1e-5, e                   # err32 sits at 0.03 of the floor: the floor is the bound
    return e


@pytest.mark.parametrize("heavy", [False, True], ids=["noise", "heavy"])
@pytest.mark.parametrize("T,cin,cout", SHAPES)
def test_the_correct_forms_pass(T, cin, cout, heavy):
    p = _problem(T, cin, cout, heavy)
    for name, conv in (("fp16 x 3", conv_f16), ("bf16 x 6", conv_bf16)):
        e = _judge(p, conv)
        print(f"T={T} {cin}->{cout} {'heavy' if heavy else 'noise'} {name}: err {e['err']:.2e} err32 {e['err32']:.2e} bound {e['bound']:.1e}")
        assert e["ok"] and e["err"] < 1e-6, (name, e)


@pytest.mark.parametrize("heavy", [False, True], ids=["noise", "heavy"])
@pytest.mark.parametrize("T,cin,cout", SHAPES)
def test_a_wrong_plane_scale_and_a_missing_product_fail(T, cin, cout, heavy):
    p = _problem(T, cin, cout, heavy)
    for name, conv in (("low accumulator x 2^-10", lambda x, w: conv_f16(x, w, scale=2.0 / H16_SCALE)),
                       ("h l' missing", lambda x, w: conv_f16(x, w, drop_hl=True))):
        e = _judge(p, conv)
        print(f"T={T} {cin}->{cout} {'heavy' if heavy else 'noise'} {name}: err {e['err']:.2e} = {e['err'] / e['bound']:.1f} x bound")
        assert not e["ok"] and e["err"] > 3 * e["bound"], (name, e)


@pytest.mark.parametrize("T,cin,cout", SHAPES)
def test_a_skipped_low_plane_step_fails_on_noise(T, cin, cout):
    p = _problem(T, cin, cout, False)
    e = _judge(p, lambda x, w: conv_f16(x, w, skip_step=96))
    print(f"T={T} {cin}->{cout} low plane of channels 96..127 skipped: err {e['err']:.2e} = {e['err'] / e['bound']:.1f} x bound")
    assert not e["ok"], e


@pytest.mark.parametrize("heavy", [False, True], ids=["noise", "heavy"])
@pytest.mark.parametrize("T,cin,cout", SHAPES)
def test_a_missing_mm_product_is_under_the_floor(T, cin, cout, heavy):
    """The sensitivity limit of the 1e-5 floor: five of the six bf16 products (m m, 2^-16 |x w| per term, missing) give 2e-6 .. 5e-6 and
    PASS.  A defect of this size in one stage is invisible to the per-stage check (DESIGN 4.7.2 says so); it is asserted here so that a
    change of the rule that moves the limit shows."""
    p = _problem(T, cin, cout, heavy)
    e = _judge(p, lambda x, w: conv_bf16(x, w, [q for q in PAIRS[6] if q != (1, 1)]))
    print(f"T={T} {cin}->{cout} {'heavy' if heavy else 'noise'} m m missing: err {e['err']:.2e} = {e['err'] / e['bound']:.2f} x bound")
    assert e["ok"] and e["err"] > 3 * e["err32"], e
