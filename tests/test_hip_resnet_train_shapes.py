"""The ResNet-18 encoder's training tape (csrc/resnet_train.hpp) in every launch shape of the training GEMM family and at workload size.  -m gpu.

The tape makes 59 GEMM launches per forward + backward (20 forward, 19 data-gradient, 20 weight-gradient: tests/train_cases.py
encoder_launches restates their M, N, batches and K steps from the convolution tables).  Which instantiation each ran is read from the
handle's launch counters before the forward and after the backward and held against train_cases.expected("encoder", rows, cfg), which
for this tape is exact: every counter it does not list must stay.  tests/test_train_cpu.py checks that the cases of part A reach all 15
instantiations, the in-launch split-K finish and the reduce launch.

Frames.  A frame puts 190 000 values through a ReLU, and float32 round-off (up to 6e-6 on those values) gates one that lies nearer to zero
differently than float64 does: that element's whole contribution then moves, about 1 / sqrt(terms) of a leaf maximum, which is no error
of a kernel and not comparable at 1e-4.  129 frames of RO.synth_frames hold a ReLU input at 1.5e-8, and the first run of part A on such
a batch missed the bound 123-fold on ResNetBlock_4/Conv_0/kernel through ONE gate (channel 187 of that block's first norm, +7.8e-7 in
float64).  So every batch here is tiled from the 7 of 192 frames whose gates are clearest (TO.clear_frames: margin >= 3 x the largest
float32 deviation of any ReLU input of the pool; tests/test_dp_train_cpu.py), row i showing frame i % 7 -- rows 32, 64 and 128 apart
differ -- with its own random feature gradient.  The parameters are the perturbed ones of tests/test_hip_resnet_train.py.

A. N = 33 (64 padded rows) and N = 129 (160 rows: five 32-row tiles, a ragged second 128-row tile) under every option set the tape
   reads, against float64 autograd on all 11 176 512 entries: |got - ref64| <= max(1e-4 leafmax64, 3 err32_leaf) + 1e-12;
   and a backward that runs under other options than its forward (it re-sizes the split-K workspace in its own dry walk).
B. N = 512 (tools/dp_agent_bench.py --train) and 1024 (RNT_MAX_FRAMES) against the float64 sum of the gradient arenas of their 32-frame
   chunks run under the defaults, the shape part A and tests/test_hip_resnet_train.py pin: the VJP is linear in dfeat and GroupNorm is
   per sample, so G(batch) = sum_c G(chunk c).  Per entry 2e-4 max|G leaf| + 1e-12; features 2e-5 against the chunks' and against
   ldp_resnet_encode.
C. bit-equality: in-launch finish == reduce launch per tile family; stream placement (train_streams, train_sides) changes no bit.
D. max-pool ties: a stem whose output is exactly one pixel times a power of two over four-level frames (TO.tie_case) -- three quarters of
   the pool windows hold their positive maximum more than once -- under the rule of A.  tests/test_dp_train_cpu.py shows that the
   last-maximum and the split-evenly rules miss that bound by a factor > 100.
"""
import functools
import json

import numpy as np
import pytest
import torch

from tests import dp_resnet_oracle as RO
from tests import dp_train_oracle as TO
from tests import train_cases as TC
from tests.golden.make_golden_dp_resnet import frames_to_input
from tests.test_hip_resnet_train import SHAPES, _check_feat, _check_grads, _params
from tests.util import rng

pytestmark = pytest.mark.gpu

SPLITS = ["t32", "t64", "t128", "t128_64", "ki2_32", "ki2_64", "nosplit", "deep", "shallow", "reduce"]       # (the tape reads neither train_gn4 nor train_group_proj)
TILES = ["t32", "t64", "t128", "t128_64"]
#         case -> (frames, configurations)
CASES = dict(e33=(33, SPLITS), e129=(129, TILES))
SEED, POOL, DISTINCT = 1029, 192, 7                      # parameters and frame pool; distinct frames of a batch
WORKLOAD = [(512, "t32"), (512, "t128"), (512, "deep"), (1024, "t32")]
ENC = "encoder0"
_ON_DEVICE = []                                          # the case whose parameters the training arena of slot 0 holds


def _rows(N):
    return -(-N // 32) * 32


@functools.lru_cache(maxsize=None)
def _clear():
    """-> (the parameters, the DISTINCT clearest frames of the pool as encoder input), once per process."""
    torch.set_num_threads(16)
    p = _params("perturbed", SEED)
    frames, info = TO.clear_frames(p, DISTINCT, POOL, SEED)
    print("clear frames", json.dumps(info))
    assert info["ratio"] >= TO.GATE_MARGIN_OVER_ROUNDOFF, info
    return p, frames_to_input(frames)


def _tiled(N):
    """-> (frames (N, 64, 64, 3): row i shows clear frame i % DISTINCT; feature gradient (N, 1024), every row its own)."""
    x = _clear()[1][np.arange(N) % DISTINCT]
    return x, rng(SEED + N).standard_normal((N, RO.FEAT)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(N):
    """Inputs and both CPU references of one VJP case (computed once, shared, never modified), as tests/test_hip_resnet_train._case."""
    p = _clear()[0]
    x, dfeat = _tiled(N)
    f64, g64, _ = TO.encoder_vjp(p, x, dfeat, torch.float64)
    f32, g32, _ = TO.encoder_vjp(p, x, dfeat, torch.float32)
    return dict(p=p, x=x, dfeat=dfeat, f64=f64, f32=f32, g64=g64, g32=g32)


@pytest.fixture(scope="module")
def eng():
    from latent_diffusion_planning_amd.engine import HipEngine
    e = HipEngine(obs_dim=7, action_dim=7, global_cond_dim=1033, pred_horizon=16, action_horizon=8)
    _ON_DEVICE.clear()
    yield e
    torch.cuda.synchronize()
    e.close()


@pytest.fixture(autouse=True)
def _options_restored(eng):
    before = {k: eng.get_option(k) for k in TC.DEFAULTS}
    assert before == TC.DEFAULTS, before
    yield
    for k, v in before.items():
        eng.set_option(k, v)


def _configure(eng, name, **more):
    for k, v in dict(TC.options(name), **more).items():
        eng.set_option(k, v)


def _load(eng, key, params):
    if _ON_DEVICE != [key]:
        eng.train_load(ENC, params)
        _ON_DEVICE[:] = [key]


def _dev(x):
    return torch.tensor(x, device="cuda") if isinstance(x, np.ndarray) else x


def _run(eng, x, dfeat):
    """Forward and backward of slot 0 -> the features (device)."""
    feat = eng.train_encoder_forward(0, _dev(x))
    eng.train_encoder_backward(0, _dev(dfeat))
    return feat


def _attested(eng, x, dfeat, cfg, what, **more):
    """_run under configuration `cfg` (plus the options of `more`), the launch counters held against train_cases.expected."""
    _configure(eng, cfg, **more)
    before = TC.read_counters(eng)
    feat = _run(eng, x, dfeat)
    must, never = TC.expected("encoder", _rows(len(x)), cfg)
    diff = TC.check_counters(before, TC.read_counters(eng), must, never, f"{what}, {_rows(len(x))} rows, {cfg}")
    assert sum(v for k, v in diff.items() if k in TC.KERNELS) == 59, diff
    return feat, {k: v for k, v in diff.items() if v}


def _grads(eng):
    return eng.train_read(ENC, eng.TRAIN_GRADS, SHAPES)


def _arena(eng):
    return eng.train_arena(ENC, eng.TRAIN_GRADS).clone()


# ---- A. every configuration against float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cfg", [(n, c) for n, v in CASES.items() for c in v[1]])
def test_every_gradient_entry_matches_float64_in_every_launch_shape(name, cfg, eng):
    N = CASES[name][0]
    c = _case(N)
    _load(eng, "clear", c["p"])
    feat, ran = _attested(eng, c["x"], c["dfeat"], cfg, name)
    print("encoder shapes A", json.dumps(dict(case=name, cfg=cfg, rows=_rows(N), ran=ran)))
    _check_feat(f"{name} under {cfg}", feat.cpu().numpy(), c)
    _check_grads(f"{name} under {cfg}", _grads(eng), c)


def test_backward_under_other_options_than_its_forward(eng):
    """Forward under the defaults, backward under train_wg_target = 1536, on slot 1, whose lane nothing in this module has used: the
    backward's own dry walk finds deeper K splits than the forward's sized the partial workspace for (a lane's workspaces only grow), and
    must re-size it without touching the activations the forward kept."""
    c = _case(33)
    eng.train_load("encoder1", c["p"])
    expect = TC.expected("encoder", 64, "t32")
    assert expect == TC.expected("encoder", 64, "deep")                # the same kernels, split deeper
    _configure(eng, "t32")
    before = TC.read_counters(eng)
    feat = eng.train_encoder_forward(1, _dev(c["x"]))
    _configure(eng, "deep")
    eng.train_encoder_backward(1, _dev(c["dfeat"]))
    diff = TC.check_counters(before, TC.read_counters(eng), *expect, "forward t32, backward deep")
    assert diff["fused"] > 41, diff                                      # (41: what the whole call splits under the defaults)
    _check_feat("forward t32, backward deep", feat.cpu().numpy(), c)
    _check_grads("forward t32, backward deep", eng.train_read("encoder1", eng.TRAIN_GRADS, SHAPES), c)


# ---- B. workload sizes by decomposition ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def workload(eng):
    """1024 tiled frames (N = 512 takes the first half) and, once per module, their 32-frame chunks run under the defaults: the chunks' features
    and the running float64 sum of their gradient arenas, kept on the device after 16 and after 32 chunks.  `leaf` maps each leaf to its
    entries' places in the arena (read back from an arena filled with its own indices, which float32 holds exactly below 2^24)."""
    n, p = 1024, _clear()[0]
    x, dfeat = (torch.tensor(v, device="cuda") for v in _tiled(n))
    _load(eng, "clear", p)
    g = eng.train_arena(ENC, eng.TRAIN_GRADS)
    assert g.numel() < 1 << 24
    g.copy_(torch.arange(g.numel(), dtype=torch.float32, device="cuda"))
    leaf = {k: torch.tensor(v.astype(np.int64).ravel(), device="cuda") for k, v in _grads(eng).items()}
    assert sum(v.numel() for v in leaf.values()) == len(torch.unique(torch.cat(list(leaf.values())))) == 11176512
    g.zero_()
    total, feats, sums = torch.zeros(g.numel(), dtype=torch.float64, device="cuda"), [], {}
    for lo in range(0, n, 32):
        f, _ = _attested(eng, x[lo:lo + 32], dfeat[lo:lo + 32], "t32", f"chunk {lo // 32}")
        feats.append(f)
        total += g.double()
        if lo + 32 in (512, 1024):
            sums[lo + 32] = total.clone()
    eng.load_encoder(0, p)                                  # the sampling path on the same leaves
    enc = eng.resnet_encode(0, x)
    return dict(p=p, x=x, dfeat=dfeat, feats=torch.cat(feats), enc=enc, sums=sums, leaf=leaf)


@pytest.mark.parametrize("N,cfg", WORKLOAD)
def test_workload_batch_is_the_sum_of_its_chunks(N, cfg, eng, workload):
    w = workload
    _load(eng, "clear", w["p"])
    feat, ran = _attested(eng, w["x"][:N], w["dfeat"][:N], cfg, f"N={N}")
    arena = _arena(eng)
    got = _grads(eng)
    ref = {k: w["sums"][N][i].reshape(SHAPES[k]).cpu().numpy() for k, i in w["leaf"].items()}
    worst, bad = TC.every_entry(got, ref, 2e-4, scale=got)
    f_chunks, f_enc = float((feat - w["feats"][:N]).abs().max()), float((feat - w["enc"][:N]).abs().max())
    print("encoder shapes B", json.dumps(dict(N=N, cfg=cfg, **worst, feat_vs_chunks=f_chunks, feat_vs_encode=f_enc, ran=ran)))
    assert not bad, f"{N} frames under {cfg}: {len(bad)} leaves over the bound:\n" + "\n".join(bad[:20])
    assert f_chunks <= 2e-5 and f_enc <= 2e-5, (f_chunks, f_enc)
    for k, v in got.items():
        assert np.isfinite(v).all() and np.abs(v).max() > 0, k
    if N == 1024:
        _run(eng, w["x"][:N], w["dfeat"][:N])
        assert torch.equal(_arena(eng), arena), "two identical calls differ"


# ---- C. bitwise properties ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["t32", "t64", "t128"])
@pytest.mark.parametrize("name", list(CASES))
def test_in_launch_finish_equals_the_reduce_launch_in_every_tile_family(name, cfg, eng):
    c = _case(CASES[name][0])
    _load(eng, "clear", c["p"])
    _configure(eng, cfg, train_fuse_reduce=0)
    c0 = TC.read_counters(eng)
    f0 = _run(eng, c["x"], c["dfeat"]).clone()
    ref = _arena(eng)
    c1 = TC.read_counters(eng)
    assert c1["reduce"] > c0["reduce"] and c1["fused"] == c0["fused"], (c0, c1)
    assert torch.isfinite(ref).all() and float(ref.abs().max()) > 0
    eng.set_option("train_fuse_reduce", 1)
    for rep in range(2):
        f1 = _run(eng, c["x"], c["dfeat"])
        got = _arena(eng)
        assert torch.equal(f0, f1) and torch.equal(ref, got), (name, cfg, rep, int((ref != got).sum()))
    c2 = TC.read_counters(eng)
    assert c2["reduce"] == c1["reduce"] and c2["fused"] > c1["fused"], (c1, c2)


@pytest.mark.parametrize("name", list(CASES))
def test_stream_placement_changes_no_bit(name, eng):
    """train_streams = 0 (everything on the caller's stream) and train_sides = 2, 3 (the weight-gradient work dealt to more side streams) only
    change where launches are enqueued: the arena equals the default's bit for bit (a missing cross-stream dependency would show here)."""
    c = _case(CASES[name][0])
    _load(eng, "clear", c["p"])
    _run(eng, c["x"], c["dfeat"])
    ref = _arena(eng)
    assert torch.isfinite(ref).all() and float(ref.abs().max()) > 0
    for opt, v in (("train_streams", 0), ("train_sides", 2), ("train_sides", 3)):
        eng.set_option(opt, v)
        for rep in range(2):
            _run(eng, c["x"], c["dfeat"])
            got = _arena(eng)
            assert torch.equal(ref, got), (name, opt, v, rep, int((ref != got).sum()))
        eng.set_option(opt, TC.DEFAULTS[opt])


# ---- D. max-pool ties ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tie_case():
    p, frames = TO.tie_case()
    x = frames_to_input(frames)
    dfeat = rng(960 + 77).standard_normal((len(x), RO.FEAT)).astype(np.float32)
    f64, g64, _ = TO.encoder_vjp(p, x, dfeat, torch.float64)
    f32, g32, _ = TO.encoder_vjp(p, x, dfeat, torch.float32)
    _, stem, _ = TO.encode_t(TO.leaves_of(p), torch.as_tensor(x, dtype=torch.float64), return_maps=True)
    return dict(p=p, x=x, dfeat=dfeat, f64=f64, f32=f32, g64=g64, g32=g32, ties=TO.pool_ties(stem))


def test_max_pool_backward_takes_the_first_maximum_of_a_tied_window(eng):
    c = _tie_case()
    print(f"ties: {c['ties']} of {len(c['x']) * 64 * 16 * 16} pool windows hold their positive maximum more than once")
    assert c["ties"] >= 10000
    _load(eng, "ties", c["p"])
    feat, _ = _attested(eng, c["x"], c["dfeat"], "t32", "ties")
    _check_feat("ties", feat.cpu().numpy(), c)
    _check_grads("ties", _grads(eng), c)
