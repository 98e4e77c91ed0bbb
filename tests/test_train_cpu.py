"""CPU checks of the training-step oracle and host logic (oracle/train.py, latent_diffusion_planning_amd/schedule.py): analytic known answers for
optax.adam and warmup_cosine_decay_schedule as restated, the autograd definition against central differences, the product's schedule against the
oracle's, the digests the goldens keep; and what tests/test_hip_train_shapes.py and tests/test_hip_resnet_train_shapes.py rest on
(tests/train_cases.py): the batch decomposition, the IDM row selection, the restated launch-shape rule, the encoder tape's restated launches."""
import math

import numpy as np
import pytest

from latent_diffusion_planning_amd.schedule import warmup_cosine_decay_schedule
from oracle import train as OT
from tests.util import idm_params, leaf_digest, rng


def test_warmup_cosine_schedule_known_answers():
    """optax 0.2.2: linear init -> peak over warmup_steps, then cosine from peak to end over decay_steps - warmup_steps, constant afterwards."""
    for mk in (OT.warmup_cosine_decay_schedule, warmup_cosine_decay_schedule):
        f = mk(1e-6, 1e-4, 1000, 500000, 1e-6)
        assert f(0) == pytest.approx(1e-6, rel=1e-12) and f(500) == pytest.approx((1e-6 + 1e-4) / 2, rel=1e-12) and f(1000) == pytest.approx(1e-4, rel=1e-12)
        mid = 1000 + (500000 - 1000) // 2
        assert f(mid) == pytest.approx(1e-4 * ((1 - 0.01) * 0.5 * (1 + math.cos(math.pi * (mid - 1000) / 499000)) + 0.01), rel=1e-12)
        assert f(500000) == pytest.approx(1e-6, rel=1e-9) and f(10**7) == pytest.approx(1e-6, rel=1e-9)
    a, b = OT.warmup_cosine_decay_schedule(1e-6, 1e-4, 500, 100000, 1e-6), warmup_cosine_decay_schedule(1e-6, 1e-4, 500, 100000, 1e-6)
    assert all(a(c) == b(c) for c in (0, 1, 499, 500, 501, 7777, 99999, 100000, 200000))
    with pytest.raises(ValueError):
        warmup_cosine_decay_schedule(1e-6, 1e-4, 10, 10, 1e-6)


def test_adam_restatement_known_answers():
    """Two steps by hand: g1 = (2, -4), g2 = (1, 0), constant lr 0.1, b1 0.9, b2 0.999, eps 1e-8 (optax.adam semantics: bias-corrected moments,
    eps added OUTSIDE the square root, learning rate read at the count BEFORE the increment)."""
    p = {"w": np.array([1.0, 1.0])}
    st = OT.adam_init(p)
    lr = lambda c: 0.1 if c == 0 else 0.2                      # noqa: E731
    p1, st = OT.adam_apply(p, {"w": np.array([2.0, -4.0])}, st, lr)
    assert st["count"] == 1 and np.allclose(st["mu"]["w"], [0.2, -0.4]) and np.allclose(st["nu"]["w"], [0.004, 0.016])
    assert np.allclose(p1["w"], [1 - 0.1 * 2 / (2 + 1e-8), 1 + 0.1 * 4 / (4 + 1e-8)], rtol=0, atol=1e-15)      # first step: -lr * sign(g)
    p2, st = OT.adam_apply(p1, {"w": np.array([1.0, 0.0])}, st, lr)
    mu = np.array([0.9 * 0.2 + 0.1 * 1.0, 0.9 * -0.4]); nu = np.array([0.999 * 0.004 + 0.001 * 1.0, 0.999 * 0.016])
    want = p1["w"] - 0.2 * (mu / (1 - 0.9 ** 2)) / (np.sqrt(nu / (1 - 0.999 ** 2)) + 1e-8)
    assert st["count"] == 2 and np.allclose(p2["w"], want, rtol=0, atol=1e-15)


def test_autograd_definition_against_central_differences():
    """oracle/train.py DEFINES jax.grad(loss) as float64 torch autograd; here a few entries of three IDM leaves against central differences of the
    float64 loss itself."""
    D, A, B, T = 25, 7, 2, 8
    ip = {k: np.asarray(v, np.float64) for k, v in idm_params(D=D, A=A).items()}
    g = rng(5)
    emb, act = g.uniform(-1, 1, (B, T + 1, D)), g.uniform(-1, 1, (B, T + 1, A))
    nz = dict(t_idm=g.integers(0, 100, B * T), noise_idm=g.standard_normal((B * T, A)))
    ref = OT.loss_and_grads(None, ip, emb, act, **nz)
    for leaf, idx in (("MLPResNet_0/MLPResNetBlock_1/Dense_0/kernel", (3, 17)), ("MLPResNet_0/MLPResNetBlock_0/LayerNorm_0/scale", (5,)),
                      ("MLP_0/Dense_0/bias", (11,)), ("MLPResNet_0/Dense_1/kernel", (100, 2))):
        h = 1e-6
        vals = []
        for sgn in (+1, -1):
            q = dict(ip)
            w = ip[leaf].copy()
            w[idx] += sgn * h
            q[leaf] = w
            vals.append(OT.loss_and_grads(None, q, emb, act, **nz)["idm_loss"])
        fd = (vals[0] - vals[1]) / (2 * h)
        assert ref["grads_idm"][leaf][idx] == pytest.approx(fd, rel=2e-5, abs=1e-9), leaf


def test_update_gates_restatement():
    cfg = dict(update_planner_every=2, update_idm_every=1, update_idm_after=3, update_planner_until=6, update_planner_after=2)
    got = [OT.update_gates(cfg, True, True, s) for s in range(8)]
    assert got == [(False, False), (False, False), (True, False), (False, True), (True, True), (False, True), (False, True), (False, True)]


def test_leaf_digest_is_deterministic_and_sensitive():
    a = rng(1).standard_normal((5, 300, 40))
    d0, d1 = leaf_digest(a, 3), leaf_digest(a.copy(), 3)
    assert np.array_equal(d0, d1) and d0.shape == (67,) and d0[0] == pytest.approx(np.sqrt((a * a).sum())) and d0[1] == np.abs(a).max()
    b = a.copy(); b[2, 7, 9] += 1e-3
    assert not np.array_equal(leaf_digest(b, 3)[:3], d0[:3])


def test_hierarchical_losses_shapes_and_central_differences():
    """agent/ldp_hier_agent.py:111-137 as oracle/train.py restates it: the planner trains on every idm_horizon-th future state, the IDM (a
    two-level U-Net) on chunks of idm_horizon actions per (state, state + idm_horizon) pair; its autograd gradient against central differences of
    the float64 loss, and the loss against the rearranges written out by hand."""
    import torch
    from oracle import torch32
    from tests.cases import HIER_IDM_DOWN, hier_idm_params
    D, A, B, ih, Tp = 25, 7, 2, 4, 4
    H = 1 + Tp * ih
    ip = {k: np.asarray(v, np.float64) for k, v in hier_idm_params(A, D).items()}
    g = rng(9)
    emb, act = g.uniform(-1, 1, (B, H, D)), g.uniform(-1, 1, (B, H, A))
    K = Tp
    nz = dict(t_idm=g.integers(0, 100, B * K), noise_idm=g.standard_normal((B * K, ih, A)))
    kw = dict(idm_horizon=ih, idm_unet_kw=dict(down_dims=HIER_IDM_DOWN))
    ref = OT.loss_and_grads(None, ip, emb, act, **nz, **kw)
    # by hand: pair k of sample b = (frame 4 k, frame 4 k + 4), its chunk = actions 4 k .. 4 k + 3
    P = torch32.TorchParams(ip, dtype=torch.float64)
    tot = 0.0
    for b in range(B):
        for k in range(K):
            r = b * K + k
            s = np.concatenate([emb[b, ih * k], emb[b, ih * k + ih]])[None]
            a0 = act[b, ih * k: ih * k + ih][None]
            noisy = OT._add_noise(torch.tensor(a0), torch.tensor(nz["noise_idm"][r:r + 1]), nz["t_idm"][r:r + 1], 100)
            pred = torch32.unet_forward(P, noisy, torch.tensor(nz["t_idm"][r:r + 1]), torch.tensor(s), down_dims=HIER_IDM_DOWN)
            tot += float(((pred - torch.tensor(nz["noise_idm"][r:r + 1])) ** 2).sum())
    assert ref["idm_loss"] == pytest.approx(tot / (B * K * ih * A), rel=1e-12)
    for leaf, idx in (("ConditionalResidualBlock1D_2/Conv1dBlock_0/Conv_0/kernel", (2, 100, 300)), ("Upsample1d_0/ConvTranspose_0/kernel", (1, 5, 9)),
                      ("Conv1dBlock_0/GroupNorm_0/scale", (17,)), ("ConditionalResidualBlock1D_0/Dense_0/kernel", (260, 3))):
        h = 1e-6
        vals = []
        for sgn in (+1, -1):
            q = dict(ip)
            w = ip[leaf].copy()
            w[idx] += sgn * h
            q[leaf] = w
            vals.append(OT.loss_and_grads(None, q, emb, act, **nz, **kw)["idm_loss"])
        fd = (vals[0] - vals[1]) / (2 * h)
        assert ref["grads_idm"][leaf][idx] == pytest.approx(fd, rel=2e-5, abs=1e-9), (leaf, idx)
    # the planner's targets: frames 1, 5, 9, 13
    from tests.util import planner_params
    pp = {k: np.asarray(v, np.float64) for k, v in planner_params(D=D).items()}
    nzp = dict(t_plan=g.integers(0, 100, B), noise_plan=g.standard_normal((B, Tp, D)))
    lp = OT.loss_and_grads(pp, None, emb, act, **nzp, **kw)
    PP = torch32.TorchParams(pp, dtype=torch.float64)
    noisy = OT._add_noise(torch.tensor(emb[:, 1::ih]), torch.tensor(nzp["noise_plan"]), nzp["t_plan"], 100)
    pred = torch32.unet_forward(PP, noisy, torch.tensor(nzp["t_plan"]), torch.tensor(emb[:, 0]))
    assert lp["plan_loss"] == pytest.approx(float(((pred - torch.tensor(nzp["noise_plan"])) ** 2).mean()), rel=1e-12)


# ---- what tests/test_hip_train_shapes.py rests on ------------------------------------------------------------------------------------------
def test_batch_gradient_is_the_weighted_sum_of_chunk_gradients_in_float64():
    """The loss is a mean over samples, GroupNorm is per sample and LayerNorm per row: G(batch) = sum_c (|c| / B) G(chunk c).  B = 5 as 3 + 2."""
    from tests import train_cases as TC
    from tests.util import planner_params
    pp, ip = planner_params(D=TC.D), idm_params(D=TC.D, A=TC.A)
    for what, run, c in (("planner", lambda c: TC.oracle_planner(pp, c), TC.planner_batch(5, 61)),
                         ("idm", lambda c: TC.oracle_idm(ip, c), TC.idm_pool(5, 62))):
        full = run(c)
        parts = [(n, run(TC.take_rows(c, sl))) for n, sl in ((3, slice(0, 3)), (2, slice(3, 5)))]
        comb = TC.combine([(n, r["grads"]) for n, r in parts])
        worst = max(float(np.abs(comb[k] - v).max()) / max(float(np.abs(v).max()), 1e-300) for k, v in full["grads"].items())
        print(f"{what}: |G(5) - (3 G(0:3) + 2 G(3:5)) / 5| <= {worst:.1e} of the leaf maximum")
        assert worst <= 1e-12
        assert sum(n / 5 * r["loss"] for n, r in parts) == pytest.approx(full["loss"], rel=1e-12)


@pytest.mark.parametrize("rows,seed", [(24, 2024), (320, 2320), (2048, 3048)])
def test_idm_row_selection_keeps_relu_inputs_clear_of_float32_round_off(rows, seed):
    """The batches of tests/test_hip_train_shapes.py (same seeds): the smallest kept margin is at least 16 x the largest |float32 - float64| ReLU
    input of the pool, a third of the pool is dropped, and the margin is _relu_margins of tests/test_hip_train.py applied per row."""
    from tests import train_cases as TC
    from tests.test_hip_train import _relu_margins
    ip = idm_params(D=TC.D, A=TC.A)
    c, info = TC.idm_rows(ip, rows, seed)
    print(f"IDM row selection, {rows} rows of {rows * 3 // 2}: smallest kept margin {info['kept_min']:.2e}, round-off {info['roundoff']:.2e}, ratio {info['ratio']:.1f}")
    assert info["ratio"] >= TC.MARGIN_OVER_ROUNDOFF, info
    assert len(c["t"]) == rows and all(len(v) == rows for v in c.values())
    emb, act = TC.idm_as_samples(c)
    m = _relu_margins(ip, emb, act, dict(noise_idm=c["noise"], t_idm=c["t"]))
    assert m.shape == (rows,) and m.min() == pytest.approx(info["kept_min"], rel=1e-9)
    pool = TC.idm_pool(rows * 3 // 2, seed)
    emb, act = TC.idm_as_samples(pool)
    mp = np.sort(_relu_margins(ip, emb, act, dict(noise_idm=pool["noise"], t_idm=pool["t"])))
    assert mp[len(mp) - rows] == pytest.approx(info["kept_min"], rel=1e-9)            # exactly the rows with the largest margins were kept


def test_restated_gemm_shape_rule_known_answers():
    """csrc/train.hip gemm_shape as tests/train_cases.py restates it, against cases worked out by hand -> (tile rows, K split, quartets)."""
    from tests import train_cases as TC
    o = lambda **kw: dict(TC.DEFAULTS, **kw)          # noqa: E731
    #      M,   N,  batches, K steps, options                      -> tile, ks, ki
    table = [
        (32, 1024, 1, 8, o(), (32, 4, 1)),                         # 16 tiles: x2 (4 steps each), x4 (2 steps each); x8 would leave one step
        (32, 1024, 1, 8, o(train_intra_split=1), (32, 2, 2)),      # the first factor of two inside the work-group
        (32, 1024, 1, 8, o(train_small_wg=0), (64, 4, 1)),         # a half-empty 64-row tile
        (96, 1024, 1, 8, o(train_small_wg=0), (64, 4, 1)),         # 32 tiles, the second row of them half empty
        (36, 1024, 1, 8, o(), (64, 4, 1)),                         # M no multiple of 32: never the 32-row tile
        (160, 256, 8, 24, o(train_big=1), (128, 8, 1)),            # 2 x 2 x 8 = 32 tiles: x8 (3 steps each) = 256 work-groups; x16 would leave one step
        (160, 256, 8, 24, o(train_big=1, train_intra_split=1), (128, 8, 1)),      # no two-quartet form of the 128-row tile
        (64, 1024, 1, 8, o(train_big=1), (32, 4, 1)),              # M < 128: not the 128-row tile
        (256, 64, 1, 8, o(train_big=1), (32, 4, 1)),               # N < 128: neither; 8 tiles
        (256, 1024, 1, 1, o(), (32, 1, 1)),                        # a weight gradient over 32 rows: one K step, no split
        (256, 1024, 1, 1, o(train_intra_split=1), (32, 1, 1)),     # ... and nothing to hand to a second quartet
        (32, 1024, 1, 8, o(train_split=0), (32, 1, 1)),
        (32, 1024, 1, 8, o(train_wg_target=48), (32, 4, 1)),       # 16 -> 32 -> 64 work-groups
        (32, 1024, 1, 64, o(train_wg_target=48), (32, 4, 1)),      # the target stops it, not the depth
        (32, 1024, 1, 64, o(train_wg_target=1536), (32, 32, 1)),   # 16 x 32 = 512 < 1536: the cap of 32
        (32, 64, 1, 4096, o(), (32, 32, 1)),                       # one tile, K deep: the cap of 32
        (256, 256, 5, 48, o(), (32, 4, 1)),                        # 4 x 8 x 5 = 160 tiles -> 320 (< 384) -> 640: split while the launch is below the target
    ]
    for M, N, nb, steps, opt, want in table:
        assert TC.gemm_shape(M, N, nb, steps, opt) == want, (M, N, nb, steps, want)
    assert TC.gemm_shape(32, 1024, 1, 8, o(), can_split=False) == (32, 1, 1)
    assert TC.kernel_of("tn", 64, 2) == "tn_64_ki2" and TC.kernel_of("nn", 128, 1) == "nn_128" and len(TC.KERNELS) == 15 and len(TC.COUNTERS) == 17


def test_the_shape_cases_reach_every_training_gemm_instantiation():
    """Over the (case, configuration) pairs tests/test_hip_train_shapes.py runs against the float64 oracle, the counters it requires to rise
    cover all 15 instantiations, the in-launch split-K finish and the reduce launch; and no requirement contradicts a prohibition."""
    from tests import train_cases as TC
    from tests.test_hip_train_shapes import CASES
    seen = set()
    for name, (model, n, _, cfgs) in CASES.items():
        for cfg in cfgs:
            must, never = TC.expected(model, -(-n // 32) * 32, cfg)
            seen |= must
    assert seen == set(TC.KERNELS) | {"fused", "reduce"}, sorted((set(TC.KERNELS) | {"fused", "reduce"}) - seen)
    # the table's cells at the batches that can reach them
    assert {"nn_32", "nt_32", "tn_32", "fused"} <= TC.expected("planner", 64, "t32")[0]
    assert {"nn_64", "nt_64", "tn_64"} <= TC.expected("planner", 32, "t64")[0]
    assert {"nn_128", "nt_128", "tn_128"} <= TC.expected("planner", 160, "t128")[0] and {"nn_128", "nt_128", "tn_128"} <= TC.expected("idm", 320, "t128")[0]
    assert "tn_128" in TC.expected("planner", 64, "t128")[0] and not {"nn_128", "nt_128"} & TC.expected("planner", 64, "t128")[0]
    assert {"tn_128", "nn_64", "nt_64"} <= TC.expected("planner", 64, "t128_64")[0]
    assert {"nn_32_ki2", "nt_32_ki2", "tn_32_ki2"} <= TC.expected("planner", 32, "ki2_32")[0]
    assert {"nn_64_ki2", "nt_64_ki2", "tn_64_ki2"} <= TC.expected("planner", 32, "ki2_64")[0] and {"nn_64_ki2", "nt_64_ki2", "tn_64_ki2"} <= TC.expected("idm", 320, "ki2_64")[0]
    assert "fused" in TC.expected("planner", 64, "deep")[0] and "reduce" in TC.expected("idm", 32, "reduce")[0]


def test_the_encoder_cases_reach_every_training_gemm_instantiation():
    """tests/test_hip_resnet_train_shapes.py, part A: the ResNet-18 tape's 59 GEMM launches as tests/train_cases.py restates them from the
    convolution tables (tap_2d / plan_taps of csrc/train_tables.hpp), the launch-table facts the restatement rests on worked out by hand, and
    the counters the (case, configuration) pairs require covering all 15 instantiations, the in-launch finish and the reduce launch."""
    from tests import train_cases as TC
    from tests.test_hip_resnet_train_shapes import CASES, WORKLOAD
    # a 3x3 at 2x2 pixels: every output pixel sees 4 live taps, every input pixel is read 4 times, the centre tap is live at all 4 pixels and a corner tap at 1
    assert TC.conv_plan(TC.VC_S1, 2, 2) == dict(f_nb=4, f_minseg=4, d_nb=4, d_minseg=4, w_nb=9, w_minseg=1)
    # 3x3 stride 2 pad (0, 1), 4 -> 2: the last output row / column loses a tap row / column; input pixel (0, 0) is read once
    assert TC.conv_plan(TC.VC_S2, 4, 2) == dict(f_nb=4, f_minseg=4, d_nb=16, d_minseg=1, w_nb=9, w_minseg=1)
    # the stride-2 1x1: the pixels it skips have data-gradient batches without segments
    assert TC.conv_plan(TC.VC_P2, 16, 8) == dict(f_nb=64, f_minseg=1, d_nb=256, d_minseg=0, w_nb=1, w_minseg=64)
    assert TC.conv_plan(TC.VC_P1, 32, 32) == dict(f_nb=1024, f_minseg=1, d_nb=1024, d_minseg=1, w_nb=1, w_minseg=1024)
    convs = TC.encoder_convs()
    assert len(convs) == 20 and sum(1 for c in convs if c[0] == TC.VC_P2) == 3 and convs[0] == (TC.VC_P1, 32, 32, 160, 64, False)
    assert convs[-1] == (TC.VC_S1, 2, 2, 512, 512, True)
    for rows in (32, 64, 160, 512, 1024):
        L = TC.known_launches("encoder", rows)
        assert [f for f, *_ in L] == ["nn"] * 20 + ["nt"] * 19 + ["tn"] * 20
        assert L[0] == ("nn", rows, 64, 1024, 5) and L[39] == ("tn", 160, 64, 1, 1024 * (rows // 32))      # the K = 160 stem and its weight gradient
        assert all(M % 32 == 0 for _, M, *_ in L)
        assert ("nt", rows, 64, 256, 0) in L                                                                # VC_P2's data gradient never splits
    seen = set()
    for name, (n, cfgs) in CASES.items():
        for cfg in cfgs:
            must, never = TC.expected("encoder", -(-n // 32) * 32, cfg)
            assert must | never == set(TC.KERNELS) | {"fused", "reduce"}          # exact for this tape
            seen |= must
    assert seen == set(TC.KERNELS) | {"fused", "reduce"}, sorted((set(TC.KERNELS) | {"fused", "reduce"}) - seen)
    at = lambda rows, cfg: TC.expected("encoder", rows, cfg)[0]          # noqa: E731
    assert at(64, "t32") == {"nn_32", "nt_32", "tn_32", "fused"} == at(64, "deep") == at(64, "shallow")
    assert at(64, "t64") == {"nn_64", "nt_64", "tn_64", "fused"}
    assert at(64, "t128") == at(64, "t32") | {"tn_128"} and at(160, "t128") == at(64, "t128") | {"nn_128", "nt_128"}
    assert {"nn_32_ki2", "nt_32_ki2", "tn_32_ki2"} <= at(64, "ki2_32") and {"nn_64_ki2", "nt_64_ki2", "tn_64_ki2"} <= at(64, "ki2_64")
    assert at(64, "nosplit") == {"nn_32", "nt_32", "tn_32"} and at(64, "reduce") == {"nn_32", "nt_32", "tn_32", "reduce"}
    # small frame counts split K in the forward and data-gradient GEMMs of the 4x4 and 2x2 stages; workload frame counts do not
    opt = TC.options("t32")
    split = lambda rows: {(f, N) for f, M, N, nb, st in TC.known_launches("encoder", rows) if f != "tn" and TC.gemm_shape(M, N, nb, st, opt)[1] > 1}      # noqa: E731
    assert ("nn", 512) in split(64) and ("nt", 256) in split(64) and not split(512) and not split(1024)
    for n, cfg in WORKLOAD:
        assert "fused" in at(n, cfg) and "reduce" not in at(n, cfg)               # (the weight gradients still split)
    # fused_part_bytes: ks blocks of one tile per output tile; 0 beyond 65536 tiles or 2^31 bytes
    assert TC.fused_part_bytes(64, 512, 4, 32, 8) == 8 * 2 * 4 * 8 * 32 * 64 * 4
    assert TC.fused_part_bytes(160, 256, 8, 128, 8) == 2 * 2 * 8 * 8 * 128 * 128 * 4
    assert TC.fused_part_bytes(1024, 64, 4096, 32, 2) == 0 and TC.fused_part_bytes(1024, 64, 2048, 32, 2) == 65536 * 2 * 32 * 64 * 4
    assert TC.fused_part_bytes(1024, 64, 2048, 32, 4) == 0
