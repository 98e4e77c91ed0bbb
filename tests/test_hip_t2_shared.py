"""The three-product form of the exact-fp32 k = 5 convs over two positions (csrc/tconv.hpp t2_shared, csrc/t2pack.hpp) against float64.  -m gpu.

    S = W2 (x0 + x1),   out0 = S + (W3 - W2) x1,   out1 = S + (W1 - W2) x0

Tolerances are the project's own for the same quantities (tests/test_hip_planner.py): 1e-5 conv + GroupNorm + Mish, 2e-5 with FiLM, 2e-5 one U-Net
evaluation, 1e-4 a sampling loop."""
import numpy as np
import pytest
import torch

from latent_diffusion_planning_amd import weights as W
from oracle import np64, torch32
from tests.util import assert_close, planner_params, rng

pytestmark = pytest.mark.gpu

D = 25


@pytest.fixture(scope="module")
def eng():
    from latent_diffusion_planning_amd.engine import HipEngine
    e = HipEngine(obs_dim=D, action_dim=7, global_cond_dim=D, pred_horizon=8, action_horizon=4)
    e.load_params(planner=planner_params())
    yield e
    e.close()


# ---- the primitive ------------------------------------------------------------------------------------------------------------------------
INPUTS = ("independent", "equal", "negated", "scaled")      # x1 vs x0; "negated": the sum fragment is exactly zero
KERNELS = ("random", "taps_equal", "tap2_zero")             # "taps_equal": taps 1, 2, 3 equal, both differences exactly zero


@pytest.mark.parametrize("cin,cout", [(512, 512), (1024, 1024), (512, 1024), (2048, 512)])
def test_primitive_at_two_positions(cin, cout):
    """conv + GroupNorm + Mish (+ FiLM) at T = 2, every (input, kernel) pair: a wrong tap-to-accumulator map, a wrong sign or a swapped
    difference shows in at least one of them.  19 samples: two row blocks, the second ragged.

    Measured on MI355X (printed on every run): all 96 comparisons inside their bounds, largest 6.0e-6 of 1e-5 (2048 -> 512) and 1.00e-5 of 2e-5
    with FiLM (2048 -> 512, x1 = 1e4 x0).  The primitive runs the 1024-column shapes on the whole-group tile <2,8,1,4>, one K slice per
    work-group; that tile keeps a second accumulator set for the odd sub-chunks (tconv.hpp T2S2).  Without it each accumulator was one
    chain over the whole K range and 1024 -> 1024 with x1 = 1e4 x0 -- where the W2 terms of S and of (W3 - W2) x1 cancel in out0 and three
    chains' round-off stands where the direct form has one -- read 1.09e-5 against the 1e-5 bound; with it 3.8e-6 (largest of the shape
    4.8e-6 / 7.5e-6).  The four-product build (`make t2direct`), which has no such second set, misses three comparisons of that shape on
    these cases: 1.09e-5 and 2.22e-5 with FiLM (x1 = x0, equal taps), 2.52e-5 with FiLM (x1 = -x0, random)."""
    from latent_diffusion_planning_amd.engine import conv1d_gn_mish_film
    B = 19
    g = rng(2000 + cin + cout)
    x0 = g.standard_normal((B, cin))
    xs = {"independent": np.stack([x0, g.standard_normal((B, cin))], 1), "equal": np.stack([x0, x0], 1),
          "negated": np.stack([x0, -x0], 1), "scaled": np.stack([x0, 1e4 * x0], 1)}
    k = g.standard_normal((5, cin, cout)) / np.sqrt(5 * cin)
    k_eq = k.copy(); k_eq[1] = k_eq[2]; k_eq[3] = k_eq[2]
    k_z = k.copy(); k_z[2] = 0.0
    ks = {"random": k, "taps_equal": k_eq, "tap2_zero": k_z}
    bias, gs, gb = 0.1 * g.standard_normal(cout), 1 + 0.1 * g.standard_normal(cout), 0.1 * g.standard_normal(cout)
    film = g.standard_normal((B, 2 * cout))
    film_t = torch.tensor(film, dtype=torch.float32, device="cuda")
    misses = []
    for kn in KERNELS:
        # the float64 truth is taken from the weights the kernel is handed: fp32 values
        p = {"c/Conv_0/kernel": ks[kn].astype(np.float32), "c/Conv_0/bias": bias.astype(np.float32),
             "c/GroupNorm_0/scale": gs.astype(np.float32), "c/GroupNorm_0/bias": gb.astype(np.float32)}
        for xn in INPUTS:
            x = xs[xn].astype(np.float32)
            ref = np64.conv1d_block(x, p, "c", 8, 5)
            ref_f = film_t.cpu().numpy().astype(np.float64)[:, None, :cout] * ref + film_t.cpu().numpy().astype(np.float64)[:, None, cout:]
            xt = torch.tensor(x, device="cuda")
            got = conv1d_gn_mish_film(xt, p["c/Conv_0/kernel"], p["c/Conv_0/bias"], p["c/GroupNorm_0/scale"], p["c/GroupNorm_0/bias"]).cpu().numpy()
            got_f = conv1d_gn_mish_film(xt, p["c/Conv_0/kernel"], p["c/Conv_0/bias"], p["c/GroupNorm_0/scale"], p["c/GroupNorm_0/bias"], film_t).cpu().numpy()
            print(f"{cin}->{cout} x={xn} w={kn}: max|err| {np.abs(got - ref).max():.2e}, with FiLM {np.abs(got_f - ref_f).max():.2e}")
            for g_, r_, tol, what in ((got, ref, 1e-5, "conv+GN+Mish"), (got_f, ref_f, 2e-5, "conv+GN+Mish+FiLM")):
                try:                                   # every pair is measured and printed before the test fails on any of them
                    assert_close(g_, r_, tol, f"{what} T=2 {cin}->{cout} x={xn} w={kn}")
                except AssertionError as e:
                    misses.append(str(e))
    assert not misses, f"{len(misses)} of {2 * len(KERNELS) * len(INPUTS)} comparisons off: " + "; ".join(misses)


# ---- every launch shape of the form, through one U-Net evaluation -------------------------------------------------------------------------
POOL = 48      # distinct plans whose float64 truth is computed once; a batch takes rows (7 i + 3) mod 48: any 16 consecutive rows differ


@pytest.fixture(scope="module")
def pool():
    g = rng(4242)
    x, cond = g.standard_normal((POOL, 8, D)).astype(np.float32), g.uniform(-1, 1, (POOL, D)).astype(np.float32)
    P = torch32.TorchParams(planner_params(), dtype=torch.float64)
    ref = torch32.unet_forward(P, torch.tensor(x, dtype=torch.float64), 17, torch.tensor(cond, dtype=torch.float64)).numpy()
    return x, cond, ref


def test_every_launch_shape_matches_float64_and_is_counted(eng, pool):
    """5 plans: K split over work-groups; 64: quarter groups; 200: half groups; 300: whole groups; 1043: two row blocks per work-group.
    Twelve of an evaluation's 30 launches are k = 5 convs over two positions at pred_horizon 8; at pred_horizon 16 the same layers run at
    four positions on the five-tap packing and the counter must not move."""
    from latent_diffusion_planning_amd.engine import HipEngine
    x, cond, ref = pool
    eng.set_option("planner_split", 0)
    eng.set_option("no_batch_split", 1)
    try:
        for B in (5, 64, 200, 300, 1043):
            rows = (7 * np.arange(B) + 3) % POOL
            n0 = eng.get_option("stat_t2_shared_launches")
            got = eng.unet_forward(torch.tensor(x[rows]), 17, torch.tensor(cond[rows])).cpu().numpy()
            n = eng.get_option("stat_t2_shared_launches") - n0
            print(f"B={B}: max|err| {np.abs(got - ref[rows]).max():.2e}, shared-form launches {n}")
            assert_close(got, ref[rows], 2e-5, f"unet forward B={B}")
            assert n == 12, (B, n)
        eng.check_fault()
    finally:
        eng.set_option("planner_split", 1)
        eng.set_option("no_batch_split", 0)
    with pytest.raises(Exception):
        eng.set_option("stat_t2_shared_launches", 0)            # read-only
    e16 = HipEngine(obs_dim=D, action_dim=7, global_cond_dim=D, pred_horizon=16, action_horizon=4)
    try:
        e16.load_params(planner=planner_params())
        e16.set_option("planner_split", 0)
        g = rng(4343)
        x16, c16 = g.standard_normal((64, 16, D)).astype(np.float32), g.uniform(-1, 1, (64, D)).astype(np.float32)
        n0 = e16.get_option("stat_t2_shared_launches")
        got = e16.unet_forward(torch.tensor(x16), 17, torch.tensor(c16)).cpu().numpy()
        assert e16.get_option("stat_t2_shared_launches") == n0
        P = torch32.TorchParams(planner_params(), dtype=torch.float64)
        ref16 = torch32.unet_forward(P, torch.tensor(x16[:8], dtype=torch.float64), 17, torch.tensor(c16[:8], dtype=torch.float64)).numpy()
        assert_close(got[:8], ref16, 2e-5, "unet forward pred_horizon 16")
        e16.check_fault()
    finally:
        e16.close()


# ---- the loop -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler,n_steps", [("ddpm", 100), ("ddim", 100), ("ddim", 50)])
def test_sampling_loops_match_the_goldens(eng, sampler, n_steps):
    """tests/test_hip_planner.py::test_plan_sample_matches_oracle, repeated here on purpose: this file is what a reader of the form runs."""
    from tests.cases import load_case
    inp, exp = load_case(f"planner_loop_{sampler}{n_steps}")
    cond, x0, nz, ref = inp["cond"], inp["x0"], inp["nz"], exp["plan"]
    for use_graph in (False, True):
        got = eng.plan_sample(torch.tensor(cond, dtype=torch.float32), x_init=torch.tensor(x0, dtype=torch.float32),
                              step_noise=torch.tensor(nz, dtype=torch.float32) if sampler == "ddpm" else None,
                              sampler=sampler, n_steps=n_steps, use_graph=use_graph)
        assert_close(got.cpu().numpy(), ref, 1e-4, f"{sampler}/{n_steps} graph={use_graph}")


# ---- publishing trained parameters re-packs ------------------------------------------------------------------------------------------------
def test_publish_repacks_the_two_position_layers():
    """One optimiser step on the planner, publish, one evaluation against the float64 forward of the published parameters (read back the way
    tests/test_hip_train.py does): the sampling path's packed differences are those of the NEW weights."""
    from latent_diffusion_planning_amd.engine import HipEngine
    e = HipEngine(obs_dim=D, action_dim=7, global_cond_dim=D, pred_horizon=8, action_horizon=4)
    try:
        e.load_params(planner=planner_params(D=D))
        g = rng(515)
        B = 4
        obs = g.uniform(-1, 1, (B, 9, D)).astype(np.float32)
        noise, t = g.standard_normal((B, 8, D)).astype(np.float32), g.integers(0, 100, B)
        x, cond = torch.tensor(g.standard_normal((3, 8, D)), dtype=torch.float32), torch.tensor(g.uniform(-1, 1, (3, D)), dtype=torch.float32)
        before = e.unet_forward(x, 17, cond).clone()
        e.train_init(["planner"])
        e.train_planner_grad(torch.tensor(obs[:, 1:].copy()), torch.tensor(noise), t, torch.tensor(obs[:, 0].copy()))
        e.train_apply("planner", 1e-3)
        e.train_publish(["planner"])
        n0 = e.get_option("stat_t2_shared_launches")
        after = e.unet_forward(x, 17, cond)
        assert e.get_option("stat_t2_shared_launches") - n0 == 12
        assert not torch.equal(after, before)
        new = e.train_read("planner", e.TRAIN_PARAMS, W.planner_shapes(W.PlannerSpec(D, D)))
        ref = torch32.unet_forward(torch32.TorchParams(new, dtype=torch.float64), x.double(), 17, cond.double()).numpy()
        assert_close(after.cpu().numpy(), ref, 2e-5, "unet forward on the published parameters")
        e.check_fault()
    finally:
        e.close()
