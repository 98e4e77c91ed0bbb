"""The conv epilogue's exchanges (csrc/tconv.hpp: the GroupNorm statistics polls pipelined over a wave's samples, the K-partials polled per
sample row -- at most two elements at a time --, the projection's values held in registers and every store behind the last sample's
arithmetic) against float64.  -m gpu.

Two ways in, because the column split (cs) and the K split (kw) exist only in the engine's dispatch:

* `ldp_conv1d_gn_mish_film_f32` takes the tile `pick_plan` gives its shape and runs it over whole GroupNorm groups (it owns no exchange
  slab): it covers the batched epilogue's cs == 1 side -- phase A, the wave sums, the normalise-and-store loop over the wave's SPW samples,
  ragged last sample blocks -- at the shapes and batches below.  Bounds as in tests/test_hip_t2_shared.py: 1e-5 conv + GroupNorm + Mish,
  2e-5 with FiLM.
* `ldp_unet_trace` runs the planner's own dispatch: up to 128 plans quarter groups (cs == 4) with the K split (kw up to 8), 129 .. 256
  half groups (cs == 2), with FiLM (first halves), a residual input (second halves) and the 1x1 projection in the same launch
  (RES_OUT).  Every stage is held against float64 on its own tapped inputs inside the bound tests/planner_stage_cases.py computes for it,
  and the table must show that the exchanges really ran.

check_fault() is clean after every case: no exchange timed out.  No case provokes a time-out."""
import numpy as np
import pytest
import torch

from oracle import np64
from tests import planner_stage_cases as PC
from tests.test_hip_planner_stages import _check_case, _close_engines  # noqa: F401  (the fixture closes the engines _check_case opens)
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
# (T, Cin, Cout) -> the batches it runs at; the float64 truth is computed once per shape, at the largest batch (samples never couple)
HALF_BATCHES, QUARTER_BATCHES = (129, 144), (5, 16, 17, 128)          # 129: nine sample blocks, the last holding one sample
SHAPES = {(2, 128, 512): HALF_BATCHES, (2, 128, 1024): HALF_BATCHES, (4, 64, 256): HALF_BATCHES,
          (2, 1024, 1024): QUARTER_BATCHES, (4, 512, 512): QUARTER_BATCHES, (8, 256, 256): QUARTER_BATCHES}
_truth = {}


def _shape_truth(T, cin, cout):
    key = (T, cin, cout)
    if key not in _truth:
        B = max(SHAPES[key])
        g = rng(7000 + 100 * T + cin + cout)
        x = g.standard_normal((B, T, cin)).astype(np.float32)
        p = {"c/Conv_0/kernel": (g.standard_normal((5, cin, cout)) / np.sqrt(5 * cin)).astype(np.float32),
             "c/Conv_0/bias": (0.1 * g.standard_normal(cout)).astype(np.float32),
             "c/GroupNorm_0/scale": (1 + 0.1 * g.standard_normal(cout)).astype(np.float32),
             "c/GroupNorm_0/bias": (0.1 * g.standard_normal(cout)).astype(np.float32)}
        film = g.standard_normal((B, 2 * cout)).astype(np.float32)
        ref = np64.conv1d_block(x, p, "c", 8, 5)                      # the truth of the fp32 values the kernel is handed
        ref_f = film.astype(np.float64)[:, None, :cout] * ref + film.astype(np.float64)[:, None, cout:]
        for a in (x, film, ref, ref_f):
            a.setflags(write=False)
        _truth[key] = (x, p, film, ref, ref_f)
    return _truth[key]


@pytest.mark.parametrize("T,cin,cout,B", [(*s, B) for s in sorted(SHAPES) for B in SHAPES[s]])
def test_primitive(eng, T, cin, cout, B):
    from latent_diffusion_planning_amd.engine import conv1d_gn_mish_film
    x, p, film, ref, ref_f = _shape_truth(T, cin, cout)
    xt, ft = torch.tensor(x[:B], device="cuda"), torch.tensor(film[:B], device="cuda")
    args = (p["c/Conv_0/kernel"], p["c/Conv_0/bias"], p["c/GroupNorm_0/scale"], p["c/GroupNorm_0/bias"])
    got = conv1d_gn_mish_film(xt, *args).cpu().numpy()
    got_f = conv1d_gn_mish_film(xt, *args, ft).cpu().numpy()
    print(f"T={T} {cin}->{cout} B={B}: max|err| {np.abs(got - ref[:B]).max():.2e}, with FiLM {np.abs(got_f - ref_f[:B]).max():.2e}")
    assert_close(got, ref[:B], 1e-5, f"conv+GN+Mish T={T} {cin}->{cout} B={B}")
    assert_close(got_f, ref_f[:B], 2e-5, f"conv+GN+Mish+FiLM T={T} {cin}->{cout} B={B}")
    eng.check_fault()                                                 # the fault block is the process's: nothing timed out anywhere


# ---- one U-Net evaluation on the planner's own dispatch ------------------------------------------------------------------------------------
def _gn(r):
    return r["kind"] in ("res1", "res2", "final")


@pytest.mark.parametrize("B", [129, 130, 144, 256])
def test_unet_stages_on_half_groups(B):
    """129 .. 256 plans: the statistics exchange between the two halves of a group (cs == 2), alone -- no K split.  B = 129: nine sample
    blocks, the last holding one sample; the other waves of that block still exchange for rows nobody stores."""
    rows = _check_case(PC.case("t8", B))
    conv = [r for r in rows if r["plan"][0] >= 0]
    half = [r for r in conv if r["cs"] == 2]
    assert all(r["kw"] == 1 for r in conv), "a K split above 128 plans"
    assert len(half) >= 20, f"{len(half)} launches on half groups"
    # FiLM (first halves), a residual input (second halves), the projection in the same launch, at two and at four positions
    for T in (2, 4):
        for kind, res in (("res1", 0), ("res1", 1), ("res2", 0)):
            assert any(r["kind"] == kind and r["plan"][5] == res and r["t"].shape[1] == T for r in half), (T, kind, res)
    assert any(r["t"].shape[1] == 2 and r["t"].shape[2] == 1024 for r in half) and any(r["t"].shape[1] == 4 and r["t"].shape[2] == 512 for r in half)


@pytest.mark.parametrize("B", [5, 16, 17, 128])
def test_unet_stages_on_quarter_groups_with_the_k_split(B):
    """Up to 128 plans: quarter groups (cs == 4: three peers per record batch) and the K split over work-groups, with and without the
    projection.  16 / 17: one full sample block / a second one holding one sample."""
    rows = _check_case(PC.case("t8", B))
    conv = [r for r in rows if r["plan"][0] >= 0]
    assert any(r["cs"] == 4 for r in conv), "no launch on quarter groups"
    kws = [r for r in conv if r["kw"] > 1]
    assert kws, "no launch with the K split"
    if B <= 17:
        assert max(r["kw"] for r in kws) == 8, sorted({r["kw"] for r in kws})
        for T in (2, 4, 8):
            assert any(r["t"].shape[1] == T and r["plan"][0] == PC.K5 for r in kws), f"no K-split k = 5 conv at {T} positions"
        assert any(r["plan"][5] == 1 for r in kws) and any(r["plan"][5] == 0 for r in kws), "K split with and without the projection"
        assert any(r["cs"] > 1 for r in kws), "K split and column split in one launch"


# ---- the loop: graph replay == eager -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [16, 144])
def test_graph_replay_equals_eager(eng, B):
    g = rng(8100 + B)
    cond = torch.tensor(g.uniform(-1, 1, (B, D)), dtype=torch.float32)
    x0 = torch.tensor(g.standard_normal((B, 8, D)), dtype=torch.float32)
    a = eng.plan_sample(cond, x_init=x0, sampler="ddim", n_steps=10, use_graph=False)
    b = eng.plan_sample(cond, x_init=x0, sampler="ddim", n_steps=10, use_graph=True)
    c = eng.plan_sample(cond, x_init=x0, sampler="ddim", n_steps=10, use_graph=True)          # replay of the cached graph
    eng.check_fault()
    assert torch.isfinite(a).all()
    assert torch.equal(a, b) and torch.equal(b, c)
