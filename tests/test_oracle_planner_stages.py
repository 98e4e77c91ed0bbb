"""The stage list of oracle/torch32.py (what tests/test_hip_planner_stages.py holds every launch of the planner U-Net against) chained end to
end IS unet_forward, bit for bit in float64 and in float32, and has the stage kinds the engine's trace table reports (CPU)."""
import pytest
import torch

from latent_diffusion_planning_amd import weights as W
from oracle import torch32
from tests.util import rng

HIER_IDM_DOWN = (256, 512)


def kinds(n_levels):
    """Per level two residual blocks (the first with the projection: res1, proj, res2), a stride-2 conv between levels; two middle blocks;
    per up level the two blocks and a transposed conv; the Conv1dBlock and the 1x1 head."""
    blk, blkp = ["res1", "res2"], ["res1", "proj", "res2"]
    k = ["input", "film"]
    for lvl in range(n_levels):
        k += blkp + blk + (["down"] if lvl < n_levels - 1 else [])
    k += blk + blk
    for lvl in range(n_levels - 1):
        k += blkp + blk + ["up"]
    return k + ["fin_block", "head"]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("T,D,G,dims", [(8, 25, 25, (256, 512, 1024)), (16, 25, 25, (256, 512, 1024)), (4, 7, 50, HIER_IDM_DOWN)],
                         ids=["T8", "T16", "hier_idm"])
def test_chained_stages_are_the_oracle(T, D, G, dims, dtype):
    pp = W.init_planner_params(W.PlannerSpec(D, G, down_dims=dims), 0)
    P = torch32.TorchParams(pp, dtype=dtype)
    g = rng(100 * T + D)
    B = 3
    x = torch.tensor(g.standard_normal((B, T, D)), dtype=dtype)
    cond = torch.tensor(g.uniform(-1, 1, (B, G)), dtype=dtype)
    k = torch.tensor([0, 99, 41])
    st = torch32.unet_stages(P, down_dims=dims)
    assert [s[0] for s in st] == kinds(len(dims))
    outs = torch32.run_unet_stages(P, st, x, k, cond)
    ref = torch32.unet_forward(P, x, k, cond, down_dims=dims)
    assert outs[-1].dtype == dtype and outs[-1].shape == (B, D, T)
    assert torch.equal(outs[-1].transpose(1, 2), ref)
    # every stage reads stages before it (or the call's inputs), and every stage but the last is read
    read = set()
    for i, (_, _, inputs, _) in enumerate(st):
        assert all(-3 <= j < i for j in inputs)
        read.update(inputs)
    assert read == set(range(-3, len(st) - 1))
    # the FiLM stage is the sum of the two parts the engine keeps apart, to round-off
    n_blocks = sum(1 for s in st if s[0] == "res1")
    ft, fg = torch32.unet_film_parts(P, k, cond, n_blocks)
    film = outs[1]
    assert film.shape == ft.shape == fg.shape == (B, sum(2 * o.shape[1] for s, o in zip(st, outs) if s[0] == "res1"))
    tol = 1e-12 if dtype == torch.float64 else 2e-5
    assert float((ft + fg - film).abs().max()) <= tol * max(1.0, float(film.abs().max()))
