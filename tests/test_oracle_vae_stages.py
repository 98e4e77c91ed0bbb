"""The stage lists of oracle/torch32.py (what tests/test_hip_vae_stages.py holds every stage of the engine against) chained end to end ARE
vae_encode_mean / vae_decode, bit for bit in float64, and have the stage kinds the engine's trace table reports (CPU)."""
import numpy as np
import pytest
import torch

from latent_diffusion_planning_amd import weights as W
from oracle import torch32
from tests.util import rng

# per level 2 (encoder) / 3 (decoder) ResnetBlock2D of two stages each, a third where the width changes (128 -> 256: down_blocks_1/resnets_0,
# up_blocks_5/resnets_0); five Downsample2D / upsamplers; mid block = block, attention, block
ENC_KINDS = (["conv_in"] + ["res1", "res2"] * 2 + ["down"] + ["res1", "shortcut", "res2", "res1", "res2", "down"]
             + ["res1", "res2", "res1", "res2", "down"] * 3 + ["res1", "res2"] * 2
             + ["res1", "res2", "attn", "res1", "res2"] + ["conv_out", "quant"])
DEC_KINDS = (["post_quant", "conv_in"] + ["res1", "res2", "attn", "res1", "res2"] + (["res1", "res2"] * 3 + ["up"]) * 5
             + ["res1", "shortcut", "res2"] + ["res1", "res2"] * 2 + ["conv_out", "nchw"])


@pytest.mark.parametrize("S,LC", [(64, 4), (96, 4), (128, 4), (64, 8)])
def test_chained_stages_are_the_oracle(S, LC):
    vp = W.init_vae_params(W.VAESpec(latent_channels=LC), seed=2)
    P = torch32.TorchParams(vp, dtype=torch.float64)
    g = rng(S * 10 + LC)
    img = torch.tensor(g.uniform(-1, 1, (1, S, S, 3)))
    enc = torch32.vae_encode_stages(P)
    assert [k for k, *_ in enc] == ENC_KINDS
    outs = torch32.run_stages(P, enc, img.permute(0, 3, 1, 2))
    assert outs[-1].shape == (1, 2 * LC, S // 32, S // 32)
    assert torch.equal(outs[-1][:, :LC].permute(0, 2, 3, 1), torch32.vae_encode_mean(P, img, latent_channels=LC))
    z = torch.tensor(g.uniform(-3, 3, (1, S // 32, S // 32, LC)))
    dec = torch32.vae_decode_stages(P)
    assert [k for k, *_ in dec] == DEC_KINDS
    outs = torch32.run_stages(P, dec, z.permute(0, 3, 1, 2))
    assert outs[-1].shape == (1, 3, S, S)
    assert torch.equal(outs[-1], torch32.vae_decode(P, z))
    # every stage reads stages before it, and every stage but the last is read
    for st in (enc, dec):
        read = set()
        for k, (_, _, inputs, _) in enumerate(st):
            assert all(-1 <= i < k for i in inputs)
            read.update(inputs)
        assert read == set(range(-1, len(st) - 1))


def test_stages_run_in_float32_too():
    vp = W.init_vae_params(seed=2)
    P32, P64 = torch32.TorchParams(vp, dtype=torch.float32), torch32.TorchParams(vp, dtype=torch.float64)
    z = torch.tensor(rng(3).uniform(-3, 3, (1, 4, 2, 2)))
    st = torch32.vae_decode_stages(P32)[:7]
    o32, o64 = torch32.run_stages(P32, st, z), torch32.run_stages(P64, st, z)
    assert o32[-1].dtype == torch.float32 and o64[-1].dtype == torch.float64
    assert float((o32[-1].double() - o64[-1]).abs().max()) < 1e-4 * max(1.0, float(o64[-1].abs().max()))
