"""flops.py counts ALGORITHMIC products: the nine-product form of the k = 5 convs over four positions (csrc/tconv.hpp t4_shared) executes 9 matrix
instructions where the conv has 14 (tap, position) pairs, and bench.py's `frac` stays work done per second over the fp32 matrix peak."""
from latent_diffusion_planning_amd import flops
from latent_diffusion_planning_amd import weights as W


def test_four_position_k5_conv_counts_fourteen_products():
    assert flops._valid_taps_same(4, 5) == 14 and flops._valid_taps_same(2, 5) == 4
    # the pinned planner figure of tests/test_host_logic.py (rm_lift planner, pred_horizon 8) holds whatever form the kernels execute
    p = W.PlannerSpec(25, 25)
    edge = 2.0 * 2 * (512 * 512 + 256 * 256)      # (edge outputs of the transposed convs: see test_flop_model_matches_survey)
    assert abs(flops.planner_forward_flops(p, 8) + edge - 0.16349e9) < 2e4
