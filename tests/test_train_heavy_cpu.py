"""The premises tests/test_hip_train_heavy.py rests on, checked without a GPU (fixtures: tests/train_heavy_cases.py).

  * the trained-like cases reach the tails no init-like case reaches: Mish inputs above 20 (the clamp of mish_x / mish_dx and the `x > 20`
    branch), below -20 and below -88 (expf underflows); IDM ReLU inputs in the thousands and half the hidden units dead.  RECORDED holds
    the census of the float64 forward as measured when the cases were built; a case must keep at least a tenth of each count.
  * the init-like sets every earlier test of the tape loads reach none of it: no Mish input beyond +-8 -- the gap this file's GPU twin closes.
  * the rule's floor stays a floor: err32_leaf <= 1e-4 max|ref64 leaf| on every leaf of every case, so no bound exceeds 3e-4 of the leaf.
  * grads32 run in float64 IS oracle.train.loss_and_grads (1e-12 of each leaf's largest entry): the restated norms change nothing but round-off.
  * the IDM rows: the per-unit gate rule keeps rows 16 round-offs clear of every gate, where the one global figure of train_cases.idm_rows
    cannot; the rows no rule keeps have at most 4 ambiguous gates, and float32 itself meets one assignment of them.
"""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import train_cases as TC
from tests import train_heavy_cases as H

#            case -> Mish inputs (above 20, below -20, below -88) of the float64 forward, as built
RECORDED = dict(ph3=(1182, 1278, 80), ph33=(12910, 13902, 860), ph129=(50855, 54523, 3403), pw3=(1199, 1204, 83), pw33=(13080, 13232, 992),
                pw129=(51387, 51994, 3951), p16h3=(2336, 2407, 157), hh3=(399, 399, 27), hh40=(5298, 5471, 265), dh3=(2624, 2528, 158),
                dh33=(28670, 28189, 1899))


@pytest.mark.parametrize("name", list(H.CASES))
def test_case_reaches_the_tails_and_float32_stays_a_floor(name):
    r = H.reference(name)
    worst, leaf = H.worst_err32_over_leafmax(r)
    print("heavy case", json.dumps(dict(case=name, err32_over_leafmax=worst, leaf=leaf, loss=r["loss"], loss32_err=abs(r["loss32"] - r["loss"]),
                                        census=r.get("census"), rows=r["rows_info"])))
    assert worst <= 1e-4, f"{name}: err32 of {leaf} is {worst:.3g} of the leaf's maximum: change the case (seed, size), not the factor"
    assert all(np.isfinite(g).all() for g in r["grads"].values()) and np.isfinite(r["loss"])
    assert abs(r["loss32"] - r["loss"]) <= 1e-5 * max(1.0, abs(r["loss"]))
    if name in RECORDED:
        c = r["census"]
        for got, rec in zip((c["above20"], c["below20"], c["below88"]), RECORDED[name]):
            assert got >= rec / 10 and rec > 0, (name, c, RECORDED[name])
    elif r["model"] == "idm":
        info = r["rows_info"]
        assert info["max_abs"] >= 1000 and info["dead"] >= 1000, info
        assert info["kept_min"] >= TC.MARGIN_OVER_ROUNDOFF and info["gates_differ"] == 0, info
    else:
        assert name == "pc3" and max(c for c in (r["census"]["above20"], r["census"]["below20"])) == 0


@pytest.mark.parametrize("name", list(H.INIT_LIKE))
def test_init_like_parameters_reach_no_tail(name):
    c = H.init_like_census(name)
    print("init-like census", json.dumps(dict(case=name, **c)))
    assert c["n"] == H.reference(name)["census"]["n"] and c["max"] <= 8.0 and c["min"] >= -8.0, c


def test_the_constant_group_has_statistics_8_and_0_exactly():
    """In float64 and in float32 alike: every addend of both sums is exact, so var = 64 - 8 * 8 = 0 and rstd = 1 / sqrt(eps)."""
    c = H.inputs_of("pc3")[0]
    for dtype in (torch.float64, torch.float32):
        f = H.grads32("planner", H.params_of("planner_const"), c, 1.3, dtype)["f"]
        mean, var = f.gn_stats[H.CONST_GN_CALL]
        assert mean.shape == (3, 8) and torch.equal(mean[:, 0], torch.full((3,), H.CONST_VALUE, dtype=dtype)) and torch.equal(var[:, 0], torch.zeros(3, dtype=dtype))
        assert float(var[:, 1:].min()) > 1e-3                        # (no other group is anywhere near)


@pytest.mark.parametrize("name", ["ph3", "p16h3", "ih24", "hh3", "dh3"])
def test_grads32_in_float64_is_the_oracle(name):
    r = H.reference(name)
    got = H.grads32(r["model"], H.params_of(r["params"]), r["inputs"], r["alpha"], torch.float64)
    assert abs(got["loss"] - r["loss"]) <= 1e-12 * abs(r["loss"])
    worst = 0.0
    for k, g in r["grads"].items():
        assert got["grads"][k].shape == g.shape
        worst = max(worst, float(np.abs(got["grads"][k] - g).max()) / float(np.abs(g).max()))
    if "dcond" in r:
        worst = max(worst, float(np.abs(got["dcond"] - r["dcond"]).max()) / float(np.abs(r["dcond"]).max()))
    print(f"{name}: grads32 in float64 against the oracle: {worst:.2e} of the leaf's maximum")
    assert worst <= 1e-12


def test_the_restated_norms_are_flax_fast_variance():
    """Equal to torch's centred form in float64; in float32 at a mean 1e4 times the spread they lose the variance where torch's keeps it --
    the cost err32 must carry, since csrc/train.hip computes the statistics the same way."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5, 16, 12, generator=g, dtype=torch.float64)
    w, b = torch.randn(16, generator=g, dtype=torch.float64), torch.randn(16, generator=g, dtype=torch.float64)
    f = H.FlaxF()
    assert float((f.group_norm(x, 4, w, b, 1e-6) - F.group_norm(x, 4, w, b, eps=1e-6)).abs().max()) <= 1e-13
    row, wr, br = x.reshape(5, -1), torch.ones(192, dtype=torch.float64), torch.zeros(192, dtype=torch.float64)
    assert float((f.layer_norm(row, (192,), wr, br, 1e-6) - F.layer_norm(row, (192,), wr, br, eps=1e-6)).abs().max()) <= 1e-13
    far = (row + 1e4).float()
    lost = (f.layer_norm(far, (192,), wr.float(), br.float(), 1e-6).double() - F.layer_norm(row, (192,), wr, br, eps=1e-6)).abs().max()
    kept = (F.layer_norm(far, (192,), wr.float(), br.float(), eps=1e-6).double() - F.layer_norm(row, (192,), wr, br, eps=1e-6)).abs().max()
    assert float(lost) > 100 * float(kept), (float(lost), float(kept))


def test_relu_takes_listed_gates_as_given():
    f = H.FlaxF(gates={1: True, 5: False})
    x = torch.tensor([[0.5, -0.25, -1.0]], dtype=torch.float64, requires_grad=True)
    y = torch.tensor([[2.0, -3.0, 4.0]], dtype=torch.float64, requires_grad=True)
    (f.relu(x).sum() + f.relu(y).sum()).backward()
    assert x.grad.tolist() == [[1.0, 1.0, 0.0]] and y.grad.tolist() == [[1.0, 0.0, 0.0]]


def test_every_entry_floor_only_ever_raises_the_bound():
    ref, got = dict(a=np.array([1.0, -2.0])), dict(a=np.array([1.0003, -2.0]))
    assert TC.every_entry(got, ref, 1e-4)[1] and TC.every_entry(got, ref, 1e-4, floor=dict(a=1e-5))[1]
    worst, bad = TC.every_entry(got, ref, 1e-4, floor=dict(a=4e-4))
    assert not bad and abs(worst["err_over_bound"] - 0.75) < 1e-6


def test_one_global_roundoff_rejects_trained_like_rows_for_the_wrong_reason():
    """train_cases.idm_rows on the trained-like set: the pool's largest round-off belongs to the x 100 units, and no row clears it 16 times;
    per unit (the premise of cases ih24 / ih320, asserted above) all but a few rows do."""
    for rows, seed in ((24, 2024), (320, 2320)):
        _, info = TC.idm_rows(H.params_of("idm_heavy"), rows, seed)
        assert info["ratio"] < TC.MARGIN_OVER_ROUNDOFF, info
        _, per_unit = H.idm_rows_per_unit(H.params_of("idm_heavy"), rows, seed)
        assert per_unit["pool_clear"] >= rows, per_unit


@pytest.mark.parametrize("pset", ["idm", "idm_heavy"])
def test_rows_no_rule_keeps_have_few_ambiguous_gates_and_float32_meets_one_assignment(pset):
    rows = H.gate_rows(pset)
    assert len(rows) == H.GATE_ROWS
    for row in rows:
        assert len(row["gates"]) <= H.MAX_GATES and len(row["refs"]) == 2 ** len(row["gates"]), row["gates"]
        met, ratios = H.assignment_met(row["run32"]["grads"], row["run32"]["loss"], row)
        cap = max(v / float(np.abs(ref["grads"][k]).max()) for ref in row["refs"] for k, v in ref["err32"].items())
        print("gate row", json.dumps(dict(params=pset, row=row["row"], margin=row["margin"], gates=row["gates"], float32_met=met, ratios=ratios,
                                          err32_over_leafmax=cap)))
        assert met is not None, (row["row"], row["gates"], ratios)
        assert cap <= 1e-4, (row["row"], cap)
