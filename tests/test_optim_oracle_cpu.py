"""tests/optim_oracle.py on the CPU: its float64 Adam is oracle.train.adam_apply, its float32 restatement lies under the floors the GPU
tests (tests/test_hip_optimizer.py) fall back to, and its generator keeps its promises for every state those tests use."""
from collections import OrderedDict

import numpy as np
import pytest

from oracle import train as OT
from tests import optim_oracle as O

F32, F64 = np.float32, np.float64


def test_adam_step64_is_the_oracles_adam_bit_for_bit():
    g = O._rng(1)
    shapes = OrderedDict(a=(3, 5), b=(7,), c=(2, 3, 4))
    tree = lambda scale: OrderedDict((k, (scale * g.standard_normal(s)).astype(F32)) for k, s in shapes.items())
    p, grads, mu = tree(1.0), tree(1e-3), tree(1e-4)
    nu = OrderedDict((k, np.square(v) * F32(3)) for k, v in tree(1e-3).items())
    lr = float(F32(1e-4))
    for count in (1, 10, 1234):
        state = dict(mu=OrderedDict((k, v.astype(F64)) for k, v in mu.items()), nu=OrderedDict((k, v.astype(F64)) for k, v in nu.items()), count=count - 1)
        new, st = OT.adam_apply(p, grads, state, lambda c: lr)
        for k in shapes:
            r = O.adam_step64(p[k], grads[k], mu[k], nu[k], lr, count)
            for got, ref in ((r["p"], new[k]), (r["mu"], st["mu"][k]), (r["nu"], st["nu"][k])):
                assert got.dtype == F64 and np.array_equal(got.view(np.uint64), ref.view(np.uint64)), (count, k)
            assert np.array_equal(r["p"], p[k].astype(F64) + r["du"])


def test_ulp32():
    x = np.array([0.0, 1.0, 1.5, 2.0, -3.0, 2.0 ** -126, 2.0 ** -130, 1e-4])
    ref = [0.0] + [float(np.spacing(F32(abs(v)))) for v in x[1:]]
    assert np.array_equal(O.ulp32(x), np.array(ref))


@pytest.mark.parametrize("count", O.COUNTS)
def test_the_float32_restatement_lies_under_the_floors(count):
    """3 * err32 against k * 2^-24: the restatement's own worst error is within three roundings' worth of every floor, so the GPU bound
    max(k * 2^-24, 3 * err32) stays of the order of the floor (a bound that err32 inflates would hide what the GPU tests look for: an
    error of 6.5e-6 in the update, 1.3e-5 in nu)."""
    st = O.reachable_state(O.POOL, count, O.STATE_SEED[count])
    for lr in O.LRS:
        for p in (st["p"], np.zeros(O.POOL, F32)):
            lr32 = float(F32(lr))
            ref = O.adam_step64(p, st["g"], st["mu"], st["nu"], lr32, count)
            r32 = O.adam_step32(p, st["g"], st["mu"], st["nu"], lr32, count)
            err = O.step_errors(r32, ref, dict(st, p=p))
            for q, (worst, bad) in err.items():
                assert bad == 0, (q, bad)
                assert worst <= O.K_OPS[q] * O.U24, (count, lr, q, worst)
            if lr == 0:
                assert np.array_equal(r32["p"].view(np.uint32), np.asarray(p, F32).view(np.uint32))
            for d in (0.0, 0.99, 0.999, 0.9999, 1.0):
                for e_old in (np.zeros(O.POOL, F32), (np.asarray(p, F64) * 1.001).astype(F32)):
                    worst, bad = O.ema_error(O.ema32(e_old, r32["p"], d), e_old, r32["p"], d)
                    assert bad == 0 and worst <= O.K_OPS["ema"] * O.U24, (count, lr, d, worst)


@pytest.mark.parametrize("count", sorted(O.STATE_SEED))
def test_the_generator_keeps_its_promises(count):
    st = O.reachable_state(O.POOL, count, O.STATE_SEED[count])          # (asserts in the generator)
    assert st["steps"] == min(count - 1, 3000)
    O.check_state(st, st["stream"], st["steps"], count)
    scale = st["stream"].scale
    assert 1e-10 <= scale.min() < 1e-9 and 1e1 < scale.max() <= 1e2      # twelve decades, both ends present
    for k in ("p", "mu", "nu", "g"):
        assert not st[k].flags.writeable
    again = O.reachable_state.__wrapped__(O.POOL, count, O.STATE_SEED[count])
    assert all(np.array_equal(again[k], st[k]) for k in ("p", "mu", "nu", "g"))      # seeded: the GPU box builds the same state


def test_the_trajectory_stream_and_restatement():
    tr = O.trajectory()
    s = tr["stream"]
    for t in (0, 1, O.TRAJ_STEPS // 2 - 1, O.TRAJ_STEPS // 2, O.TRAJ_STEPS - 1):
        g = s(t)                                           # (asserts: no subnormal square)
        assert not g[s.never].any() and bool(g[s.zeroed].any()) == (t < O.TRAJ_STEPS // 2)
    r64, r32 = tr["r64"], tr["r32"]
    moved = np.abs(r64["p"] - tr["p0"])
    live = np.ones(O.POOL, bool)
    live[s.never] = False
    assert moved[live].min() > 0 and moved.max() <= 1.01 * O.TRAJ_STEPS * O.TRAJ_LR * 4.0
    err = np.abs(r32["p"].astype(F64) - r64["p"])
    assert err.mean() <= 1e-3 * moved.mean()               # float32 Adam follows float64 Adam to a thousandth of the distance moved
    worst, bad = O._rel(np.abs(r32["nu"].astype(F64) - r64["nu"]), r64["nu"])
    assert bad == 0 and worst <= 1e-5                      # 300 steps of four roundings each, never worse than their sum


def test_grad_norm_restatements():
    g = O.GradStream(O.POOL, 300, zero_from=0)(3)
    g = np.concatenate([g, g[:333]])                       # not a multiple of 1024
    n64, n32 = O.grad_norm64(g), O.grad_norm32_striped(g)
    assert abs(n32 - n64) <= 1e-6 * n64
    ones = np.ones(5000, F32)
    assert O.grad_norm32_striped(ones) == float(F32(np.sqrt(5000.0))) and O.grad_norm64(ones) == np.sqrt(5000.0)


def test_pool_index_uses_every_state():
    idx = O.pool_index(OrderedDict(a=40000, b=7, c=30000), O.POOL, 3)
    assert [v.size for v in idx.values()] == [40000, 7, 30000]
    assert np.array_equal(np.unique(np.concatenate(list(idx.values()))), np.arange(O.POOL))
