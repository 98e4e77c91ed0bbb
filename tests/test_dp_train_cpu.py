"""DPTrainAgent without a GPU: the differentiable restatement of the encoder and of the DP loss (tests/dp_train_oracle.py) against
tests/dp_resnet_oracle.py, the conditions the committed goldens rest on, and the host logic of `update` on a recording stub engine."""
import os

import numpy as np
import pytest
import torch

from latent_diffusion_planning_amd import weights as W
from tests import dp_resnet_oracle as RO
from tests import dp_train_oracle as TO
from tests.golden.make_golden_dp_resnet import TIE_TOL
from tests.golden.make_golden_dp_train import AH, CASES, LOSS_TOL, MAX_BYTES, OH, T, conditions, golden_path
from tests.train_stub import TrainStub
from tests.util import rng


def _golden(name):
    cfg, shared, _, _ = CASES[name]
    z = np.load(golden_path(name))
    data = RO.BY_NAME[cfg]
    p = RO.planner_params(data, int(z["seed_params"]), OH)
    enc = RO.encoder_params(data, int(z["seed_encoder"]), shared)
    obs = {k[len("in_obs__"):]: z[k] for k in z.files if k.startswith("in_obs__")}
    return z, data, shared, p, enc, {"obs": obs, "actions": z["in_actions"]}


# ---- the restatement and the goldens ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_the_oracle_on_the_goldens_inputs(name):
    z, data, shared, p, enc, batch = _golden(name)
    nobs = RO.normalized_obs(data, batch["obs"])
    for k, x in RO.encoder_inputs(data, nobs, OH, shared).items():
        feat = TO.encode_t(TO.leaves_of(enc[k]), torch.as_tensor(np.asarray(x), dtype=torch.float64)).detach().numpy()
        np.testing.assert_allclose(feat, RO.encode(enc[k], x), rtol=0, atol=1e-12)
    t, noise = z["in_t"].astype(np.int64), z["in_noise"]
    r = TO.loss_and_grads(data, p, enc, batch["obs"], batch["actions"], t, noise, OH, shared)
    ref = RO.loss(data, p, enc, batch["obs"], batch["actions"], t, noise, OH, shared)
    assert abs(r["loss"] - ref["loss"]) <= 1e-12 * ref["loss"]
    np.testing.assert_allclose(r["cond"], ref["cond"], rtol=0, atol=1e-12)
    assert abs(r["loss"] - float(z["out_loss"])) <= 1e-12 * r["loss"]
    np.testing.assert_allclose(r["dcond"], z["out_dcond"], rtol=0, atol=1e-6 * np.abs(r["dcond"]).max())      # (stored in float32)


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_satisfies_the_generators_conditions(name):
    z, data, shared, p, enc, batch = _golden(name)
    t64, t32, gap, l64, l32 = conditions(data, p, enc, batch, z["in_t"].astype(np.int64), z["in_noise"], shared)
    assert t64 == 0 and t32 == 0, "a max-pool window's positive maximum is attained twice: the tie rule would be exercised"
    assert gap > TIE_TOL
    assert abs(l32 - l64) <= LOSS_TOL * l64
    assert abs(float(z["out_loss32"]) - float(z["out_loss"])) <= LOSS_TOL * float(z["out_loss"])
    assert os.path.getsize(golden_path(name)) < MAX_BYTES == 450 * 1024


def test_pool_ties_counts_only_positive_repeated_maxima():
    x = torch.zeros((1, 1, 4, 4), dtype=torch.float64)
    assert TO.pool_ties(x) == 0                             # ties at 0: the ReLU backward kills them
    x[0, 0, 0, 0] = x[0, 0, 1, 1] = 2.0
    assert TO.pool_ties(x) == 1                             # window (0, 0) holds both; no other window holds either twice
    x[0, 0, 1, 1] = 3.0
    assert TO.pool_ties(x) == 0


def test_tie_case_separates_the_first_maximum_rule_from_a_wrong_one():
    """The case tests/test_hip_resnet_train_shapes.py runs the GPU's max-pool backward on (TO.tie_case): most pool windows hold their positive
    maximum more than once, identically in float64 and float32; F.max_pool2d's gradient is that of "the first maximum in row-major order";
    and a kernel that took the last maximum, or split the gradient among the tied entries, would miss conv_init/kernel's gradient by at
    least 100 x the GPU rule's bound (1e-4 leafmax): a wrong rule cannot pass there."""
    from tests.golden.make_golden_dp_resnet import frames_to_input
    p, frames = TO.tie_case()
    x = frames_to_input(frames)
    d = rng(960 + 77).standard_normal((3, RO.FEAT)).astype(np.float32)
    ties, taps = [], {}
    for dt in (torch.float64, torch.float32):
        _, stem, _ = TO.encode_t(TO.leaves_of(p, dt), torch.as_tensor(x, dtype=dt), return_maps=True, taps=taps.setdefault(dt, []))
        ties.append(TO.pool_ties(stem))
    assert ties[0] == ties[1] >= 10000 and ties[0] <= 3 * 64 * 16 * 16, ties
    # and no ReLU input of the case lies where float32 round-off could gate it the other way (the pool's equal values are exactly equal)
    gate = min(float(a.abs().min()) for a in taps[torch.float64])
    roundoff = max(float((b.double() - a).abs().max()) for a, b in zip(taps[torch.float64], taps[torch.float32]))
    assert gate >= TO.GATE_MARGIN_OVER_ROUNDOFF * roundoff, (gate, roundoff)
    f64, g64, _ = TO.encoder_vjp(p, x, d)
    _, g32, _ = TO.encoder_vjp(p, x, d, torch.float32)
    key = "conv_init/kernel"
    leafmax = float(np.abs(g64[key]).max())
    err32 = float(np.abs(g32[key] - g64[key]).max())
    bound = max(1e-4 * leafmax, 3.0 * err32) + 1e-12              # the GPU rule on this leaf
    got = {}
    for rule in ("first", "last", "split"):
        f, g, _ = TO.encoder_vjp(p, x, d, pool=TO.pool_with_rule(rule))
        np.testing.assert_allclose(f, f64, rtol=0, atol=1e-12)     # the rules differ in the backward only
        got[rule] = g
    print(f"tie case: {ties[0]} of {3 * 64 * 16 * 16} windows tied; err32 {err32 / leafmax:.1e} leafmax; conv_init/kernel off by "
          f"{np.abs(got['last'][key] - g64[key]).max() / leafmax:.2f} (last) and {np.abs(got['split'][key] - g64[key]).max() / leafmax:.2f} (split) leafmax")
    assert bound == pytest.approx(1e-4 * leafmax, rel=1e-6), "float32's own error sets the bound: the margin below would not be the rule's"
    for k, ref in g64.items():
        assert np.abs(got["first"][k] - ref).max() <= 1e-12 * np.abs(ref).max(), k
    for rule in ("last", "split"):
        assert np.abs(got[rule][key] - g64[key]).max() >= 100.0 * bound, rule


def test_clear_frames_keep_every_gate_clear_of_float32_round_off():
    """What the batches of tests/test_hip_resnet_train_shapes.py rest on (same seeds): the kept frames' smallest |ReLU input| and pool gap is
    at least 3 x the largest |float32 - float64| of any ReLU input of the pool, exactly the frames with the largest margins are kept, a
    frame's margin does not depend on its batch -- and 129 frames as they come do hold a gate inside that round-off."""
    from tests.golden.make_golden_dp_resnet import frames_to_input
    from tests.test_hip_resnet_train import _params
    from tests.test_hip_resnet_train_shapes import DISTINCT, POOL, SEED
    p = _params("perturbed", SEED)
    frames, info = TO.clear_frames(p, DISTINCT, POOL, SEED)
    print(f"clear frames: {DISTINCT} of {POOL}, smallest kept margin {info['kept_min']:.2e}, round-off {info['roundoff']:.2e}, ratio {info['ratio']:.1f}")
    assert frames.shape == (DISTINCT, 64, 64, 3) and info["ratio"] >= TO.GATE_MARGIN_OVER_ROUNDOFF, info
    pool = RO.synth_frames(POOL, SEED)
    margin, roundoff = TO.gate_margins(p, frames_to_input(pool[:129]))
    print(f"129 frames as they come: smallest margin {margin.min():.2e}, round-off {roundoff:.2e}")
    assert margin.min() < roundoff
    kept, _ = TO.gate_margins(p, frames_to_input(frames))
    assert kept.min() == pytest.approx(info["kept_min"], rel=1e-6)                    # alone or in the pool: the same margin
    assert sum(1 for f in pool[:129] if any(np.array_equal(f, k) for k in frames)) == int((margin >= info["kept_min"] * (1 - 1e-6)).sum())


def test_encoder_vjp_is_linear_in_dfeat_and_matches_finite_differences():
    small = {k: np.asarray(v, np.float32) for k, v in W.init_resnet_params(RO.SPEC, seed=5, perturb=True).items()}
    x = (rng(6).uniform(-1, 1, (1, 64, 64, 3))).astype(np.float32)
    d = rng(7).standard_normal((1, RO.FEAT))
    _, g, _ = TO.encoder_vjp(small, x, d)
    key, idx, h = "norm_init/bias", 3, 1e-6
    up, dn = dict(small), dict(small)
    up[key] = small[key].astype(np.float64).copy(); up[key][idx] += h
    dn[key] = small[key].astype(np.float64).copy(); dn[key][idx] -= h
    fd = ((RO.encode(up, x) - RO.encode(dn, x)) * d).sum() / (2 * h)
    assert abs(fd - g[key][idx]) <= 1e-5 * max(1.0, abs(fd))


# ---- host logic on a stub engine ---------------------------------------------------------------------------------------------------------
class DPStub(TrainStub):
    """TrainStub plus the encoder calls of DPTrainAgent.update: features and the condition gradient are seeded, nothing is computed."""

    def __init__(self):
        super().__init__()
        self.loaded.update({f"encoder{i}": None for i in range(4)})
        self.encoder_uploads = [0] * 4

    def load_encoder(self, slot, params, version=None):
        self.calls.append(("load_encoder", slot))
        self.loaded[f"encoder{slot}"] = version
        self.encoder_uploads[slot] += 1

    def train_encoder_forward(self, slot, img):
        self.calls.append(("enc_fwd", slot, tuple(img.shape)))
        n = img.shape[0]
        return (torch.arange(n * 1024, dtype=torch.float32).reshape(n, 1024) + 1e6 * (slot + 1))

    def train_planner_grad_cond(self, x0, noise, t, cond, alpha=1.0):
        self.calls.append(("planner_grad_cond", x0, noise, np.asarray(t), cond, alpha))
        return torch.tensor(self.PLAN_LOSS), -cond

    def train_encoder_backward(self, slot, dfeat):
        self.calls.append(("enc_bwd", slot, dfeat))


def _stub_agent(cfg="rm_img", shared=False, oh=OH):
    from latent_diffusion_planning_amd.dp_agent import DPState
    from latent_diffusion_planning_amd.dp_train_agent import DPTrainAgent
    from latent_diffusion_planning_amd.schedule import warmup_cosine_decay_schedule
    data = RO.BY_NAME[cfg]
    small = W.ResNetSpec(n_filters=8)
    enc = {k: DPState(W.init_resnet_params(small, seed=20 + i), None, ema_is_params=True) for i, k in enumerate(RO.encoder_keys(data, shared))}
    pl = DPState({"Dense_0/kernel": rng(3).standard_normal((4, 16)).astype(np.float32), "Dense_0/bias": np.zeros(16, np.float32)}, None,
                 ema_is_params=True)
    config = dict(n_diffusion_steps=100, lowdim_obs=list(data["lowdim_obs"]), rgb_obs=list(data["rgb_obs"]), obs_horizon=oh, name="dp_agent",
                  action_dim=7, pred_horizon=T, action_horizon=AH, shared_encoder=shared)
    norm = {"obs": dict(data["obs_normalization"]["obs"]), "actions": dict(data["obs_normalization"]["actions"])}
    ag = DPTrainAgent(pl, enc, norm, config, DPStub(), RO.planner_spec(data, oh), torch.device("cpu"),
                      lr_schedule=warmup_cosine_decay_schedule(1e-6, 1e-4, 500, 100000, 1e-6))
    ag.planner_ema_decay, ag.encoder_ema_decay = 0.99, 0.98
    ag._planner_shapes = lambda: {k: v.shape for k, v in pl.params.items()}
    ag._encoder_shapes = lambda: W.resnet_shapes(small)
    return ag, data


def _batch(data, B, seed, oh=OH):
    b = RO.synth_image_batch(data, B, oh, seed, with_actions=True, T=T)
    g = rng(seed + 1)
    return b, dict(t=g.integers(0, 100, B), noise=g.standard_normal((B, T, 7)).astype(np.float32))


@pytest.mark.parametrize("cfg,shared,keys", [("rm_img", False, ["agentview_image"]),
                                             ("rm_img2", False, ["agentview_image", "robot0_eye_in_hand_image"]),
                                             ("rm_img2", True, ["shared"])])
def test_metric_keys_and_call_order(cfg, shared, keys):
    ag, data = _stub_agent(cfg, shared)
    batch, noise = _batch(data, 2, 1)
    new, m = ag.update(batch, 0, 0, noise=noise)
    want = ["loss", "obs_min", "obs_max", "obs_mean", "obs_std", "planner_lr", "planner_step"]
    want += [f"enc_{k}_{s}" for k in keys for s in ("lr", "step")]
    assert sorted(m) == sorted(want)
    assert float(m["loss"]) == DPStub.PLAN_LOSS
    eng = ag._engine
    kinds = [k for k in eng.kinds() if k not in ("stats",)]
    n = len(keys)
    assert kinds == ["load", "ema"] * (n + 1) + ["enc_fwd"] * n + ["planner_grad_cond"] + ["enc_bwd"] * n + ["apply"] * (n + 1)
    assert [c[1:] for c in eng.of("ema")] == [("planner", 0.99)] + [(f"encoder{i}", 0.98) for i in range(n)]
    ncam = len(data["rgb_obs"])
    assert [c[2] for c in eng.of("enc_fwd")] == [(2 * OH * (ncam if shared else 1), 64, 64, 3)] * n
    assert type(new) is type(ag) and new.planner_ema_decay == 0.99 and new.encoder_ema_decay == 0.98
    assert sorted(new.config) == sorted(ag.config) and len(new.config) == 9
    assert new.planner_state.step == 1 and all(st.step == 1 for st in new.encoder_state_dict.values())
    with pytest.raises(NotImplementedError):
        new.update_mixed(batch, batch, 0, 0)


def test_each_states_lr_follows_its_own_step_and_nothing_is_reloaded():
    ag, data = _stub_agent("rm_img2")
    batch, noise = _batch(data, 2, 2)
    wrist = "robot0_eye_in_hand_image"
    esd = dict(ag.encoder_state_dict)
    esd[wrist] = esd[wrist].replace(step=300)
    ag = ag.replace(planner_state=ag.planner_state.replace(step=40), encoder_state_dict=esd)
    sched = ag.lr_schedule
    ag1, m = ag.update(batch, 0, 0, noise=noise)
    assert (m["planner_step"], m["enc_agentview_image_step"], m[f"enc_{wrist}_step"]) == (40, 0, 300)
    assert m["planner_lr"] == np.float32(sched(40)) and m["enc_agentview_image_lr"] == np.float32(sched(0))
    assert m[f"enc_{wrist}_lr"] == np.float32(sched(300))
    eng = ag._engine
    assert [(c[1], c[2]) for c in eng.of("apply")] == [("planner", float(np.float32(sched(40)))), ("encoder0", float(np.float32(sched(0)))),
                                                       ("encoder1", float(np.float32(sched(300))))]
    assert [(c[1], c[2]) for c in eng.of("load")] == [("planner", 40), ("encoder0", 0), ("encoder1", 300)]
    eng.calls.clear()
    ag2, m2 = ag1.update(batch, 0, 1, noise=noise)          # the token hand-off: the arenas hold ag1's states
    assert eng.of("load") == [] and eng.of("ema") == [] and eng.of("write") == []
    assert (m2["planner_step"], m2[f"enc_{wrist}_step"]) == (41, 301)
    # replace(encoder_state_dict=...) with one new tree reloads only that slot
    esd = dict(ag2.encoder_state_dict)
    other = {k: v + 1 for k, v in ag.encoder_state_dict[wrist].params.items()}
    esd[wrist] = esd[wrist].replace(params=other, ema_params=other)
    eng.calls.clear()
    ag2.replace(encoder_state_dict=esd).update(batch, 0, 2, noise=noise)
    assert [c[1] for c in eng.of("load")] == ["encoder1"]
    # a superseded state cannot be read back
    with pytest.raises(RuntimeError, match="superseded by a later update"):
        ag1.planner_state.params


def test_sampling_side_publishes_a_trained_encoder_instead_of_uploading_it():
    ag, data = _stub_agent("rm_img2")
    batch, noise = _batch(data, 2, 3)
    eng = ag._engine
    ag._sync_weights()                                      # host trees: uploaded
    assert eng.encoder_uploads == [1, 1, 0, 0] and len(eng.of("load_params")) == 1
    new, _ = ag.update(batch, 0, 0, noise=noise)
    eng.calls.clear()
    new._sync_weights()
    assert eng.encoder_uploads == [1, 1, 0, 0] and eng.of("load_params") == []
    assert [c[1] for c in eng.of("publish")] == [["planner"], ["encoder0"], ["encoder1"]]
    eng.calls.clear()
    new._sync_weights()
    assert eng.calls == []


@pytest.mark.parametrize("oh", [1, 2])
@pytest.mark.parametrize("shared", [False, True])
def test_inverse_condition_layout(oh, shared):
    from latent_diffusion_planning_amd.dp_agent import dp_image_cond
    from latent_diffusion_planning_amd.dp_train_agent import dp_image_cond_inverse
    ag, data = _stub_agent("rm_img2", shared, oh)
    B, ncam = 3, 2
    frames = [ncam * oh] if shared else [oh, oh]
    g = rng(9)
    feats = [torch.tensor(g.standard_normal((B * f, 1024)).astype(np.float32)) for f in frames]
    low = torch.tensor(g.standard_normal((B, oh, RO.lowdim_dim(data))).astype(np.float32))
    cond = dp_image_cond(feats, low)
    assert cond.shape == (B, RO.cond_dim(data, oh))
    back = dp_image_cond_inverse(cond, frames)
    assert len(back) == len(feats) and all(torch.equal(a, b) and a.is_contiguous() for a, b in zip(back, feats))
    # and inside update: every encoder's backward receives its own block of the (stub's) condition gradient -cond
    batch, noise = _batch(data, B, 4, oh)
    ag.update(batch, 0, 0, noise=noise)
    eng = ag._engine
    cond_u = eng.of("planner_grad_cond")[0][4]
    for c, want in zip(eng.of("enc_bwd"), dp_image_cond_inverse(-cond_u, frames)):
        assert torch.equal(c[2], want)
    nobs = RO.normalized_obs(data, batch["obs"])
    ins = RO.encoder_inputs(data, nobs, oh, shared)
    feats_u = {k: (torch.arange(v.shape[0] * 1024, dtype=torch.float32).reshape(-1, 1024) + 1e6 * (i + 1)).numpy() for i, (k, v) in enumerate(ins.items())}
    np.testing.assert_array_equal(cond_u.numpy()[:, :sum(frames) * 1024], RO.obs_cond_from_features(data, nobs, feats_u, oh, shared)[:, :sum(frames) * 1024])


def test_dpagent_update_still_raises_its_message():
    from latent_diffusion_planning_amd.dp_agent import DPAgent
    ag, _ = _stub_agent()
    plain = DPAgent(ag.planner_state, ag.encoder_state_dict, ag.obs_normalization, ag.config, None, ag._planner_spec, torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="backward pass of the ResNet encoder.*trained with the reference"):
        plain.update({}, 0, 0)
    with pytest.raises(ValueError, match="optimiser settings"):
        ag.replace().__class__(ag.planner_state, ag.encoder_state_dict, ag.obs_normalization, ag.config, DPStub(), ag._planner_spec,
                               torch.device("cpu")).update({}, 0, 0)
