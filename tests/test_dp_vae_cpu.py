"""DPVAEAgent without a GPU: the DP condition layout, the create validations, the random_shift refusal, the EMA oracle, the
fixtures, the state's version tokens and the harness's dp* branch."""
import numpy as np
import pytest
import torch

from tests import cfgs, dp_oracle
from tests.golden.make_golden_dp import AH, CASES, N_UPDATE, OH, T, golden_path


def test_condition_layout_is_the_references_expression():
    from latent_diffusion_planning_amd.dp_vae_agent import dp_obs_cond
    data = cfgs.BY_NAME["rm"]
    batch = cfgs.synth_latent_batch(data, 3, 4, 5)
    nobs = dp_oracle.normalized_obs(data, batch["obs"])
    # the per-frame rows LDPAgent.get_obs_cond builds: [image latent | low-dim keys in order]
    low = np.concatenate([nobs[k] for k in data["lowdim_obs"]], axis=-1)
    frames = np.concatenate([nobs[data["rgb_obs"][0]], low], axis=-1)
    got = dp_obs_cond(torch.tensor(frames), OH, 16).numpy()
    want = dp_oracle.obs_cond(data, nobs, OH)                                  # agent/dp_repr_agent.py:76-85
    np.testing.assert_array_equal(got, want)
    # and it is NOT LDP's per-frame interleave
    assert not np.array_equal(got, frames[:, :OH].reshape(3, -1))
    assert got.shape == (3, OH * frames.shape[-1])


def _create(**over):
    from latent_diffusion_planning_amd.dp_vae_agent import DPVAEAgent
    data = cfgs.BY_NAME["rm"]
    kw = dp_oracle.dp_kwargs(data, OH, T, AH)
    kw.update(over)
    return DPVAEAgent.create(0, None, data["shape_meta"], **kw)


@pytest.mark.parametrize("over", [
    dict(planner=dict(down_dims=[256, 512, 1000], kernel_size=5, n_groups=8)),
    dict(planner=dict(down_dims=[256, 512, 1024], kernel_size=3, n_groups=8)),
    dict(planner=dict(down_dims=[256, 512, 1024], kernel_size=5, n_groups=4)),
    dict(rgb_obs=["latent_agentview_image", "latent_robot0_eye_in_hand_image"]),
    dict(vae_feature_dim=48),
])
def test_create_refuses_what_is_not_built(over):
    with pytest.raises(NotImplementedError):
        _create(**over)


def test_random_shift_is_refused_by_update():
    from latent_diffusion_planning_amd.dp_vae_agent import DPState, DPVAEAgent
    data = cfgs.BY_NAME["rm"]
    ag = DPVAEAgent(DPState({}), None, {"obs": {}}, dict(random_shift=4), None, None, None, torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="random_shift"):
        ag.update(cfgs.synth_latent_batch(data, 2, 2, 1, with_actions=True), 0, 0)


def test_ema_oracle_is_the_closed_form():
    """After n updates from e_0 = p_0: e_n = d^n p_0 + (1 - d) sum_k d^(n-k) p_k."""
    from collections import OrderedDict
    g = np.random.Generator(np.random.PCG64(0))
    d = 0.99
    ps = [OrderedDict(w=g.standard_normal(5), b=g.standard_normal(3)) for _ in range(6)]
    e = OrderedDict(ps[0])
    for p in ps[1:]:
        e = dp_oracle.ema_update(e, p, d)
    n = len(ps) - 1
    for k in e:
        closed = d ** n * ps[0][k] + (1 - d) * sum(d ** (n - j) * ps[j][k] for j in range(1, n + 1))
        np.testing.assert_allclose(e[k], closed, rtol=1e-12)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_integrity(name):
    z = np.load(golden_path(name))
    fn, args = CASES[name]
    inp, seeds, _ = fn(*args)                  # the inputs are regenerated from their seeds: the stored ones must be those
    for k, v in inp.items():
        np.testing.assert_array_equal(z[f"in_{k}"], np.asarray(v, np.float32), err_msg=k)
    for k, v in seeds.items():
        assert int(z[f"seed_{k}"]) == v
    for k in z.files:
        if k.startswith("out_"):
            assert np.all(np.isfinite(z[k])), k
    if name.startswith("dp_vae_sample"):
        B = z["in_x_init"].shape[0]
        assert z["out_action"].shape == (B, AH, z["in_x_init"].shape[-1]) and B <= 5
    else:
        assert z["out_loss"].shape == (N_UPDATE,) and z["out_grads"].shape[1] == 67
        assert np.abs(z["out_params_after_n"] - z["out_ema_after_n"]).max() > 0      # the EMA lags the parameters


def test_state_tokens_keep_params_and_ema_apart():
    from latent_diffusion_planning_amd.dp_vae_agent import DPState
    p = {"a": np.ones(3, np.float32)}
    st = DPState(p, None, ema_is_params=True)
    assert st.ema_params is st.params and st.ema_version != st.version
    q = {"a": np.zeros(3, np.float32)}
    moved = st.replace(params=q)                             # new parameters; the EMA stays the old ones
    np.testing.assert_array_equal(moved.ema_params["a"], p["a"])
    assert moved.version != st.version and moved.ema_version == st.ema_version
    restored = st.replace(params=q, ema_params=q)            # load_snapshot: params = EMA = restored
    assert restored.ema_is_params and restored.ema_version != st.ema_version
    np.testing.assert_array_equal(restored.ema_params["a"], q["a"])


class _FakeDP:
    config = {"name": "dp_vae_agent"}

    def __init__(self):
        self.calls = []

    def get_metrics(self, batch, rng):
        self.calls.append("get_metrics")
        return {"loss": np.float32(0.5)}

    def sample(self, batch, rng):
        self.calls.append("sample")
        return np.full((batch["actions"].shape[0], 2, 3), 0.25, np.float32), {}

    def sample_action(self, batch, rng):
        raise AssertionError("eval_bc.py:129-131 never calls sample_action for a dp agent")


def test_harness_dp_branch():
    from latent_diffusion_planning_amd import harness
    pol = _FakeDP()
    actions = np.zeros((4, 5, 3), np.float32)
    m = harness.eval_loss_metrics(pol, {"obs": {}, "actions": actions}, 0)
    assert pol.calls == ["get_metrics", "sample"]
    assert m["loss"] == 0.5 and m["full_action_mse"] == pytest.approx(0.0625)
    assert "action_mse" not in m and "plan_mse" not in m
