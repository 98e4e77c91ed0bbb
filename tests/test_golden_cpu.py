"""The committed golden fixtures are reproducible from the oracle (CPU): re-evaluates the cheap
cases bit-for-bit and checks every fixture's stored inputs against its seed."""
import numpy as np
import pytest

from oracle import np64
from tests.cases import CASES, load_case
from tests.util import idm_params


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_loads_and_inputs_match_seed(name):
    inp, exp = load_case(name)
    assert exp and all(np.isfinite(v).all() for v in exp.values())


@pytest.mark.parametrize("name", ["idm_loop_rm_ddpm100", "idm_loop_aloha_ddim50", "planner_loop_ddim50"])
def test_oracle_reproduces_fixture(name):
    """Bit for bit on every host: the loop fixtures are evaluated with the GEMMs in a fixed order, without BLAS, and with
    correctly rounded float32 sqrt / sin / cos (tests/cases.py _fixed_order)."""
    fn, args = CASES[name]
    inp, compute = fn(*args)
    for k in inp:                                   # the fixture was generated from float32-rounded inputs
        inp[k][...] = np.asarray(inp[k], dtype=np.float32)
    out = compute()
    _, exp = load_case(name)
    for k, v in out.items():
        np.testing.assert_allclose(v, exp[k], rtol=0, atol=1e-12)


def test_fixture_agrees_with_the_numpy_definition():
    """idm_loop fixtures come from the torch-float64 restatement; the explicit NumPy loop
    (oracle/np64.py) must land on the same numbers."""
    inp, exp = load_case("idm_loop_rm_ddpm100")
    ref = np64.idm_sample(idm_params(), np.asarray(inp["tr"], np.float32), np.asarray(inp["a0"], np.float32),
                          np.asarray(inp["nz"], np.float32), 100, 100, "ddpm")
    np.testing.assert_allclose(ref, exp["act"], rtol=0, atol=5e-6)


def test_pin_hook_refuses_cleanly_without_the_jax_stack():
    """tests/golden/regen_from_reference.py regenerates every fixture from the JAX reference.  jax /
    flax / diffusers are not installable in the build image: the script must say exactly which module is missing and
    exit with code 3, touching nothing.  (Where they ARE installed this test is skipped: run the script instead.)"""
    import importlib.util
    import os
    import subprocess
    import sys
    if all(importlib.util.find_spec(m) is not None for m in ("jax", "flax", "diffusers")):
        pytest.skip("the JAX stack is present: run tests/golden/regen_from_reference.py")
    here = os.path.dirname(os.path.abspath(__file__))
    script = os.path.join(here, "golden", "regen_from_reference.py")
    before = {f: os.path.getmtime(os.path.join(here, "golden", f)) for f in os.listdir(os.path.join(here, "golden"))}
    r = subprocess.run([sys.executable, script, "--write"], capture_output=True, text=True)
    missing = next(m for m in ("jax", "flax", "diffusers") if importlib.util.find_spec(m) is None)
    assert r.returncode == 3 and f"cannot import '{missing}'" in r.stderr
    assert before == {f: os.path.getmtime(os.path.join(here, "golden", f)) for f in os.listdir(os.path.join(here, "golden"))}


# ---- the parts of the pin hook that can run without jax: it pins nothing here, it makes the one
# ---- command that CAN pin everything less likely to die on its first real run
def _regen_module():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "regen_from_reference.py")
    if not os.path.exists(path):
        pytest.skip("regen_from_reference.py does not travel to the GPU box (.gpurunignore)")
    spec = importlib.util.spec_from_file_location("regen_from_reference", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pin_hook_tree_comparison_names_what_differs(capsys):
    R = _regen_module()
    ours = {"Dense_0": {"kernel": np.zeros((3, 4)), "bias": np.zeros(4)}, "Block_1": {"Conv_0": {"kernel": np.zeros((5, 2, 2))}}}
    assert R.tree_shapes(ours) == {"Dense_0/kernel": (3, 4), "Dense_0/bias": (4,), "Block_1/Conv_0/kernel": (5, 2, 2)}
    R.assert_same_tree("toy", ours, {k: dict(v) for k, v in ours.items()})
    assert "3 leaves, names and shapes equal module.init()" in capsys.readouterr().out
    theirs = {"Dense_0": {"kernel": np.zeros((3, 5)), "bias": np.zeros(4)}, "Block_0": {"Conv_0": {"kernel": np.zeros((5, 2, 2))}}}
    with pytest.raises(SystemExit) as e:
        R.assert_same_tree("toy", ours, theirs)
    msg = str(e.value)
    assert "missing here: ['Block_0/Conv_0/kernel']" in msg and "not in the reference: ['Block_1/Conv_0/kernel']" in msg
    assert "('Dense_0/kernel', (3, 4), (3, 5))" in msg


@pytest.mark.parametrize("sampler,n_steps", [("ddpm", 100), ("ddim", 50), ("ddim", 100)])
def test_pin_hook_loop_visits_the_timesteps_and_noise_rows_the_oracle_does(sampler, n_steps):
    """run_loop (what the pin hook wraps around the reference network and FlaxDDPMScheduler.step) against
    np64.idm_sample with the oracle's own network and scheduler plugged in: same k sequence, same noise row per step."""
    R = _regen_module()
    from tests.util import rng
    ip = idm_params()
    g = rng(5)
    tr, a0, nz = g.uniform(-1, 1, (3, 50)), g.standard_normal((3, 7)), g.standard_normal((n_steps, 3, 7))
    tables = np64.ddpm_tables(100)
    seen = []

    def eps_net(a, k):
        seen.append(k)
        return np64.idm_forward(ip, tr, a, k)

    got = R.run_loop(eps_net, np.asarray(a0, np.float64), nz if sampler == "ddpm" else None, 100, n_steps, sampler,
                     step_ddpm=lambda eps, k, x, z: np64.ddpm_step(eps, k, x, z if k > 0 else 0.0, tables),
                     step_ddim=lambda eps, k, kp, x: np64.ddim_step(eps, k, kp, x, tables))
    want = np64.idm_sample(ip, tr, a0, nz.astype(np.float32) if sampler == "ddpm" else None, 100, n_steps, sampler)
    stride = 100 // n_steps
    assert seen == [(n_steps - 1 - i) * stride for i in range(n_steps)] and seen[-1] == 0
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


def test_pin_hook_write_round_trip_on_a_copy(tmp_path):
    """regen_fixture on a temp copy of a fixture with the oracle as the 'reference': differences are zero, --write keeps
    the inputs, rewrites the outputs as float64 and records who pinned it; a deliberately different 'reference' shows up
    in the printed difference and in the rewritten file."""
    import shutil
    R = _regen_module()
    from tests.cases import golden_path
    name = "idm_loop_rm_ddim50"
    path = str(tmp_path / (name + ".npz"))
    shutil.copy(golden_path(name), path)
    fn, args = CASES[name]
    inp, compute = fn(*args)
    lines = []
    assert R.regen_fixture(name, path, inp, compute, False, "nobody", log=lines.append) <= 1e-12
    assert lines and "max|reference - stored| = " in lines[0]
    with np.load(path) as z:
        assert "pinned_by" not in z.files
    inp, compute = fn(*args)
    worst = R.regen_fixture(name, path, inp, lambda: {k: v + 0.25 for k, v in compute().items()}, True, "JAX reference at X; jax 0.4.26")
    assert abs(worst - 0.25) < 1e-9
    with np.load(path) as new, np.load(golden_path(name)) as old:
        assert str(new["pinned_by"]) == "JAX reference at X; jax 0.4.26"
        for k in old.files:
            if k.startswith("in_"):
                assert np.array_equal(new[k], old[k]) and new[k].dtype == old[k].dtype
            else:
                assert new[k].dtype == np.float64 and np.allclose(new[k], old[k] + 0.25, atol=1e-12)


def test_pin_hook_names_only_plan_and_refusal():
    """--check-names-only (round 5): the PLAN of what it compares is jax-free -- labels, constructor facts, init input shapes and this
    repository's shape tables for planner (T = 8 / 16, D = 25 / 30), IDM and the hierarchical agent's two-level IDM U-Net; without flax the
    mode stops with the exact missing module like the full run does."""
    import importlib.util
    import os
    import subprocess
    import sys
    R = _regen_module()
    plan = R.name_check_plan()
    labels = [p[0] for p in plan]
    assert any("T=16" in lb for lb in labels) and any("hier" in lb for lb in labels) and sum("idm D=" in lb for lb in labels) == 2
    for label, kind, facts, shp, ours in plan:
        assert kind in ("unet", "idm") and all(isinstance(v, tuple) for v in ours.values())
        if kind == "unet":
            assert shp["x"][2] == facts["input_dim"] and shp["cond"][1] == facts["global_cond_dim"]
            assert ours["Conv_0/kernel"] == (1, facts["down_dims"][0], facts["input_dim"])
            n_blocks = 2 * len(facts["down_dims"]) + 2 + 2 * (len(facts["down_dims"]) - 1)
            assert f"ConditionalResidualBlock1D_{n_blocks - 1}/Dense_0/kernel" in ours and f"ConditionalResidualBlock1D_{n_blocks}/Dense_0/kernel" not in ours
    if importlib.util.find_spec("flax") is None:
        script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "regen_from_reference.py")
        r = subprocess.run([sys.executable, script, "--check-names-only"], capture_output=True, text=True)
        missing = next(m for m in ("jax", "flax") if importlib.util.find_spec(m) is None)
        assert r.returncode == 3 and f"cannot import '{missing}'" in r.stderr


@pytest.mark.parametrize("name", ["agent_get_metrics_rm", "agent_hier_sample_viz_rm_ddim50_b3", "planner_loop_heavy_ddim50"])
def test_pin_hook_round_trip_on_the_round4_and_round5_fixtures(tmp_path, name):
    """regen_fixture on the get_metrics, hierarchical and trained-like fixtures with the oracle as the 'reference' (what the hook does
    after swapping np64.unet_forward / idm_forward / ddpm_add_noise and cases.hier_idm_fn for the reference's): zero difference; the
    trained-like fixture's `ref32_err` (this repository's float32 floor) is neither compared nor overwritten by --write."""
    import shutil
    R = _regen_module()
    from tests.cases import golden_path
    path = str(tmp_path / (name + ".npz"))
    shutil.copy(golden_path(name), path)
    fn, args = CASES[name]
    inp, compute = fn(*args)
    lines = []
    assert R.regen_fixture(name, path, inp, compute, True, "JAX reference at X", log=lines.append) <= 1e-9
    assert not any("ref32_err" in ln for ln in lines)
    with np.load(path) as new, np.load(golden_path(name)) as old:
        assert set(new.files) == set(old.files) | {"pinned_by"}
        if "out_ref32_err" in old.files:
            assert float(new["out_ref32_err"]) == float(old["out_ref32_err"])
