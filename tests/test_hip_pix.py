"""The pixel-observed reach task on the GPU (csrc/pix.hip, toyenv.Reach2DPixelEnv): `ldp_pix_render` against the NumPy
restatement of tests/pix_oracle.py byte for byte, the environment's frames and the recorded demonstrations against the same, the StableVAE
on drawn frames and encode_demos against the agent's own encode, and the closed loop pixels -> VAE -> planner -> IDM -> action with a
random-weight agent against a hand-written observe -> sample -> step loop."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import pix_oracle as P
from tests import toyenv_oracle as O
from tests.util import idm_params, planner_params, rng

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = 0x1234_5678_9ABC_DEF1
FRAME = 64 * 64 * 3
FILL = 0xAB


def _rows(M, seed):
    """(pos, goal) rows (M, 2): uniform in the square, with the rows a renderer can get wrong written over the first ones and the last one --
    the walls (+-1), outside the square (+-3), NaN, p = g, and a centre on a pixel centre."""
    g = rng(seed)
    pos, goal = g.uniform(-1, 1, (M, 2)).astype(F32), g.uniform(-1, 1, (M, 2)).astype(F32)
    special = [((1, -1), (-1, 1)), ((3, 0), (0.5, -3)), ((np.nan, 0.2), (0.3, np.nan)), ((0.25, -0.5), (0.25, -0.5)),
               ((P.CENTRES[7], P.CENTRES[60]), (-3, -3)), ((-1, -1), (1, 1))]
    for i, (p, q) in enumerate(special[:M]):
        r = (M - 1) if i == 0 else i - 1                                            # the first special row goes LAST: the end of the buffer
        pos[r], goal[r] = p, q
    return pos, goal


def _render(pos_ptr, ps, goal_ptr, gs, M, out):
    from latent_diffusion_planning_amd import _pixlib
    _pixlib.check(_pixlib.load().ldp_pix_render(pos_ptr, ps, goal_ptr, gs, M, out.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))


def _buffer(M):
    """M frames and 16 guard bytes of torch.empty memory, pre-filled: an unwritten byte shows, and so does a byte written past the end."""
    out = torch.empty(M * FRAME + 16, dtype=torch.uint8, device="cuda")
    out.fill_(FILL)
    assert out.data_ptr() % 16 == 0
    return out


def _same_frames(got, want, what=""):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert not len(bad), f"{what}: {len(bad)} bytes differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


# ---- the kernel against the restatement, byte for byte -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rows257():
    pos, goal = _rows(257, 11)
    return pos, goal, P.render(pos, goal)


@pytest.mark.parametrize("layout", ["packed", "state"])
@pytest.mark.parametrize("M", [1, 3, 257])
def test_render_equals_the_restatement(M, layout, rows257):
    pos, goal = _rows(M, 11)
    want = rows257[2] if M == 257 else P.render(pos, goal)
    out = _buffer(M)
    if layout == "packed":                                                          # recorded (M, 2) tables, stride 2
        p, g = torch.from_numpy(pos).cuda(), torch.from_numpy(goal).cuda()
        _render(p.data_ptr(), 2, g.data_ptr(), 2, M, out)
    else:                                                                           # the live state (M, 8): goal = state + 2, strides 8
        st = np.full((M, 8), 7.0, F32)
        st[:, 0:2], st[:, 2:4] = pos, goal
        s = torch.from_numpy(st).cuda()
        _render(s.data_ptr(), 8, s.data_ptr() + 8, 8, M, out)
    got = out.cpu().numpy()
    assert np.all(got[M * FRAME:] == FILL), "the 16 bytes after the last frame were written"
    _same_frames(got[:M * FRAME].reshape(M, 64, 64, 3), want, f"M={M} {layout}")
    assert want[..., 2].max() == 252 and want[..., 0].any() and want[..., 1].any()


def test_frames_do_not_depend_on_the_split(rows257):
    pos, goal, want = rows257
    p, g = torch.from_numpy(pos).cuda(), torch.from_numpy(goal).cuda()
    a, b = _buffer(100), _buffer(157)
    _render(p.data_ptr(), 2, g.data_ptr(), 2, 100, a)
    _render(p.data_ptr() + 100 * 8, 2, g.data_ptr() + 100 * 8, 2, 157, b)
    got = torch.cat([a[:100 * FRAME], b[:157 * FRAME]]).reshape(257, 64, 64, 3)
    _same_frames(got, want, "[0, 100) + [100, 257)")
    assert bool((a[100 * FRAME:] == FILL).all()) and bool((b[157 * FRAME:] == FILL).all())


def test_refusals_on_device_pointers():
    from latent_diffusion_planning_amd import _lib, _pixlib
    lib = _pixlib.load()
    s, out = torch.zeros((4, 8), device="cuda"), _buffer(4)
    p, f = s.data_ptr(), out.data_ptr()
    for call, word in ((lambda: lib.ldp_pix_render(p, 8, p + 8, 8, 0, f, None), "M must be"),
                       (lambda: lib.ldp_pix_render(None, 8, p + 8, 8, 4, f, None), "null pos"),
                       (lambda: lib.ldp_pix_render(p, 8, p + 8, 1, 4, f, None), "goal_stride"),
                       (lambda: lib.ldp_pix_render(p, 8, p + 8, 8, 4, f + 4, None), "aligned")):
        with pytest.raises(_lib.LDPHipError, match=word) as e:
            _pixlib.check(call())
        assert e.value.code == -1
    torch.cuda.synchronize()
    assert bool((out == FILL).all())                                                # a refused call wrote nothing


# ---- Reach2DPixelEnv -------------------------------------------------------------------------------------------------------------------------
def _env(N, A=2):
    from latent_diffusion_planning_amd.toyenv import Reach2DPixelEnv
    return Reach2DPixelEnv(N, action_dim=A)


def test_pixel_env_observes_its_state():
    N = 5
    env = _env(N)
    env.reset(SEED, 40)
    ob = env.observe()
    assert list(ob) == ["obs"] and set(ob["obs"]) == {"pos", "image"}
    pos, img = ob["obs"]["pos"], ob["obs"]["image"]
    assert pos.shape == (N, 1, 2) and pos.dtype == torch.float32 and pos.is_cuda
    assert img.shape == (N, 1, 64, 64, 3) and img.dtype == torch.uint8 and img.device == env.state.device and img.is_contiguous()
    st = env.state.cpu().numpy()
    assert np.array_equal(st, O.reset(N, SEED, 40))                                 # the task itself is Reach2DEnv's
    assert np.array_equal(pos.cpu().numpy()[:, 0], st[:, 0:2])
    _same_frames(img[:, 0], P.render_state(st), "after the reset")
    # a whole expert episode later the frames still are the render of the state read back
    for _ in range(O.H // 4):
        env.step_scripted("expert", 0.1, n_sub=4)
    st2 = env.state.cpu().numpy()
    assert np.array_equal(st2, O.rollout(N, O.EXPERT, 0.1, seed=SEED, episode0=40)[0]) and not np.array_equal(st2[:, :2], st[:, :2])
    _same_frames(env.observe()["obs"]["image"][:, 0], P.render_state(st2), "after the episode")


def test_goal_observation_puts_the_point_on_the_goal():
    env = _env(3)
    env.reset(SEED, 7)
    before = env.state.clone()
    g = env.goal_observation()
    st = before.cpu().numpy()
    assert set(g) == {"pos", "image"} and g["image"].shape == (3, 1, 64, 64, 3) and g["image"].dtype == torch.uint8
    img = g["image"][:, 0].cpu().numpy()
    assert np.array_equal(img[..., 0], img[..., 1]) and img[..., 0].any()
    _same_frames(img, P.render(st[:, 2:4], st[:, 2:4]), "p = g")
    assert np.array_equal(g["pos"].cpu().numpy()[:, 0], st[:, 2:4]) and torch.equal(env.state, before)


# ---- collect_pixel_demos -----------------------------------------------------------------------------------------------------------------------
N_DEMO = 4
ROWS = N_DEMO * O.H                                       # 192 frames


@pytest.fixture(scope="module")
def demos():
    from latent_diffusion_planning_amd.toyenv import collect_pixel_demos
    return collect_pixel_demos(N_DEMO, SEED, 0.1, episode0=2000)


def test_recorded_frames_equal_the_restatement(demos):
    _, act, pos, goal, _ = O.rollout(N_DEMO, O.EXPERT, 0.1, seed=SEED, episode0=2000)
    t = demos.tables
    assert set(t) == {"pos", "image", "actions"} and demos.obs_keys == ("pos", "image") and demos.total_n_sequences == ROWS
    assert t["image"].shape == (ROWS, 64, 64, 3) and t["image"].dtype == torch.uint8 and t["pos"].shape == (ROWS, 2) and t["actions"].shape == (ROWS, 2)
    assert t["pos"].dtype == t["actions"].dtype == torch.float32
    assert np.array_equal(t["pos"].cpu().numpy(), pos.reshape(ROWS, 2)) and np.array_equal(t["actions"].cpu().numpy(), act.reshape(ROWS, 2))
    _same_frames(t["image"], P.render(pos.reshape(ROWS, 2), goal.reshape(ROWS, 2)), "demonstration frames")
    b = demos.bounds.cpu().numpy()
    assert np.array_equal(b[:, 0], np.repeat(np.arange(N_DEMO) * O.H, O.H)) and np.array_equal(b[:, 1], b[:, 0] + O.H)


def test_a_drawn_batch_has_the_shapes_the_vae_trains_on(demos):
    idx = torch.tensor([0, 5, O.H - 1, ROWS - 1], dtype=torch.int32)
    batch = demos.sample(4, 0, 0, indices=idx.tolist())
    img = batch["obs"]["image"]
    assert img.shape == (4, 1, 64, 64, 3) and img.dtype == torch.uint8 and batch["obs"]["pos"].shape == (4, 1, 2)
    assert torch.equal(img[:, 0], demos.tables["image"][idx.long().cuda()])
    drawn = next(demos.batches(6, seed=1))
    assert drawn["obs"]["image"].shape == (6, 1, 64, 64, 3) and drawn["obs"]["image"].dtype == torch.uint8 and drawn["actions"].shape == (6, 1, 2)


# ---- the StableVAE on the frames, and encode_demos ---------------------------------------------------------------------------------------------
def test_two_vae_updates_on_drawn_frames(demos):
    from latent_diffusion_planning_amd.toyenv import reach2d_vae_config
    from latent_diffusion_planning_amd.vae_model import StableVAEModel
    cfg = reach2d_vae_config()
    model = StableVAEModel.create(3, None, cfg["shape_meta"], **cfg["vae_kwargs"])
    try:
        it = demos.batches(8, seed=2)
        for step in range(2):
            model, m = model.update(next(it), 10 + step, step)
            vals = {k: float(v) for k, v in m.items()}
            assert all(np.isfinite(v) for v in vals.values()), vals
            assert 0 < vals["loss_mse"] < 4 and -1 <= vals["img_min"] <= vals["img_max"] <= 1 and vals["vae_step"] == step
        p = model.get_params()["vae_params"]
        assert all(np.isfinite(np.asarray(v)).all() for v in p.values())
    finally:
        model._engine.close()


@pytest.fixture(scope="module")
def agent():
    from latent_diffusion_planning_amd import weights as W
    from latent_diffusion_planning_amd.agent import LDPAgent
    from latent_diffusion_planning_amd.toyenv import reach2d_pixel_config
    cfg = reach2d_pixel_config()
    ag = LDPAgent.create(0, None, cfg["shape_meta"], vae_params=W.init_vae_params(seed=2), **cfg["agent_kwargs"])
    assert ag.config["obs_dim"] == 18
    pp, ip = planner_params(D=18), idm_params(D=18, A=2)
    ag = ag.replace(planner_state=ag.planner_state.replace(params=pp, ema_params=pp), idm_state=ag.idm_state.replace(params=ip, ema_params=ip))
    yield ag
    ag._engine.close()


@pytest.fixture(scope="module")
def encoded(demos, agent):
    from latent_diffusion_planning_amd.toyenv import encode_demos
    return encode_demos(demos, agent, chunk=64)


def test_encode_demos_equals_the_agents_own_encode(demos, agent, encoded):
    ds, (lo, hi) = encoded
    z = ds.tables["latent_image"]
    assert set(ds.tables) == {"pos", "latent_image", "actions"} and ds.obs_keys == ("pos", "latent_image") and (ds.frame_stack, ds.seq_length) == (1, 9)
    assert z.shape == (ROWS, 16) and z.dtype == torch.float32 and bool(torch.isfinite(z).all()) and float(z.std()) > 0
    assert ds.tables["pos"] is demos.tables["pos"] and ds.tables["actions"] is demos.tables["actions"]
    # agent.vae_encode on the same 64 frames, normalised as encode_demos normalises them: the raw latents under the agent's own latent map
    frames = demos.tables["image"][:64]
    x = agent._engine.normalize_bounds(frames, [0.0], [255.0], True)
    want = (frames.float() / 255 - 0.5) / 0.5
    assert float((x - want).abs().max()) <= 4e-7                                    # (x / 255 - 0.5) / 0.5 as preencode: three roundings of <= 2^-24 each way
    got = agent.vae_encode({"image": x.reshape(64, 1, 64, 64, 3)})["latent_image"].tensor
    ref = agent._apply_norm(z[:64].reshape(64, 1, 16).contiguous(), agent.obs_normalization["obs"]["latent_image"], True)
    assert got.shape == (64, 1, 16) and torch.equal(got, ref)
    # the bounds are the table's own
    zn = z.cpu().numpy()
    assert lo.shape == hi.shape == (16,) and lo.dtype == hi.dtype == F32
    assert np.array_equal(lo, zn.min(0)) and np.array_equal(hi, zn.max(0))


def test_encode_demos_does_not_depend_on_the_chunk(demos, agent, encoded):
    """chunk = 64 and chunk = 192 on the same 192 frames: both at most 256 frames, so the same arithmetic form on different tilings of the
    batch; they agree within 1e-4 (not compared across the 256-frame boundary, where the form changes)."""
    from latent_diffusion_planning_amd.toyenv import encode_demos
    whole, (lo, hi) = encode_demos(demos, agent, chunk=192)
    a, b = encoded[0].tables["latent_image"], whole.tables["latent_image"]
    err = float((a - b).abs().max())
    print(f"chunk 64 vs 192: max |diff| {err:.3e} on latents of max |z| {float(b.abs().max()):.3f}")
    assert err <= 1e-4
    assert np.abs(lo - encoded[1][0]).max() <= 1e-4 and np.abs(hi - encoded[1][1]).max() <= 1e-4


# ---- the closed loop: pixels -> VAE -> planner -> IDM -> action -> environment --------------------------------------------------------------------
N_LOOP, RNG = 3, 21


def _hand_loop(env, call, episodes=(0,)):
    n, states = 0, []
    for e0 in episodes:
        env.reset(SEED, e0)
        for c in range(O.H // 4):
            n += 1
            batch = env.observe()
            assert batch["obs"]["image"].dtype == torch.uint8
            action = call(batch, RNG * 1000003 + n)[0]
            assert action.shape == (N_LOOP, 4, 2)
            env.step(action.tensor)
        states.append(env.state.clone())
    return states


def test_run_device_eval_on_pixels_equals_the_hand_loop_and_repeats(agent):
    from latent_diffusion_planning_amd import harness
    sample = lambda batch, r, cycle=None: agent.sample(batch, r, sampler="ddim", n_steps=10)      # noqa: E731
    env = _env(N_LOOP)
    want = _hand_loop(env, sample, episodes=(0, N_LOOP))
    assert not np.array_equal(want[1][:, :2].cpu().numpy(), O.reset(N_LOOP, SEED, N_LOOP)[:, :2])                 # the policy moved the points
    for rep in range(2):
        res = harness.run_device_eval(env, sample, 2 * N_LOOP, SEED, RNG)
        assert torch.equal(env.state.view(torch.int32), want[1].view(torch.int32)), f"state after the last round, run {rep}"
        s = torch.cat(want).cpu().numpy()
        ok = s[:, O.FIRST] != 0
        assert res["success_rate"] == float(ok.mean()) and res["blocked_share"] == float(s[:, O.BLOCKED].sum() / (len(s) * O.H))
        assert res["n_calls"] == 24 and res["cycles_per_episode"] == 12
    # the goal reaches the plan through the pixels and through nothing else: another goal, another action
    env.reset(SEED, 0)
    b1 = env.observe()
    env.state[:, 3] = -env.state[:, 3] - 0.2
    b2 = env.observe()
    assert torch.equal(b1["obs"]["pos"], b2["obs"]["pos"]) and not torch.equal(b1["obs"]["image"], b2["obs"]["image"])
    a1, a2 = sample(b1, 5)[0].tensor, sample(b2, 5)[0].tensor
    assert not torch.equal(a1, a2)


def test_fit_on_encoded_demonstrations(agent, encoded):
    from latent_diffusion_planning_amd import harness
    from latent_diffusion_planning_amd.toyenv import with_latent_bounds
    ds, bounds = encoded
    ag = with_latent_bounds(agent, bounds)
    assert ag.obs_normalization["obs"]["latent_image"]["min"].shape == (16,) and agent.obs_normalization["obs"]["latent_image"]["min"] == -1.0
    logged = []
    fitted, m = harness.fit(ag, ds.batches(32, seed=2), 10, 4, log_every=5, on_log=lambda s, d: logged.append((s, d)))
    assert [s for s, _ in logged] == [5, 10]
    for _, d in logged:
        assert np.isfinite(d["loss"]) and np.isfinite(d["plan_loss"]) and np.isfinite(d["idm_loss"]), d
    env = _env(N_LOOP)
    res = harness.run_device_eval(env, lambda b, r, c: fitted.sample(b, r, sampler="ddim", n_steps=10), N_LOOP, SEED, RNG)
    assert 0 <= res["success_rate"] <= 1 and bool(torch.isfinite(env.state).all())
