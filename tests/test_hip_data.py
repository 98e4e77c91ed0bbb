"""The device-resident data layer on the GPU (csrc/data.hip, latent_diffusion_planning_amd/data.py) against the NumPy oracle
(tests/data_oracle.py).  -m gpu.  Copies and integer draws have no tolerance: every comparison is bitwise."""
import numpy as np
import pytest
import torch

from latent_diffusion_planning_amd import data as D
from tests import cfgs
from tests import data_oracle as O
from tests.util import idm_params, make_agent, planner_params, rng

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 7, 40]
OBS = {"k1": (1,), "k7": (7,), "k9": (9,), "k16": (16,), "k36": (36,)}           # 4, 28, 36, 64 and 144 bytes a row
IMG = "img"                                                                     # 12 288 bytes a row
SEED64 = 0xC0FFEE1234567890


def _episodes(lengths, seed, with_img=True):
    g = rng(seed)
    eps = []
    for T in lengths:
        ep = {k: g.standard_normal((T,) + s).astype(np.float32) for k, s in OBS.items()}
        ep["actions"] = g.uniform(-1, 1, (T, 7)).astype(np.float32)
        if with_img:
            ep[IMG] = g.integers(0, 256, (T, 64, 64, 3)).astype(np.uint8)
        eps.append(ep)
    return eps


@pytest.fixture(scope="module")
def small():
    """The episodes and the oracle's weld, computed once and never changed."""
    eps = _episodes(LENGTHS, 11)
    keys = list(OBS) + [IMG]
    tables, st, en = O.weld(eps, ["actions"] + keys)
    return eps, keys, tables, st, en


def _assert_batch(got, ref, what=""):
    assert set(got) == set(ref) and set(got["obs"]) == set(ref["obs"])
    for k in [k for k in ref if k != "obs"]:
        g = got[k].cpu().numpy()
        assert g.dtype == ref[k].dtype and g.shape == ref[k].shape and np.array_equal(g, ref[k]), (what, k)
    for k, r in ref["obs"].items():
        g = got["obs"][k].cpu().numpy()
        assert g.dtype == r.dtype and g.shape == r.shape and np.array_equal(g, r), (what, k)


@pytest.mark.parametrize("fs, sl", [(1, 1), (2, 8), (2, 16), (4, 4)])
def test_every_index_of_a_small_set_matches_the_oracle(small, fs, sl):
    eps, keys, tables, st, en = small
    ds = D.DeviceDataset.from_episodes(eps, keys, frame_stack=fs, seq_length=sl)
    total = sum(LENGTHS)
    assert ds.total_n_sequences == total and ds.n_demos == len(LENGTHS)
    got = ds.sample(total, 0, 0, indices=np.arange(total))
    assert got["actions"].shape == (total, sl, 7) and got["obs"][IMG].shape == (total, fs + sl - 1, 64, 64, 3) and got["obs"][IMG].dtype == torch.uint8
    _assert_batch(got, O.batch(tables, st, en, np.arange(total), keys, ["actions"], fs, sl), f"fs {fs} sl {sl}")
    # explicit device indices, in another order and with repeats
    idx = torch.tensor([49, 0, 3, 3, 10, 9, 2, 1], device="cuda")
    _assert_batch(ds.sample(8, 0, 0, indices=idx), O.batch(tables, st, en, idx.cpu().numpy(), keys, ["actions"], fs, sl))


@pytest.mark.parametrize("step", [0, 2 ** 32 - 1])
@pytest.mark.parametrize("B", [1, 257, 4096])
def test_draw_equals_the_oracle_integers(small, B, step):
    eps, keys, *_ = small
    ds = D.DeviceDataset.from_episodes(eps, keys, frame_stack=2, seq_length=8)
    got = ds.draw(B, SEED64, step).cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, O.draw(SEED64, step, 0, B, [sum(LENGTHS)])[2])


def test_sample_without_indices_is_sample_of_the_draw(small):
    eps, keys, tables, st, en = small
    ds = D.DeviceDataset.from_episodes(eps, keys, frame_stack=2, seq_length=8)
    a = ds.sample(257, SEED64, 5)
    idx = ds.draw(257, SEED64, 5)
    used = torch.full((257,), -1, dtype=torch.int64, device="cuda")
    a2 = ds.sample(257, SEED64, 5, index_out=used)                                  # the launch reports the rows it used
    assert torch.equal(used, idx) and torch.equal(a2["obs"][IMG], a["obs"][IMG])
    far = torch.tensor([-5, 10 ** 12], device="cuda")                                # explicit indices outside the table are clamped into it
    clamped = torch.empty(2, dtype=torch.int64, device="cuda")
    c = ds.sample(2, 0, 0, indices=far, index_out=clamped)
    assert clamped.tolist() == [0, sum(LENGTHS) - 1] and torch.equal(c["actions"], ds.sample(2, 0, 0, indices=[0, sum(LENGTHS) - 1])["actions"])
    b = ds.sample(257, 1, 2, indices=idx)
    for k in keys:
        assert torch.equal(a["obs"][k], b["obs"][k]), k
    assert torch.equal(a["actions"], b["actions"])
    _assert_batch(a, O.batch(tables, st, en, O.draw(SEED64, 5, 0, 257, [sum(LENGTHS)])[2], keys, ["actions"], 2, 8))
    assert not torch.equal(ds.draw(257, SEED64, 5), ds.draw(257, SEED64, 6)) and not torch.equal(ds.draw(257, SEED64, 5), ds.draw(257, SEED64 + 1, 5))


def test_row_offset_keys_the_draw_by_the_global_row(small):
    eps, keys, *_ = small
    ds = D.DeviceDataset.from_episodes(eps, keys, frame_stack=2, seq_length=8)
    whole, part = ds.sample(8, 77, 3), ds.sample(3, 77, 3, row_offset=3)
    for k in keys:
        assert torch.equal(whole["obs"][k][3:6], part["obs"][k]), k
    assert torch.equal(whole["actions"][3:6], part["actions"])
    assert torch.equal(ds.draw(8, 77, 3)[3:6], ds.draw(3, 77, 3, row_offset=3))


def test_mixture_of_three_datasets_matches_the_oracle():
    lengths = ([1, 2, 7], [40], [2, 7, 40, 5])
    split = [0.2, 0.3, 0.5]
    keys = ["k9", "optimal", "k36"]
    parts, welded_eps = [], []
    for i, ln in enumerate(lengths):
        eps = _episodes(ln, 20 + i, with_img=False)
        parts.append(D.DeviceDataset.from_episodes(eps, keys, frame_stack=2, seq_length=8, optimal=int(i == 0)))
        welded_eps += [dict(ep, optimal=np.full((len(ep["actions"]), 1), float(i == 0), np.float32)) for ep in eps]
    mix = D.DeviceDataset.mix(parts, split)
    totals = [sum(ln) for ln in lengths]
    tables, st, en = O.weld(welded_eps, ["actions"] + keys)
    B = 4096
    which, _, welded = O.draw(SEED64, 9, 0, B, totals, split)
    got_idx = mix.draw(B, SEED64, 9).cpu().numpy()
    assert np.array_equal(got_idx, welded)
    base = np.concatenate([[0], np.cumsum(totals)])
    assert np.array_equal(np.searchsorted(base, got_idx, side="right") - 1, which) and len(set(which.tolist())) == 3
    got = mix.sample(B, SEED64, 9)
    _assert_batch(got, O.batch(tables, st, en, welded, keys, ["actions"], 2, 8))
    opt = got["obs"]["optimal"].cpu().numpy()
    assert np.array_equal(opt[:, 0, 0] == 1.0, which == 0) and set(np.unique(opt).tolist()) == {0.0, 1.0}


def test_a_table_offset_by_four_bytes_takes_the_word_path_and_agrees():
    """k16 rows are 64 bytes: on a 16-byte aligned base they move as 16-byte vectors.  The same table at base + 4 (a sliced tensor) can only
    move as 4-byte words.  Both results are the same bytes, and the oracle's."""
    eps = _episodes(LENGTHS, 31, with_img=False)
    keys = ["k16", "k36"]
    ds = D.DeviceDataset.from_episodes(eps, keys, frame_stack=2, seq_length=8)
    total = ds.total_n_sequences
    shifted = {}
    for k, t in ds.tables.items():
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
        buf[1:] = t.reshape(-1)
        shifted[k] = buf[1:].view(t.shape)
        assert shifted[k].data_ptr() % 16 == 4 and shifted[k].is_contiguous()
    ds4 = D.DeviceDataset(shifted, ds.bounds, keys, ("actions",), 2, 8, [0], [total], [1.0], len(LENGTHS))
    assert ds.tables["k16"].data_ptr() % 16 == 0
    a, b = ds.sample(total, 0, 0, indices=np.arange(total)), ds4.sample(total, 0, 0, indices=np.arange(total))
    tables, st, en = O.weld(eps, ["actions"] + keys)
    _assert_batch(a, O.batch(tables, st, en, np.arange(total), keys, ["actions"], 2, 8))
    for k in keys:
        assert torch.equal(a["obs"][k], b["obs"][k]), k
    assert torch.equal(a["actions"], b["actions"])


def test_byte_offsets_past_two_gib_are_64_bit():
    """A uint8 table of just over 2^31 bytes, allocated on the device and never on the host; only its last four rows are written.  The windows at
    the last indices read rows whose byte offsets need 32 bits and more."""
    row = 12288
    R = (2 ** 31) // row + 6                                                        # 174 768 rows, 2 147 549 184 bytes
    assert R * row > 2 ** 31 and (R - 4) * row > 2 ** 31
    table = torch.empty((R, row), dtype=torch.uint8, device="cuda")
    last = torch.from_numpy(rng(41).integers(0, 256, (4, row)).astype(np.uint8))
    table[R - 4:] = last.cuda()
    act = torch.zeros((R, 1), dtype=torch.float32, device="cuda")
    act[R - 4:, 0] = torch.arange(4, dtype=torch.float32, device="cuda")
    # two episodes: [0, R - 4) and [R - 4, R), written on the device
    bounds = torch.empty((R, 2), dtype=torch.int32, device="cuda")
    bounds[: R - 4, 0], bounds[: R - 4, 1] = 0, R - 4
    bounds[R - 4:, 0], bounds[R - 4:, 1] = R - 4, R
    ds = D.DeviceDataset({"img": table, "actions": act}, bounds, ["img"], ("actions",), 2, 3, [0], [R], [1.0], 2)
    idx = np.arange(R - 4, R)
    got = ds.sample(4, 0, 0, indices=idx)
    img, a = got["obs"]["img"].cpu().numpy(), got["actions"].cpu().numpy()
    for b, i in enumerate(idx):
        rows = [r - (R - 4) for r in O.window_rows(int(i), R - 4, R, 2, 3)]
        assert np.array_equal(img[b], last.numpy()[rows]), b
        assert a[b, :, 0].tolist() == [float(r) for r in rows[1:]]
    # and the draw reaches the end of a table this long without leaving it
    d = ds.draw(4096, SEED64, 1).cpu().numpy()
    assert np.array_equal(d, O.draw(SEED64, 1, 0, 4096, [R])[2]) and d.max() < R and d.max() > R // 2


# ---- end to end: the batches feed update ------------------------------------------------------------------------------------------------
def _rm_episodes(lengths, seed):
    data = cfgs.BY_NAME["rm"]
    eps = []
    for i, T in enumerate(lengths):
        b = cfgs.synth_latent_batch(data, 1, T, seed + i, with_actions=True)
        eps.append(dict({k: v[0] for k, v in b["obs"].items()}, actions=b["actions"][0]))
    return eps, list(data["lowdim_obs"]) + list(data["rgb_obs"])


def _params(ag):
    """Host copies of both networks' parameters, taken NOW: a trained state lives in the engine's arenas until the next update supersedes it."""
    return {**{f"planner/{k}": np.array(v) for k, v in ag.planner_state.params.items()},
            **{f"idm/{k}": np.array(v) for k, v in ag.idm_state.params.items()}}


def _same_params(pa, b):
    pb = _params(b)
    assert set(pa) == set(pb)
    bad = [k for k in pa if not np.array_equal(np.asarray(pa[k]), np.asarray(pb[k]))]
    assert not bad, bad[:5]


@pytest.fixture(scope="module")
def rm_setup():
    eps, keys = _rm_episodes([12, 1, 30, 5], 300)
    eps2, _ = _rm_episodes([3, 20], 400)
    ag, _ = make_agent("rm", planner_params(), idm_params())
    yield ag, keys, eps, eps2
    ag._engine.close()


def test_fit_equals_update_on_the_oracle_batches(rm_setup):
    """harness.fit on device batches == agent.update on the oracle's NumPy batches of the same (seed, step): parameters bit for bit."""
    from latent_diffusion_planning_amd import harness
    ag, keys, eps, _ = rm_setup
    ds = D.DeviceDataset.from_episodes(eps, keys, frame_stack=1, seq_length=9)
    logged = []
    fitted, m = harness.fit(ag, ds.batches(16, seed=5), 3, 7, log_every=3, on_log=lambda s, d: logged.append((s, d)))
    got, loss = _params(fitted), float(m["loss"])
    tables, st, en = O.weld(eps, ["actions"] + keys)
    ref = ag
    for step in range(3):
        batch = O.batch(tables, st, en, O.draw(5, step, 0, 16, [len(st)])[2], keys, ["actions"], 1, 9)
        ref, mr = ref.update(batch, 7 + step, step)
    _same_params(got, ref)
    assert fitted.planner_state.step == 3 and loss == float(mr["loss"])
    assert [s for s, _ in logged] == [3] and logged[0][1]["loss"] == loss


def test_fit_with_a_mixed_iterator_equals_update_mixed(rm_setup):
    from latent_diffusion_planning_amd import harness
    ag, keys, eps, eps2 = rm_setup
    ds = D.DeviceDataset.from_episodes(eps, keys, frame_stack=1, seq_length=9)
    ds2 = D.DeviceDataset.from_episodes(eps2, keys, frame_stack=1, seq_length=9)
    mixed = D.DeviceDataset.mix([ds, ds2], 0.25)
    fitted, _ = harness.fit(ag, ds.batches(16, seed=5), 3, 7, mixed_iter=mixed.batches(8, seed=6))
    got = _params(fitted)
    tables, st, en = O.weld(eps, ["actions"] + keys)
    mt, ms, me = O.weld(eps + eps2, ["actions"] + keys)
    ref = ag
    for step in range(3):
        batch = O.batch(tables, st, en, O.draw(5, step, 0, 16, [len(st)])[2], keys, ["actions"], 1, 9)
        mb = O.batch(mt, ms, me, O.draw(6, step, 0, 8, [len(st), len(ms) - len(st)], [0.25, 0.75])[2], keys, ["actions"], 1, 9)
        ref, _ = ref.update_mixed(batch, mb, 7 + step, step)
    _same_params(got, ref)


def test_sample_on_a_side_stream_then_update_on_the_default_stream(rm_setup):
    """The stream contract of DeviceDataset.sample: the outputs belong to the calling stream; a consumer on another stream waits for it."""
    ag, keys, eps, _ = rm_setup
    ds = D.DeviceDataset.from_episodes(eps, keys, frame_stack=1, seq_length=9)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        batch = ds.sample(32, 123, 4)
    done = torch.cuda.Event()
    done.record(side)
    torch.cuda.current_stream().wait_event(done)
    got = _params(ag.update(batch, 11, 0)[0])
    tables, st, en = O.weld(eps, ["actions"] + keys)
    ref, _ = ag.update(O.batch(tables, st, en, O.draw(123, 4, 0, 32, [len(st)])[2], keys, ["actions"], 1, 9), 11, 0)
    _same_params(got, ref)
    torch.cuda.synchronize()


def test_the_data_class_iterator_is_sample_at_the_iteration_count(tmp_path):
    """`train_dataloader()` of a data class: batch n is `train_dataset.sample(batch_size, seed, n)`, on device tensors read from .npz containers."""
    eps = _episodes([3, 9, 1], 51, with_img=False)
    src = {}
    for n, ep in enumerate(eps):
        src[f"data/demo_{n}/actions"] = ep["actions"]
        src[f"data/demo_{n}/obs/k9"], src[f"data/demo_{n}/next_obs/k9"] = ep["k9"], ep["k9"][::-1].copy()
    np.savez(str(tmp_path / "d.npz"), **src)
    data = D.RobomimicLatentData(name="rm", train_path=str(tmp_path / "d.npz"), eval_path=None, train_latent_path=None, eval_latent_path=None,
                                 train_n_episode_overfit=None, eval_n_episode_overfit=None, batch_size=33, n_workers=2, prefetch_factor=2, obs_horizon=2,
                                 seq_length=8, env_params=None, meta=dict(lowdim_obs=["k9", "optimal"], rgb_obs=[], shape_meta={}), seed=9)
    ds = data.train_dataset
    assert ds.total_n_sequences == 3 + 9 + 1 + 3 and ds.device.type == "cuda"
    it = iter(data.train_dataloader())
    for n in range(3):
        got, ref = next(it), ds.sample(33, 9, n)
        assert torch.equal(got["actions"], ref["actions"]) and all(torch.equal(got["obs"][k], ref["obs"][k]) for k in ("k9", "optimal"))
    assert got["obs"]["k9"].shape == (33, 9, 9) and got["actions"].shape == (33, 8, 7) and float(got["obs"]["optimal"].min()) == 1.0
