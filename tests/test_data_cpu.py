"""The training data layer without a GPU: the NumPy oracle (tests/data_oracle.py) against hand-worked windows, the host side of
latent_diffusion_planning_amd/data.py (weld, n_overfit, thresholds, file containers) against the oracle, the draw's range, and the C ABI
(header <-> binding, LDP_EINVAL paths that make no HIP call)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from latent_diffusion_planning_amd import _lib
from latent_diffusion_planning_amd import data as D
from oracle import philox
from tests import data_oracle as O


def _built():
    return os.path.exists(_lib.LIB_PATH)


# ---- the oracle against hand-worked windows -----------------------------------------------------------------------------------------
def test_an_episode_of_one_row_fills_the_whole_window_with_that_row():
    # episodes [0, 3), [3, 4), [4, 9); fs = 2, sl = 8 -> W = 9
    assert O.window_rows(3, 3, 4, 2, 8) == [3] * 9
    assert O.window_rows(3, 3, 4, 2, 8, first=1) == [3] * 8


def test_windows_at_the_first_and_last_row_of_an_episode_clamp_inside_it():
    s, e = 4, 9
    assert O.window_rows(4, s, e, 2, 8) == [4, 4, 5, 6, 7, 8, 8, 8, 8]                # first row: one padded frame in front, tail clamped
    assert O.window_rows(8, s, e, 2, 8) == [7, 8, 8, 8, 8, 8, 8, 8, 8]                # last row: everything after it is the last row
    assert O.window_rows(6, s, e, 4, 4) == [4, 4, 5, 6, 7, 8, 8]                      # fs - 1 = 3 frames back: rows 3 -> 4 (clamped), 4, 5
    assert O.window_rows(6, s, e, 4, 4, first=3) == [6, 7, 8, 8]                      # actions: sl rows from the sample on
    assert O.window_rows(6, s, e, 1, 1) == [6]


def test_a_neighbour_episode_never_leaks_into_a_window():
    lengths = [1, 2, 7, 40]
    starts = np.concatenate([[0], np.cumsum(lengths)])
    for s, e in zip(starts[:-1], starts[1:]):
        for i in range(s, e):
            for fs, sl in ((1, 1), (2, 8), (2, 16), (4, 4)):
                rows = O.window_rows(i, s, e, fs, sl)
                assert len(rows) == fs + sl - 1 and min(rows) >= s and max(rows) < e and rows[fs - 1] == i
                assert all(b - a in (0, 1) for a, b in zip(rows, rows[1:]))


def test_the_oracle_batch_follows_the_reference_padding_rule_on_a_worked_example():
    """Two episodes of 3 and 2 rows, one key whose value is its welded row number: the window of index 3 (first row of episode 2) with
    fs = 2, sl = 3 is [3, 3, 4, 4] (one frame padded in front, one behind) and its actions [3, 4, 4]."""
    eps = [{"x": np.arange(0, 3, dtype=np.float32)[:, None], "actions": np.arange(0, 3, dtype=np.float32)[:, None]},
           {"x": np.arange(3, 5, dtype=np.float32)[:, None], "actions": np.arange(3, 5, dtype=np.float32)[:, None]}]
    tables, st, en = O.weld(eps, ["actions", "x"])
    assert st.tolist() == [0, 0, 0, 3, 3] and en.tolist() == [3, 3, 3, 5, 5]
    b = O.batch(tables, st, en, [3, 2], ["x"], ["actions"], 2, 3)
    assert b["obs"]["x"][0, :, 0].tolist() == [3, 3, 4, 4] and b["actions"][0, :, 0].tolist() == [3, 4, 4]
    assert b["obs"]["x"][1, :, 0].tolist() == [1, 2, 2, 2] and b["actions"][1, :, 0].tolist() == [2, 2, 2]


# ---- weld: files -> tables ---------------------------------------------------------------------------------------------------------
LOW, CAM = "robot0_eef_pos", "agentview_image"


def _file_arrays(n_eps=12, seed=5):
    """A robomimic-shaped file as {dataset path: array}: episode demo_<n> has n % 3 + 1 steps of seeded random values."""
    g = np.random.Generator(np.random.PCG64(seed))
    src, lat = {}, {}
    for n in range(n_eps):
        T = n % 3 + 1
        ep = f"demo_{n}"
        src[f"data/{ep}/actions"] = g.uniform(-1, 1, (T, 7)).astype(np.float32)
        src[f"data/{ep}/obs/{LOW}"] = g.uniform(-1, 1, (T, 3)).astype(np.float32)
        src[f"data/{ep}/next_obs/{LOW}"] = g.uniform(-1, 1, (T, 3)).astype(np.float32)
        src[f"data/{ep}/obs/{CAM}"] = g.integers(0, 256, (T, 4, 4, 3)).astype(np.uint8)
        src[f"data/{ep}/next_obs/{CAM}"] = g.integers(0, 256, (T, 4, 4, 3)).astype(np.uint8)
        lat[f"data/{ep}/latent/{CAM}"] = g.standard_normal((T + 1, 2, 2, 4)).astype(np.float32)
    return src, lat


def _oracle_tables(src, lat, names, obs_keys, optimal, append_last):
    eps = []
    for ep in names:
        T = len(src[f"data/{ep}/actions"])
        latents = {CAM: lat[f"data/{ep}/latent/{CAM}"][: T + 1 if append_last else T]}
        eps.append(O.episode_rows({k: src[f"data/{ep}/obs/{k}"] for k in (LOW, CAM)}, {k: src[f"data/{ep}/next_obs/{k}"] for k in (LOW, CAM)},
                                  src[f"data/{ep}/actions"], latents, obs_keys, optimal, append_last))
    return O.weld(eps, ["actions"] + list(obs_keys), optimal)


OBS_KEYS = [LOW, "optimal", f"latent_{CAM}", CAM]


@pytest.fixture(scope="module")
def npz_files(tmp_path_factory):
    src, lat = _file_arrays()
    d = tmp_path_factory.mktemp("data")
    sp, lp = str(d / "low_dim.npz"), str(d / "latent.npz")
    np.savez(sp, **src)
    from latent_diffusion_planning_amd.preencode import save_latents
    save_latents(lp, lat, {"total": 12, "min_z": -3.0, "max_z": 3.0})
    return src, lat, sp, lp


def _same(ds, ref):
    tables, st, en = ref
    assert ds.total_n_sequences == len(st)
    assert np.array_equal(ds.bounds.numpy(), np.stack([st, en], 1))
    for k, t in tables.items():
        got = ds.tables[k].numpy()
        assert got.dtype == t.dtype and got.shape == t.shape and np.array_equal(got, t), k


def test_weld_sorts_demo_10_after_demo_9_and_appends_the_robomimic_row(npz_files):
    src, lat, sp, lp = npz_files
    names = O.demo_sort([f"demo_{n}" for n in (10, 9, 0, 1, 11, 2, 3, 4, 5, 6, 7, 8)])
    assert names.index("demo_10") == names.index("demo_9") + 1 and names[1] == "demo_1" and names[2] == "demo_2"
    ds = D.DeviceDataset.from_files(sp, lp, OBS_KEYS, frame_stack=2, seq_length=8, device="cpu")
    _same(ds, _oracle_tables(src, lat, names, OBS_KEYS, 1, True))
    assert ds.n_demos == 12 and ds.total_n_sequences == sum(n % 3 + 1 + 1 for n in range(12))
    assert ds.tables[CAM].dtype.is_floating_point is False                         # camera frames stay bytes
    # the last row of an episode: the last next_obs row / the last action again
    assert np.array_equal(ds.tables[LOW].numpy()[1], src[f"data/demo_0/next_obs/{LOW}"][-1])
    assert np.array_equal(ds.tables["actions"].numpy()[1], src["data/demo_0/actions"][-1])


def test_aloha_flavour_has_t_rows_and_nothing_appended(npz_files):
    src, lat, sp, _ = npz_files
    names = O.demo_sort([f"demo_{n}" for n in range(12)])
    keys = [LOW, "optimal", CAM]
    ds = D.DeviceDataset.from_files(sp, None, keys, frame_stack=1, seq_length=4, optimal=0, append_last=False, device="cpu")
    _same(ds, _oracle_tables(src, lat, names, keys, 0, False))
    assert ds.total_n_sequences == sum(n % 3 + 1 for n in range(12)) and float(ds.tables["optimal"].max()) == 0.0


@pytest.mark.parametrize("n_overfit", [3, 12, ["demo_10", "demo_2", "demo_9"]])
def test_n_overfit_is_applied_after_the_sort(npz_files, n_overfit):
    src, lat, sp, lp = npz_files
    names = O.select(O.demo_sort([f"demo_{n}" for n in range(12)]), n_overfit)
    if isinstance(n_overfit, list):
        assert names == ["demo_2", "demo_9", "demo_10"]
    else:
        assert names == [f"demo_{n}" for n in range(n_overfit)]
    ds = D.DeviceDataset.from_files(sp, lp, OBS_KEYS, frame_stack=1, seq_length=2, n_overfit=n_overfit, device="cpu")
    _same(ds, _oracle_tables(src, lat, names, OBS_KEYS, 1, True))
    assert ds.n_demos == len(names)


def test_from_files_round_trip_through_hdf5(tmp_path):
    from latent_diffusion_planning_amd import hdf5_io
    try:
        hdf5_io.load()
    except hdf5_io.HDF5Unavailable as e:
        pytest.skip(str(e))
    src, lat = _file_arrays(n_eps=11)
    sp, lp = str(tmp_path / "image.hdf5"), str(tmp_path / "latent.hdf5")
    with hdf5_io.File(sp, "w") as f:
        for name, a in src.items():
            f.write_dataset(name, a, dtype=a.dtype)
    hdf5_io.write_latent_file(lp, lat, {"total": 11})
    names = O.demo_sort([f"demo_{n}" for n in range(11)])
    ds = D.DeviceDataset.from_files(sp, lp, OBS_KEYS, frame_stack=2, seq_length=8, device="cpu")
    _same(ds, _oracle_tables(src, lat, names, OBS_KEYS, 1, True))
    assert ds.env_meta is None                                                     # no env_args attribute in this file


def test_from_files_without_libhdf5_raises_hdf5_unavailable(tmp_path):
    from latent_diffusion_planning_amd import hdf5_io
    try:
        hdf5_io.load()
    except hdf5_io.HDF5Unavailable:
        with pytest.raises(hdf5_io.HDF5Unavailable):
            D.DeviceDataset.from_files(str(tmp_path / "x.hdf5"), None, [LOW], device="cpu")


def test_mix_welds_the_datasets_one_behind_the_other(npz_files):
    _, _, sp, lp = npz_files
    parts = [D.DeviceDataset.from_files(sp, lp, OBS_KEYS, frame_stack=1, seq_length=2, n_overfit=n, optimal=int(i == 0), device="cpu")
             for i, n in enumerate((2, 5, 3))]
    m = D.DeviceDataset.mix(parts, [0.2, 0.3, 0.5])
    tot = [p.total_n_sequences for p in parts]
    assert m.set_base == [0, tot[0], tot[0] + tot[1]] and m.set_total == tot and m.total_n_sequences == sum(tot)
    assert np.array_equal(m.bounds.numpy()[tot[0]:tot[0] + tot[1]], parts[1].bounds.numpy() + tot[0])
    assert m.tables["optimal"].numpy()[:tot[0]].min() == 1.0 and m.tables["optimal"].numpy()[tot[0]:].max() == 0.0
    with pytest.raises(ValueError):
        D.DeviceDataset.mix(parts, [0.5, 0.5])
    with pytest.raises(ValueError):
        D.DeviceDataset.mix([m, parts[0]], 0.5)


# ---- draw ---------------------------------------------------------------------------------------------------------------------------
def test_draw_thresholds():
    assert O.thresholds(0.25) == [2 ** 30, 2 ** 32] == D.split_thresholds(D._as_split(0.25, 2))
    want = [int(np.floor(0.2 * 2.0 ** 32)), int(np.floor((0.2 + 0.3) * 2.0 ** 32)), 2 ** 32]
    assert want[0] == 858993459 and want[1] == 2 ** 31
    assert O.thresholds([0.2, 0.3, 0.5]) == want == D.split_thresholds([0.2, 0.3, 0.5])
    assert D.split_thresholds([1.0]) == [2 ** 32] == O.thresholds([1.0])
    assert D.split_thresholds([0.5, 0.5, 0.0])[-1] == 2 ** 32                       # the last one is forced, whatever the sum rounds to


@pytest.mark.parametrize("total", [1, 2, 2 ** 31 - 1])
def test_the_draw_stays_inside_the_dataset(total):
    w = philox.words(0xDEADBEEFCAFEF00D, 0, 7, O.STREAM_DATA, 4096)
    _, idx, welded = O.draw(0xDEADBEEFCAFEF00D, 7, 0, 4096, [total])
    assert idx.min() >= 0 and idx.max() < total and np.array_equal(idx, welded)
    assert np.array_equal(idx, (w[:, 0].astype(np.uint64) * np.uint64(total)) >> np.uint64(32))
    if total == 2:
        assert set(idx.tolist()) == {0, 1}
    # the extreme words map to the two ends
    assert (0 * total) >> 32 == 0 and ((2 ** 32 - 1) * total) >> 32 == total - 1


def test_the_mixture_draw_follows_the_split():
    ds, idx, welded = O.draw(3, 0, 0, 8192, [5, 11, 40], [0.2, 0.3, 0.5])
    frac = np.bincount(ds, minlength=3) / 8192.0
    assert np.all(np.abs(frac - [0.2, 0.3, 0.5]) < 4 * np.sqrt(0.25 / 8192))        # four binomial standard deviations at most
    assert np.array_equal(welded, idx + np.asarray([0, 5, 16])[ds]) and idx[ds == 0].max() < 5 and idx[ds == 1].max() < 11
    a = O.draw(3, 0, 0, 8, [5, 11, 40], [0.2, 0.3, 0.5])[2]
    b = O.draw(3, 0, 3, 3, [5, 11, 40], [0.2, 0.3, 0.5])[2]
    assert np.array_equal(a[3:6], b)                                                # keyed by the global row


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_data_entry_points():
    syms = _lib.header_symbols()
    assert "ldp_data_sample" in syms and "ldp_data_draw" in syms and syms == sorted(_lib.SIGNATURES)
    hdr = open(_lib.HEADER_PATH).read()
    assert re.search(r"#define LDP_PHILOX_STREAM_DATA 11u", hdr) and _lib.PHILOX_STREAM_DATA == O.STREAM_DATA == 11
    ids = [int(v) for v in re.findall(r"#define LDP_PHILOX_STREAM_\w+ (\d+)u", hdr)]
    assert len(ids) == len(set(ids))
    assert int(re.search(r"#define LDP_DATA_MAX_KEYS (\d+)", hdr).group(1)) == _lib.DATA_MAX_KEYS == 16
    assert int(re.search(r"#define LDP_DATA_MAX_SETS (\d+)", hdr).group(1)) == _lib.DATA_MAX_SETS == 8
    # ldp_data_key: two pointers, an int64 and two int32
    assert C.sizeof(_lib.LdpDataKey) == 32 and _lib.LdpDataKey.row_bytes.offset == 16 and _lib.LdpDataKey.n_rows.offset == 28


def _call(n_keys=1, row_bytes=36, B=4, fs=2, sl=8, table=0x1000, bounds=0x2000, keys_null=False, total=100, set_total=100, first=0, rows=9):
    """ldp_data_sample with made-up (never dereferenced) device addresses: every case below must fail before any HIP call."""
    lib = _lib.load()
    keys = (_lib.LdpDataKey * max(n_keys, 1))()
    for k in keys:
        k.table, k.out, k.row_bytes, k.first_row, k.n_rows = table, 0x3000, row_bytes, first, rows
    base, tot, thr = (C.c_int64 * 1)(0), (C.c_int64 * 1)(set_total), (C.c_uint64 * 1)(2 ** 32)
    rc = lib.ldp_data_sample(None if keys_null else keys, n_keys, bounds, total, base, tot, thr, 1, 1, 0, 0, B, fs, sl, None, None, None)
    return rc, lib.ldp_last_error().decode()


@pytest.mark.skipif(not _built(), reason="libldp_hip.so not built")
@pytest.mark.parametrize("kw, text", [
    (dict(n_keys=17), "n_keys"), (dict(n_keys=0), "n_keys"), (dict(row_bytes=38), "multiple of 4"), (dict(row_bytes=0), "multiple of 4"),
    (dict(B=0), "B must"), (dict(fs=0), "frame_stack"), (dict(sl=0), "seq_length"), (dict(table=None), "null table"),
    (dict(keys_null=True), "null key table"), (dict(bounds=None), "null key table"), (dict(set_total=2 ** 31, total=2 ** 31 - 1), "2^31"),
    (dict(total=2 ** 31), "total_rows"), (dict(first=1, rows=9), "window rows"), (dict(table=0x1002), "4-byte aligned"),
])
def test_bad_arguments_return_einval_without_a_hip_call(kw, text):
    rc, msg = _call(**kw)
    assert rc == -1 and text in msg, (rc, msg)


@pytest.mark.skipif(not _built(), reason="libldp_hip.so not built")
def test_draw_bad_arguments_return_einval():
    lib = _lib.load()
    base, tot, thr = (C.c_int64 * 1)(0), (C.c_int64 * 1)(10), (C.c_uint64 * 1)(2 ** 32)
    assert lib.ldp_data_draw(base, tot, thr, 1, 1, 0, 0, 0, 0x1000, None) == -1 and b"B must" in lib.ldp_last_error()
    assert lib.ldp_data_draw(base, tot, thr, 1, 1, 0, 0, 4, None, None) == -1
    assert lib.ldp_data_draw(base, tot, thr, 9, 1, 0, 0, 4, 0x1000, None) == -1 and b"n_sets" in lib.ldp_last_error()
    assert lib.ldp_data_draw(None, tot, thr, 1, 1, 0, 0, 4, 0x1000, None) == -1
    tot[0] = 0
    assert lib.ldp_data_draw(base, tot, thr, 1, 1, 0, 0, 4, 0x1000, None) == -1 and b"2^31" in lib.ldp_last_error()


# ---- the data classes (the yaml `_target_`s) ------------------------------------------------------------------------------------------
META = dict(lowdim_obs=[LOW, "optimal"], rgb_obs=[f"latent_{CAM}"], shape_meta=dict(ac_dim=7))


def test_robomimic_and_aloha_classes_take_the_reference_keywords(npz_files):
    src, lat, sp, lp = npz_files
    kw = dict(name="rm_lift_latent_img64_data", train_path=sp, eval_path=sp, train_latent_path=lp, eval_latent_path=lp,
              train_n_episode_overfit=None, eval_n_episode_overfit=10, batch_size=32, n_workers=8, prefetch_factor=2, obs_horizon=2,
              seq_length=8, env_params=dict(env_kwargs={}), meta=META, seed=3, device="cpu")
    rm = D.RobomimicLatentData(**kw)
    keys = META["lowdim_obs"] + META["rgb_obs"]
    names = O.demo_sort([f"demo_{n}" for n in range(12)])
    _same(rm.train_dataset, _oracle_tables(src, lat, names, keys, 1, True))
    _same(rm.val_dataset, _oracle_tables(src, lat, names[:10], keys, 1, True))
    assert rm.train_dataset is rm.train_dataset and rm.shape_meta == META["shape_meta"] and rm.env_params == dict(env_kwargs={})
    it = rm.train_dataloader()
    assert it.dataset is rm.train_dataset and (it.batch_size, it.seed, it.step) == (32, 3, 0) and iter(it) is it
    assert (rm.train_dataset.frame_stack, rm.train_dataset.seq_length) == (2, 8)
    al = D.ALOHASimLatentData(**dict(kw, meta=dict(META, rgb_obs=[]), hdf5_use_swmr=True))
    _same(al.train_dataset, _oracle_tables(src, lat, names, META["lowdim_obs"], 1, False))


def test_mixed_class_marks_the_first_dataset_optimal_and_takes_a_float_split(npz_files):
    src, lat, sp, lp = npz_files
    mx = D.RobomimicMixedLatentData(name="rm_mixed", train_paths=[sp, sp], eval_paths=[], train_latent_paths=[lp, lp], eval_latent_paths=[],
                                    batch_size=16, n_workers=4, prefetch_factor=2, train_n_episode_overfit=[3, 5], eval_n_episode_overfit=[],
                                    train_split=0.25, eval_split=0.5, obs_horizon=1, seq_length=4, env_params=None, meta=META, device="cpu")
    ds = mx.train_dataset
    n0 = sum(n % 3 + 2 for n in range(3))
    assert ds.split == [0.25, 0.75] and ds.set_base == [0, n0] and ds.set_total == [n0, sum(n % 3 + 2 for n in range(5))]
    opt = ds.tables["optimal"].numpy()[:, 0]
    assert opt[:n0].tolist() == [1.0] * n0 and not opt[n0:].any()
    val = mx.val_dataset                                                            # no eval paths: the first train file, ten episodes, optimal 0
    assert val.n_demos == 10 and not val.tables["optimal"].numpy().any()
    with pytest.raises(ValueError):
        D.RobomimicMixedLatentData(name="x", train_paths=[sp, sp], eval_paths=[], train_latent_paths=[lp, lp], eval_latent_paths=[], batch_size=4,
                                   train_n_episode_overfit=[3], train_split=0.5, meta=META, device="cpu")


# ---- harness.fit: the loop's bookkeeping, on a stub agent ------------------------------------------------------------------------------
class _Stub:
    def __init__(self, log):
        self.log = log

    def update(self, batch, rng, step):
        self.log.append(("update", batch, None, rng, step))
        return self, {"loss": np.float32(step), "plan": np.zeros(3)}

    def update_mixed(self, batch, mixed, rng, step):
        self.log.append(("mixed", batch, mixed, rng, step))
        return self, {"loss": np.float32(-step)}


def test_fit_steps_seeds_and_log_cadence():
    from latent_diffusion_planning_amd import harness
    calls, logged = [], []
    ag, m = harness.fit(_Stub(calls), iter(range(100, 200)), 5, 40, log_every=2, on_log=lambda s, d: logged.append((s, d)))
    assert [(c[0], c[1], c[3], c[4]) for c in calls] == [("update", 100 + i, 40 + i, i) for i in range(5)]
    assert logged == [(2, {"loss": 1.0}), (4, {"loss": 3.0})] and float(m["loss"]) == 4.0         # scalars only; the host looks at log steps alone
    calls.clear()
    harness.fit(_Stub(calls), iter(range(100, 200)), 3, np.array([0, 7], np.uint32), mixed_iter=iter(range(500, 600)), start_step=10)
    assert [(c[0], c[1], c[2], c[3], c[4]) for c in calls] == [("mixed", 100 + i, 500 + i, 17 + i, 10 + i) for i in range(3)]
