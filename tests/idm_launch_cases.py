"""Cases, inputs, the expected-dispatch rule and the coverage table of tests/test_hip_idm_launches.py (importable without a GPU:
tests/test_idm_launches_cpu.py uses the same functions and tables).

The fused IDM block (csrc/idm.hip) exists in 14 instantiations -- idm_block_kernel<HS, RINGED, STREAM> (12) and idm_block_h16_kernel<HS> (2) --
and every one is reached at <= 250 rows through the public options; the handle counts each enqueued launch per instantiation (read-only
options stat_idm_*), so a case states which counter it must move."""
import numpy as np
import torch

from tests.planner_stage_cases import ref_rows, stage_error      # noqa: F401  (the row rule and the tolerance rule are the planner suite's)
from tests.util import rng

NB = 3                                       # MLPResNet blocks (idm_blocks)
AP = 32                                      # padded action columns: the Philox element stride of a row
# name -> (obs_dim, action_dim, heavy weights).  aloha: A > 8 is a second pass of the tail's eight dot-product chains
CONFIGS = {"rm": (25, 7, False), "aloha": (30, 14, False), "rmh": (25, 7, True)}

# every IDM option a case may set, with its default (Options, csrc/engine.hpp)
DEFAULTS = dict(idm_hs=0, idm_stream=-1, idm_noring=0, idm_rt_major=1, idm_f16=1, idm_f16_min_rows=1040, idm_f16_hs=0, idm_unfused=0)

F32_COUNTERS = tuple(f"stat_idm_f32_hs{hs}{ring}{nt}" for hs in (1, 2, 4, 8) for ring in (("", "_ring") if hs >= 4 else ("",)) for nt in ("", "_nt"))
F16_COUNTERS = ("stat_idm_f16_hs2", "stat_idm_f16_hs4")
COUNTERS = F32_COUNTERS + F16_COUNTERS + ("stat_idm_unfused",)


def case(config, R, **opts):
    assert config in CONFIGS and all(k in DEFAULTS for k in opts)
    return (config, R, tuple(sorted(opts.items())))


def case_id(c):
    return f"{c[0]}-R{c[1]}" + "".join(f"-{k[4:]}={v}" for k, v in c[2])


F16 = dict(idm_f16_min_rows=32, idm_hs=0)

# ---- rm: every instantiation, every partial-access mode -------------------------------------------------------------------------------------
PLAIN_CASES = [case("rm", R, idm_hs=hs, idm_stream=st) for hs in (1, 2, 4, 8) for st in (0, 1, 2) for R in (17, 37)]
# 16 row tiles, the last with 10 rows, and 16 HS work-groups <= n_cu: one work-group per CU, the ringed variant
RINGED_CASES = [case("rm", 250, idm_hs=hs, idm_stream=st) for hs in (4, 8) for st in (0, 2)]
# 32-row tiles, ragged and exact
F16_CASES = [case("rm", R, idm_f16_hs=fh, idm_stream=st, **F16) for fh in (0, 2) for st in (0, 2) for R in (33, 64, 250)]
DEFAULT_CASES = [case("rm", R) for R in (1, 16, 17, 37, 250, 1024)]
UNFUSED_CASES = [case("rm", 37, idm_unfused=1)]
# ---- aloha: a plain, a ringed and an fp16 case of each streaming mode, the default rule, the unfused path --------------------------------
ALOHA_CASES = [case("aloha", 37, idm_hs=2, idm_stream=1), case("aloha", 17, idm_hs=1, idm_stream=2), case("aloha", 250, idm_hs=8, idm_stream=0),
               case("aloha", 250, idm_hs=4, idm_stream=2), case("aloha", 33, idm_stream=0, **F16), case("aloha", 250, idm_f16_hs=2, idm_stream=2, **F16),
               case("aloha", 16), case("aloha", 1024), case("aloha", 37, idm_unfused=1)]
# ---- the trained-like weight set (tests.util.idm_params_heavy: hidden activations ~5e3) ---------------------------------------------------
HEAVY_CASES = [case("rmh", 37, idm_hs=4, idm_stream=0), case("rmh", 64, idm_stream=0, **F16)]

CASES = PLAIN_CASES + RINGED_CASES + F16_CASES + DEFAULT_CASES + UNFUSED_CASES + ALOHA_CASES + HEAVY_CASES
# DDPM-100 with explicit step noise, and the in-kernel Philox noise: one plain, one ringed, one fp16 case per config
DDPM_CASES = [case("rm", 37, idm_hs=2, idm_stream=1), case("rm", 250, idm_hs=8, idm_stream=0), case("rm", 33, idm_stream=2, **F16),
              case("aloha", 37, idm_hs=2, idm_stream=1), case("aloha", 250, idm_hs=4, idm_stream=2), case("aloha", 33, idm_stream=0, **F16)]
# rows 0 .. R_small - 1 of the large call == the small call, bit for bit: (config, large R, small R, options)
SUBBATCH = [("rm", 250, 37, dict(idm_hs=4)), ("rm", 250, 37, dict(idm_hs=1, idm_stream=1)), ("rm", 250, 64, dict(F16)),
            ("aloha", 250, 37, dict(idm_hs=8)), ("aloha", 250, 64, dict(F16))]
# a small call after a large one runs with the grown workspace's stride (Rp = ws_R): (config, options) at R = 37 around an R = 300 call
STRIDE = [("rm", dict(idm_hs=2, idm_stream=0)), ("rm", dict(F16, idm_stream=0))]
# placement only (XCD affinity by hidden slice instead of by row tile), once per kernel family at R = 250
PLACEMENT = [case("rm", 250, idm_hs=2), case("rm", 250, idm_hs=8), case("rm", 250, **F16)]
# what a handle runs at large batches after a range fault: the 16-row kernel chosen by the default rule, streaming by the row count
FALLBACK = [case("rm", 2048, idm_f16=0), case("rm", 4096, idm_f16=0)]

DDIM_STEPS = (1, 2, 5)                      # both parities of the state ping-pong, and the loop of one step (no fused scheduler update)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def inputs(config, R, first=0, seed=0, steps=0):
    """s (R, 2 D), a (R, A), timesteps (R,) and step noise (steps, R, A).  Row n depends on (seed, first + n) only.  s is uniform [-1, 1]; a is
    of kind (first + n) % 3: 0 N(0, 1) (a_T-like), 1 uniform [-1, 1] (a late-step action), 2 within 1e-3 of the +-1 clip; the timestep is per
    row, row 0 at 0 and row 1 at 99; the step noise is N(0, 1)."""
    D, A = CONFIGS[config][:2]
    s, a, k = np.empty((R, 2 * D), np.float32), np.empty((R, A), np.float32), np.empty(R, np.int32)
    nz = np.empty((steps, R, A), np.float32)
    for n in range(R):
        r = first + n
        g = rng(700_000 + 10_007 * seed + r)
        s[n] = g.uniform(-1, 1, 2 * D)
        if r % 3 == 0:
            a[n] = g.standard_normal(A)
        elif r % 3 == 1:
            a[n] = g.uniform(-1, 1, A)
        else:
            a[n] = np.where(g.integers(0, 2, A) == 1, 1.0, -1.0) * (1.0 + 1e-3 * g.uniform(-1, 1, A))
        k[n] = 0 if r == 0 else 99 if r == 1 else int(g.integers(0, 100))
        if steps:
            nz[:, n] = rng(800_000 + 10_007 * seed + r).standard_normal((steps, A))
    return torch.tensor(s), torch.tensor(a), torch.tensor(k), torch.tensor(nz)


# ---- the dispatch rule (csrc/idm.hip: idm_hidden_split, FusedSeq::launch, FusedSeq::base, idm_f16_at), restated ------------------------------
def loop_rows(R, explicit_noise=False):
    """Rows a sampling loop is launched over (engine.hpp bucket_rows): whole 16-row tiles, unless explicit step noise fixes the stride."""
    return R if explicit_noise else (R + 15) // 16 * 16


def hidden_split(R, opts, n_cu=256):
    """Hidden slices per row tile of the fp32 kernel: the forced value, else eight while the grid is one round of one work-group per CU,
    else the split with the cheapest staircase in the number of rounds the grid needs (prices in ms per loop; float32 like the host's)."""
    o = dict(DEFAULTS, **opts)
    if o["idm_hs"]:
        return o["idm_hs"]
    nrt, cu = (R + 15) // 16, n_cu if n_cu > 0 else 256
    if nrt * 8 <= cu:
        return 8
    r1, r2, r4 = ((nrt * hs + cu - 1) // cu for hs in (1, 2, 4))
    f = np.float32
    c1 = f(3.7) + f(12.6) * f(r1)
    c2 = f(9.3) if r2 == 1 else f(14.0) + f(6.7) * f(r2 - 2)
    c4 = f(5.1) if r4 == 1 else f(8.5) + f(4.1) * f(r4 - 2)
    if c1 <= c2 and c1 <= c4:
        return 1
    return 2 if c2 <= c4 else 4


def f16_at(R, opts, range_fallback=False):
    """The 32-row kernel on fp16 planes: from idm_f16_min_rows rows, unless the handle fell back to the fp32 range, the split is forced or the
    path is the unfused one (weights that do not fit the planes aside: none of the suite's sets)."""
    o = dict(DEFAULTS, **opts)
    return bool(o["idm_f16"] and not range_fallback and not o["idm_hs"] and not o["idm_unfused"] and R >= o["idm_f16_min_rows"])


def stream_parts(R, opts, range_fallback=False):
    """Access mode of the K-partials: 0 plain, 1 non-temporal chosen at run time, 2 the instantiation with the non-temporal path only; by
    default 2 from 128 row tiles."""
    o = dict(DEFAULTS, **opts)
    nrt = (R + 31) // 32 if f16_at(R, opts, range_fallback) else (R + 15) // 16
    return (2 if nrt >= 128 else 0) if o["idm_stream"] < 0 else o["idm_stream"]


def expected_kernel(R, opts, n_cu=256, range_fallback=False):
    """The counter that a call launched over R rows moves."""
    o = dict(DEFAULTS, **opts)
    if o["idm_unfused"]:
        return "stat_idm_unfused"
    if f16_at(R, opts, range_fallback):
        return f"stat_idm_f16_hs{o['idm_f16_hs'] if o['idm_f16_hs'] in (2, 4) else 4}"
    hs, nrt = hidden_split(R, opts, n_cu), (R + 15) // 16
    ringed = hs >= 4 and nrt * hs <= n_cu and nrt >= 16 and not o["idm_noring"]
    return f"stat_idm_f32_hs{hs}" + ("_ring" if ringed else "") + ("_nt" if stream_parts(R, opts, range_fallback) == 2 else "")


# ---- what a call launches (FusedSeq::blocks / tail), as prologue flag sets -------------------------------------------------------------------
def launch_flags(kind, n_steps=0):
    """The prologue flags of every fused launch of one call, in order: kind 'forward' (one evaluation) or 'sample' (a loop of n_steps)."""
    ev = [("IF_BLOCK", "IF_IN")] + [("IF_BLOCK", "IF_RED")] * (NB - 1)
    if kind == "forward":
        return ev + [("IF_TAIL", "IF_EPSOUT")]
    out = []
    for i in range(n_steps):
        out += ev if i == 0 else [("IF_BLOCK", "IF_IN", "IF_TAIL", "IF_STEP")] + ev[1:]
    return out + [("IF_TAIL", "IF_STEP")]


def expected_counts(kind, R, opts, n_cu=256, range_fallback=False, n_steps=0, explicit_noise=False):
    """{counter: launches} one eager call moves: NB + 1 for an evaluation, NB n_steps + 1 for a loop; the unfused path counts its calls (one per
    evaluation)."""
    rows = R if kind == "forward" else loop_rows(R, explicit_noise)
    name = expected_kernel(rows, opts, n_cu, range_fallback)
    if name == "stat_idm_unfused":
        return {name: 1 if kind == "forward" else n_steps}
    return {name: len(launch_flags(kind, n_steps))}


# every test of tests/test_hip_idm_launches.py -> the calls it makes per case: (kind, n_steps)
COVERAGE = {
    "test_one_evaluation": (CASES + FALLBACK, [("forward", 0)]),
    "test_ddim_loops": (CASES, [("sample", n) for n in DDIM_STEPS]),
    "test_ddpm_loop_with_explicit_noise": (DDPM_CASES, [("sample", 100)]),
    "test_philox_key_of_the_in_kernel_noise": (DDPM_CASES, [("sample", 100)]),
}
