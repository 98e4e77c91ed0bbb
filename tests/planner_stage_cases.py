"""Cases, inputs, the checking rule and the coverage table of tests/test_hip_planner_stages.py (importable without a GPU: the CPU tests
tests/test_planner_stages_cpu.py and tests/test_planner_stage_coverage.py use the same functions and tables)."""
import re
from pathlib import Path

import numpy as np
import torch

from tests.util import rng

HIER_IDM_DOWN = (256, 512)
DIMS = (256, 512, 1024)

# name -> (obs_dim, global_cond_dim, pred_horizon, down_dims, heavy weights)
MODELS = {
    "t8": (25, 25, 8, DIMS, False),            # rm_lift / rm_can / rm_square
    "t8h": (25, 25, 8, DIMS, True),            # ... on tests.util.planner_params_heavy() (activations ~5e3)
    "t16": (25, 25, 16, DIMS, False),          # rm_square at pred_horizon 16
    "d30": (30, 30, 8, DIMS, False),           # aloha: obs_dim 30
    "g50": (25, 50, 8, DIMS, False),           # obs_horizon 2
    "d40": (40, 40, 8, DIMS, False),           # 33 .. 64 observation channels: the first conv reads a 64-channel chunk
    "dp": (7, 1033, 16, DIMS, False),          # DPAgent: actions, conditioned on the ResNet features of two frames
    "dpvae": (7, 32, 16, DIMS, False),         # DPVAEAgent: actions, conditioned on two 16-dim latents
    "hier": (7, 50, 4, HIER_IDM_DOWN, False),  # LDPHierAgent's IDM: a two-level U-Net over 4 action positions
}

# every planner option a case may set, with its default (Options, csrc/engine.hpp)
DEFAULTS = dict(no_csplit=0, no_kw=0, no_mb2=0, safe_mode=0, t2_mb2=0, planner_split=1, planner_split_f16=1, planner_split_cs2=1,
                planner_split_8w=1, planner_split_mb2=1, planner_split_t2res=1, planner_split_t2res16=1, planner_split_t2all16=1,
                planner_split_updown=1, planner_split_c256=1, planner_split_t16=1, no_fin_rows=0, up_full_depth=0, by_sample=2, place2d=0,
                kw_min_it=1, kw_bmax=128)


def case(model, B, **opts):
    assert model in MODELS and all(k in DEFAULTS for k in opts)
    return (model, B, tuple(sorted(opts.items())))


def case_id(c):
    return f"{c[0]}-B{c[1]}" + "".join(f"-{k}={v}" for k, v in c[2])


BF16, F32 = dict(planner_split_f16=0), dict(planner_split=0)

# ---- the batch sizes of every model, each B > 256 also on three bf16 planes and on the exact-fp32 kernels ------------------------------
BASE_CASES = ([case("t8", B) for B in (5, 64, 128, 200, 256, 300, 400, 512, 600, 1043)]
              + [case("t16", B) for B in (5, 64, 300, 1043)]
              + [case("d30", 300), case("g50", 300), case("d40", 5), case("dp", 300), case("dpvae", 64)]
              + [case("hier", B) for B in (5, 300, 1030)]
              + [case("t8h", B) for B in (5, 300, 1043)])
FORM_CASES = [case(m, B, **o) for m, B, _ in BASE_CASES if B > 256 and m != "t8h" for o in (BF16, F32)]
# planner_split = 2 (tests): split operands at any batch whose plan has no column / K split -- at 200 plans the groups are halved, so nothing
# moves unless the column split is off too
FORM_CASES += [case("t8", 200, planner_split=2, no_kw=1), case("t8", 200, planner_split=2, no_csplit=1),
               case("t8", 64, planner_split=2, no_csplit=1, no_kw=1, planner_split_f16=0)]

# ---- every option that changes a plan, at a batch where it does: (option, value, model, B, the options it is toggled on top of) ----------
OPTION_CASES = [
    ("no_csplit", 1, "t8", 200, {}), ("no_kw", 1, "t8", 64, {}), ("no_mb2", 1, "t8", 1043, F32), ("safe_mode", 1, "t8", 64, {}),
    ("t2_mb2", 1, "t8", 200, {}), ("planner_split_cs2", 0, "t8", 400, {}), ("planner_split_cs2", 0, "t8", 400, dict(planner_split_t2res16=0)),
    ("planner_split_8w", 0, "t8", 300, {}), ("planner_split_8w", 0, "t16", 300, {}), ("planner_split_8w", 0, "t8", 1043, {}),
    ("planner_split_mb2", 0, "t16", 1043, {}), ("planner_split_t2res", 0, "t8", 1043, {}), ("planner_split_t2res16", 0, "t8", 400, {}),
    ("planner_split_t2all16", 0, "t8", 400, {}), ("planner_split_updown", 0, "t8", 300, {}), ("planner_split_c256", 0, "t8", 300, {}),
    ("planner_split_t16", 0, "t16", 300, {}), ("no_fin_rows", 1, "t8", 64, {}), ("no_fin_rows", 1, "t8", 300, {}), ("no_fin_rows", 1, "t16", 64, {}),
    ("no_fin_rows", 1, "hier", 5, {}), ("up_full_depth", 1, "t8", 200, {}), ("kw_bmax", 32, "t8", 64, {}), ("kw_min_it", 4, "t8", 5, {}),
]
# the stages an option is about, as a predicate on the stage's row WITHOUT the option (plan = mode, to, nwn, ks, cpi, res, mb, kws, split);
# exact: those and no others change plan; else: a non-empty subset of them
ABOUT = {
    "no_csplit": (lambda r: r["cs"] > 1, True), "no_kw": (lambda r: r["kw"] > 1, True), "safe_mode": (lambda r: r["cs"] > 1 or r["kw"] > 1, True),
    "no_mb2": (lambda r: r["plan"][6] == 2 and r["plan"][8] == 0, True),
    "t2_mb2": (lambda r: r["plan"][:2] == (K5_MODE, 2) and r["t"].shape[2] == 1024 and r["plan"][5] == 0, True),
    "planner_split_cs2": (lambda r: r["tile"] == 33, True),
    "planner_split_8w": (lambda r: r["plan"][8] == 3 and r["tile"] in (16, 17, 32), False),
    "planner_split_mb2": (lambda r: r["plan"][6] == 2 and r["plan"][1] == 4 and r["plan"][8] in (2, 3), True),
    "planner_split_t2res": (lambda r: r["tile"] == 32 and r["plan"][5] == 1, True),
    "planner_split_t2res16": (lambda r: r["tile"] == 34, True), "planner_split_t2all16": (lambda r: r["tile"] == 34 and r["plan"][5] == 0, True),
    "planner_split_updown": (lambda r: r["tile"] == 17, True), "planner_split_c256": (lambda r: r["tile"] == 16 and r["t"].shape[2] == 256, True),
    "planner_split_t16": (lambda r: r["tile"] == 16 and r["plan"][1] == 16, True), "no_fin_rows": (lambda r: r["kind"] == "head", True),
    "up_full_depth": (lambda r: r["kind"] == "up", True), "kw_bmax": (lambda r: r["kw"] > 1, True), "kw_min_it": (lambda r: r["kw"] > 1, False),
}
K5_MODE = 0
# options that move work-groups over the chip and nothing else: every tap equals the default's bit for bit
BITWISE_OPTIONS = [("by_sample", 0, "t8", 300), ("by_sample", 1000, "t8", 300), ("place2d", 1, "t8", 300), ("by_sample", 0, "t8", 200)]
# rows traced inside a batch == the same rows traced as their own batch of the same regime (257 .. 512 | 513 .. 992 | >= 993 plans):
# (model, B, first row of the sub-batch, which runs to the batch's end)
SUBBATCH = [("t8", 400, 90), ("t8", 600, 59), ("t8", 1043, 37)]


def all_cases():
    out = (list(BASE_CASES) + list(FORM_CASES) + [case(m, B, **dict(base, **{o: v})) for o, v, m, B, base in OPTION_CASES]
           + [case(m, B, **base) for o, v, m, B, base in OPTION_CASES])
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def inputs(model, B, first=0, seed=0):
    """x (B, T, D), timesteps (B,), cond (B, G).  Row n depends on (seed, first + n) only and is of kind (first + n) % 3: 0 an N(0, 1) state
    (x_T-like), 1 a uniform [-1, 1] state (a clipped late-step plan), 2 a state constant over time plus 1e-3 noise.  Conditions are uniform
    [-1, 1]; the timestep is per row, row 0 at 0 and row 1 at 99."""
    D, G, T = MODELS[model][:3]
    x, k, cond = np.empty((B, T, D), np.float32), np.empty(B, np.int32), np.empty((B, G), np.float32)
    for n in range(B):
        r = first + n
        g = rng(900_000 + 10_007 * seed + r)
        if r % 3 == 0:
            x[n] = g.standard_normal((T, D))
        elif r % 3 == 1:
            x[n] = g.uniform(-1, 1, (T, D))
        else:
            x[n] = g.uniform(-1, 1, (1, D)) + 1e-3 * g.standard_normal((T, D))
        cond[n] = g.uniform(-1, 1, G)
        k[n] = 0 if r == 0 else 99 if r == 1 else int(g.integers(0, 100))
    return torch.tensor(x), torch.tensor(k), torch.tensor(cond)


def ref_rows(B, seed=0):
    """The rows the float64 / float32 reference is computed for (samples never couple: GroupNorm is per sample): every row up to 48 plans,
    else rows 0, 15, 16, 31, 32, every row of the last (ragged) 16-row block, the first row of the last 32-row block and one seeded row of
    each eighth of the batch -- at most 48."""
    if B <= 48:
        return list(range(B))
    rows = {0, 15, 16, 31, 32, (B - 1) // 32 * 32} | set(range((B - 1) // 16 * 16, B))
    g = rng(31_000 + 7 * seed + B)
    for e in range(8):
        lo, hi = e * B // 8, (e + 1) * B // 8
        rows.add(int(g.integers(lo, hi)))
    rows = sorted(rows)
    assert len(rows) <= 48
    return rows


# ---- the rule --------------------------------------------------------------------------------------------------
FLOOR, FACTOR = 1e-5, 3.0


def stage_error(got, ref64, ref32):
    """|got - ref64| <= max(1e-5, 3 err32) max(1, max|ref64|) with err32 the error of the float32 evaluation of the same function on the same
    input.  All three (rows, ...).  -> dict(err, err32, bound, ok, row): errors relative to max(1, max|ref64|), `row` the row of the largest."""
    got, ref64, ref32 = (torch.as_tensor(t).double() for t in (got, ref64, ref32))
    assert got.shape == ref64.shape == ref32.shape, (got.shape, ref64.shape, ref32.shape)
    scale = max(1.0, float(ref64.abs().max()))
    d = (got - ref64).abs()
    err, err32 = float(d.max()) / scale, float((ref32 - ref64).abs().max()) / scale
    bound = max(FLOOR, FACTOR * err32)
    return dict(err=err, err32=err32, bound=bound, ok=bool(np.isfinite(err) and err <= bound), row=int(d.flatten(1).max(1).values.argmax()))


# ---- the regime rule, per stage -------------------------------------------------------------------------
# shapes (mode, positions, columns per work-group) that have a tile over a QUARTER / a HALF of a GroupNorm group; a conv asked for a narrower
# part than its shape has takes the next wider one
K5, DOWN, UP, P1 = 0, 1, 2, 3
QUARTER = {(K5, 2, 32), (K5, 4, 16), (K5, 8, 16), (K5, 4, 32)}
HALF = {(K5, 8, 16), (K5, 4, 32), (K5, 2, 64), (K5, 4, 16), (K5, 2, 32), (K5, 8, 32), (K5, 4, 64), (K5, 16, 16), (DOWN, 4, 16), (DOWN, 2, 32), (DOWN, 8, 16),
        (UP, 4, 32), (UP, 8, 16), (UP, 16, 16), (P1, 8, 16)}
# 16-row split tiles of the stride-2 / transposed convs: (mode, positions, group width)
UPDOWN16 = {(DOWN, 4, 32), (DOWN, 4, 64), (DOWN, 2, 64), (UP, 4, 64), (UP, 8, 32), (UP, 8, 64), (UP, 16, 32)}
# tiles that carry the K split over work-groups: (mode, positions, nwn, ks, cpi)
KSPLIT_TILES = {(K5, 8, 1, 8, 1), (K5, 2, 2, 4, 2), (K5, 4, 1, 8, 1), (K5, 4, 2, 4, 2), (K5, 4, 2, 4, 1), (DOWN, 4, 4, 2, 1), (UP, 8, 4, 2, 2),
                (DOWN, 4, 1, 8, 1), (DOWN, 2, 2, 4, 2), (UP, 4, 2, 4, 2), (UP, 8, 1, 8, 1)}
FORMS = {0: "f32", 1: "bf16", 2: "bf16", 3: "f16", 4: "f16"}


def expected_dispatch(row, B, opts, ncu=256):
    """(form, mb, cs, K split?) of one conv stage as the documents state the regimes:

    * cs -- work-groups per GroupNorm group: 4 while 4 x 8 x ceil(B / 16) work-groups are co-resident (B <= 128 on 256 CUs), 2 while 2 x 8 x
      ceil(B / 16) are (B <= 256), else 1; always 1 under no_csplit and in safe mode; a shape without a tile that narrow takes the next wider.
    * K split over work-groups: up to 128 plans (kw_bmax), never under no_kw / safe mode, on the tiles that carry it, while twice the grid
      still fits the chip and the K iterations halve into at least kw_min_it per work-group.
    * up to 256 plans every layer is exact fp32 (planner_split = 2, tests: split operands wherever the plan has no column / K split).
    * above 256 plans the k = 5 convs of the 256- / 512- / 1024-channel levels that read a >= 64-channel tensor (all but the first conv), the
      stride-2 and the transposed convs run on split operands: two fp16 planes (planner_split_f16, no range fallback), else three bf16 planes.
      T = 8 / 4 (and T = 16 at 256 channels without the projection, fp16 only): 16-row tiles, one row block -- the 1024-channel T = 4 layers
      without the projection two row blocks from 993 plans.  T = 2 (512 / 1024 channels): from 993 plans 32-row tiles (two row blocks; with
      the projection on fp16 planes: the 16-row instruction over two row blocks); 257 .. 992 plans: 16-row fp16 tiles over whole groups, one
      row block (planner_split_t2res16 / _t2all16), else between 353 and 512 plans the 32-row tile over half groups (cs = 2), else exact fp32.
    * exact-fp32 k = 5 tiles at T = 2, and at T = 4 without the projection, take two row blocks from 993 plans (no_mb2: never)."""
    o = dict(DEFAULTS, **opts)
    mode, to, res = row["plan"][0], row["t"].shape[1] if row["kind"] != "head" else row["plan"][1], row["plan"][5]
    cout = row["t"].shape[2] if row["kind"] != "head" else 32 * ((row["channels"] + 31) // 32)
    cin = row["ca"] + max(row["cb"], 0)
    gw = cout // 8 if cout >= 256 else 32
    nsb, nsb32 = (B + 15) // 16, (B + 31) // 32
    no_split = bool(o["no_csplit"] or o["safe_mode"])
    cs_want = 1 if no_split else 4 if nsb * 32 <= ncu else 2 if nsb * 16 <= ncu else 1
    mb_want = 2 if (not o["no_mb2"] and cs_want == 1 and nsb32 * 8 >= ncu) else 1
    no_kw = bool(o["no_kw"] or o["safe_mode"])
    f16 = bool(o["planner_split_f16"])
    if row["kind"] == "head":
        by_rows = not o["no_fin_rows"]
        cs = 1 if by_rows else cs_want
        cs = 2 if cs >= 2 and (P1, to, gw // 2) in HALF else 1
        return "f32", 1, cs, False
    cs = cs_want
    if cs == 4 and (mode, to, gw // 4) not in QUARTER:
        cs = 2
    if cs == 2 and (mode, to, gw // 2) not in HALF:
        cs = 1
    first = row["kind"] == "res1" and row["block"] == 0
    if o["t2_mb2"] and mode == K5 and to == 2 and cout == 1024 and not res and cs == 2 and 128 < B <= 256:
        return "f32", 2, 4, False
    regime = B > 256 or (o["planner_split"] >= 2 and (B > o["kw_bmax"] or no_kw))
    form, mb = "f32", 1
    sp = "f16" if f16 else "bf16"
    if o["planner_split"] and regime and mode == K5 and not first and cs == 1 and cout % 256 == 0 and cin % 64 == 0:
        if to == 2 and cout % 512 == 0:
            if nsb32 * 8 >= ncu or o["planner_split"] >= 2:                    # 32-row tiles
                form, mb = (sp, 2) if (not res or (o["planner_split_t2res"] and f16)) else ("bf16", 2)
            else:
                cs2 = bool(o["planner_split_cs2"] and not no_split and 2 * nsb32 * 8 <= ncu and 8 * nsb32 * 8 >= 3 * ncu)
                whole16 = bool(o["planner_split_t2res16"] and o["planner_split_t2all16"] and f16)
                if (cs2 or whole16) and f16 and o["planner_split_t2res16"] and (res or o["planner_split_t2all16"]):
                    form, mb = "f16", 1                                         # 16-row tiles over whole groups
                elif cs2:
                    form, mb, cs = ("bf16" if res else sp), 2, 2               # 32-row tiles over half groups
        elif to in (4, 8) and (cout > 256 or o["planner_split_c256"]):
            form = sp
            if to == 4 and gw == 128 and o["planner_split_mb2"] and nsb32 * 8 >= ncu and not (res and f16):
                mb = 2
            if to == 8 and gw == 128:
                form = "bf16"
        elif to == 16 and cout == 256 and not res and f16 and o["planner_split_t16"] and o["planner_split_c256"]:
            form = "f16"
    if o["planner_split"] and o["planner_split_updown"] and regime and mode in (DOWN, UP) and cs == 1 and (mode, to, gw) in UPDOWN16:
        form = sp
    if form == "f32" and mode == K5 and mb_want == 2 and ((to == 4 and not res and gw in (64, 32)) or (to == 2 and gw in (128, 64))):
        mb = 2
    plan = row["plan"]
    nit = cin // (16 * plan[3] * plan[4]) if form == "f32" else 0
    ksplit = (form == "f32" and not no_kw and B <= o["kw_bmax"] and tuple(plan[:5]) in KSPLIT_TILES and mb == 1
              and nsb * (cout // (16 * plan[2])) * 2 <= min(ncu, 256) and nit % 2 == 0 and nit // 2 >= max(1, o["kw_min_it"]))
    return form, mb, cs, ksplit


def dispatch_of(row):
    return FORMS[row["plan"][8]], row["plan"][6], row["cs"], row["kw"] > 1


# ---- instantiations ----------------------------------------------------------------------------------------------------------------------
MODES = {"K5": 0, "DOWN": 1, "UP": 2, "P1": 3}
CSRC = Path(__file__).resolve().parent.parent / "latent_diffusion_planning_amd" / "csrc"


# the launcher macro a list is expanded with (csrc/tconv_inst.hpp) -> (mb, kws, split); mb None: the row's seventh argument
CASE_MACROS = {"LDP_CASE": (1, 0, 0), "LDP_CASE2": (2, 0, 0), "LDP_CASE3": (1, 1, 0), "LDP_CASE_S": (2, 0, 1), "LDP_CASE_S1": (1, 0, 1),
               "LDP_CASE_S2": (2, 0, 2), "LDP_CASE_SH": (None, 0, 3), "LDP_CASE_SH32": (2, 0, 4)}


def instantiations():
    """Every X(...) row with a planner mode (K5 / DOWN / UP / P1) of the instantiation lists in csrc/tconv_*.hip, as the plan that launches
    it: -> {(mode, to, nwn, ks, cpi, res, mb, kws, split): 'file:LIST'} -- the tuple a trace row's `plan` is."""
    out = {}
    for f in sorted(CSRC.glob("tconv_*.hip")):
        text = f.read_text()
        lists = {m.group(1): m.group(2) for m in re.finditer(r"#define[ \t]+(\w+)\(X\)((?:.*\\\n)*.*\n)", text)}
        used = re.findall(r"^\s*(\w+)\((LDP_CASE\w*)\)", text, flags=re.M)
        assert {n for n, _ in used} == set(lists), (f.name, used, sorted(lists))
        for name, macro in used:
            mb, kws, split = CASE_MACROS[macro]
            for x in re.finditer(r"\bX\(\s*MODE_(\w+)\s*,([^)]*)\)", lists[name]):
                if x.group(1) not in MODES:
                    continue
                a = [int(v) for v in x.group(2).split(",")]
                assert len(a) == (6 if mb is None else 5), (f.name, name, x.group(0))
                key = (MODES[x.group(1)], *a[:5], a[5] if mb is None else mb, kws, split)
                assert key not in out, f"{key} is instantiated twice: {out[key]} and {f.name}:{name}"
                out[key] = f"{f.name}:{name}"
    return out


def plan_text(key):
    mode = {v: k for k, v in MODES.items()}[key[0]]
    return f"{mode}<to{key[1]} nwn{key[2]} ks{key[3]} cpi{key[4]} res{key[5]} mb{key[6]} kws{key[7]} split{key[8]}>"
