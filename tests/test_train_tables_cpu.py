"""csrc/train_tables.hpp on the host: the builder of the training convolutions' launch tables, built into a stand-alone program with the
address and undefined-behaviour sanitizers (the sanitizers live in that program only).  Its tables are held against the restatement in
tests/train_cases.py entry by entry (the order of a batch's segments is the summation order of its split K), and, independently of that
restatement, against the convolution written from its definition in numpy: the three tables must compute the convolution, its transpose and
its weight gradient.  cin = 2, cout = 3 throughout, so that a swapped multiplier in an offset shows."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import train_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "latent_diffusion_planning_amd", "csrc")
CIN, COUT = 2, 3

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "train_tables.hpp"
using namespace ldp::train_tables;
// argv: 1d|2d mode Sin Sout cin cout  (1d: positions in / out; 2d: image sides in / out) -> the plan, then every segment and batch, on stdout
int main(int argc, char** argv) {
  if (argc != 7) return 2;
  const int mode = atoi(argv[2]), Sin = atoi(argv[3]), Sout = atoi(argv[4]), cin = atoi(argv[5]), cout = atoi(argv[6]);
  LaunchTables tb;
  ConvPlan p;
  if (!strcmp(argv[1], "1d")) p = plan_1d(tb, mode, Sin, Sout, cin, cout);
  else if (!strcmp(argv[1], "2d")) p = plan_2d(tb, mode, Sin, Sout, cin, cout);
  else return 2;
  printf("plan %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", p.Tin, p.Tout, p.cin, p.cout, p.ntaps, p.f_b0, p.f_nb, p.f_minseg, p.d_b0, p.d_nb, p.d_minseg,
         p.w_b0, p.w_nb, p.w_minseg);
  for (const GemmSeg& s : tb.segs) printf("seg %lld %lld\n", s.a_off, s.b_off);
  for (const GemmBatch& b : tb.batches) printf("batch %lld %d %d %lld\n", b.c_off, b.seg_begin, b.seg_end, b.bias_off);
  return 0;
}
"""

# (family, mode, side / length in, out): the smallest shapes at which the builder can go wrong
CASES = [
    ("1d", TC.MODE_K5, 2, 2),        # taps 0 and 4 are dead everywhere: w_nb = 3, their batches are dropped
    ("1d", TC.MODE_K5, 4, 4),
    ("1d", TC.MODE_DOWN, 4, 2),      # the last tap falls on the right padding
    ("1d", TC.MODE_UP, 2, 4),
    ("1d", TC.MODE_P1, 4, 4),
    ("2d", TC.VC_S1, 2, 2),
    ("2d", TC.VC_S1, 4, 4),
    ("2d", TC.VC_S2, 4, 2),
    ("2d", TC.VC_S2, 2, 1),
    ("2d", TC.VC_UP, 2, 4),
    ("2d", TC.VC_P1, 2, 2),
    ("2d", TC.VC_P2, 4, 2),          # the input pixels the stride skips have no segment: d_minseg = 0
]
IDS = [f"{f}-mode{m}-{a}to{b}" for f, m, a, b in CASES]
PLAN_KEYS = ("Tin", "Tout", "cin", "cout", "ntaps", "f_b0", "f_nb", "f_minseg", "d_b0", "d_nb", "d_minseg", "w_b0", "w_nb", "w_minseg")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("train_tables")
    src = d / "main.cpp"
    src.write_text(MAIN)
    exe = d / "train_tables"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def built(prog, family, mode, Sin, Sout):
    """-> dict(plan, segs, batches) as the program printed them."""
    r = subprocess.run([str(prog), family, str(mode), str(Sin), str(Sout), str(CIN), str(COUT)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    out = dict(plan=None, segs=[], batches=[])
    for line in r.stdout.splitlines():
        kind, *v = line.split()
        v = [int(x) for x in v]
        if kind == "plan":
            out["plan"] = dict(zip(PLAN_KEYS, v))
        elif kind == "seg":
            out["segs"].append(tuple(v))
        else:
            assert v[3] == 0, "a convolution's batches carry no bias offset"
            out["batches"].append(tuple(v[:3]))
    assert out["plan"] is not None
    return out


@pytest.mark.parametrize("family,mode,Sin,Sout", CASES, ids=IDS)
def test_tables_equal_the_restatement(prog, family, mode, Sin, Sout):
    got, want = built(prog, family, mode, Sin, Sout), TC.conv_tables(family, mode, Sin, Sout, CIN, COUT)
    assert got["segs"] == want["segs"]
    assert got["batches"] == want["batches"]
    assert got["plan"] == dict(want["plan"], cin=CIN, cout=COUT)
    if family == "2d" and mode != TC.VC_UP:                               # the count restatement the launch-shape tests use says the same
        assert TC.conv_plan(mode, Sin, Sout) == {k: got["plan"][k] for k in ("f_nb", "f_minseg", "d_nb", "d_minseg", "w_nb", "w_minseg")}


def test_the_cases_reach_what_they_are_chosen_for(prog):
    p = built(prog, "1d", TC.MODE_K5, 2, 2)["plan"]
    assert (p["ntaps"], p["w_nb"]) == (5, 3)
    assert built(prog, "2d", TC.VC_P2, 4, 2)["plan"]["d_minseg"] == 0
    d = built(prog, "1d", TC.MODE_DOWN, 4, 2)
    assert d["plan"]["f_minseg"] == 2 and d["segs"][d["batches"][1][1]:d["batches"][1][2]] == [(2 * CIN, 0), (3 * CIN, CIN * COUT)]


# ---- the convolutions from their definitions: padded input, explicit loops -------------------------------------------------------------------
def conv_def(family, mode, Sin, Sout, x, w):
    """x (Tin, cin), w (ntaps, cin, cout) float64 -> y (Tout, cout).  1-D: k = 5 pad (2, 2); k = 3 stride 2 with XLA SAME pads (0, 1); the
    transposed k = 4 stride 2 as lax.conv_transpose computes it under SAME (input dilated by 2, pads (2, 2), the kernel not flipped); 1x1.
    2-D (pixels row-major, taps (dy, dx) row-major): 3x3 pad 1; 3x3 stride 2 pads (0, 1) in both directions; nearest x2, then 3x3 pad 1; 1x1;
    1x1 stride 2."""
    cin, cout = x.shape[1], w.shape[2]
    if family == "1d":
        if mode == TC.MODE_UP:
            u = np.zeros((2 * Sin - 1, cin))
            u[::2] = x
            x, stride, k, pads = u, 1, 4, (2, 2)
        else:
            stride, k, pads = {TC.MODE_K5: (1, 5, (2, 2)), TC.MODE_DOWN: (2, 3, (0, 1)), TC.MODE_P1: (1, 1, (0, 0))}[mode]
        xp = np.pad(x, (pads, (0, 0)))
        assert stride * (Sout - 1) + k == len(xp)                         # (the last output's last tap is the padded input's last element)
        y = np.zeros((Sout, cout))
        for to in range(Sout):
            for j in range(k):
                y[to] += xp[stride * to + j] @ w[j]
        return y
    img = x.reshape(Sin, Sin, cin)
    if mode == TC.VC_UP:
        img = img.repeat(2, axis=0).repeat(2, axis=1)
    stride, k, pads = {TC.VC_S1: (1, 3, (1, 1)), TC.VC_S2: (2, 3, (0, 1)), TC.VC_UP: (1, 3, (1, 1)), TC.VC_P1: (1, 1, (0, 0)), TC.VC_P2: (2, 1, (0, 0))}[mode]
    xp = np.pad(img, (pads, pads, (0, 0)))
    y = np.zeros((Sout, Sout, cout))
    for oy in range(Sout):
        for ox in range(Sout):
            for dy in range(k):
                for dx in range(k):
                    y[oy, ox] += xp[stride * oy + dy, stride * ox + dx] @ w[dy * k + dx]
    return y.reshape(Sout * Sout, cout)


@pytest.mark.parametrize("family,mode,Sin,Sout", CASES, ids=IDS)
def test_tables_compute_the_convolution_its_transpose_and_its_weight_gradient(prog, family, mode, Sin, Sout):
    t = built(prog, family, mode, Sin, Sout)
    p, segs, batches = t["plan"], t["segs"], t["batches"]
    Tin, Tout, ntaps, wtap = p["Tin"], p["Tout"], p["ntaps"], CIN * COUT
    assert (Tin, Tout) == ((Sin, Sout) if family == "1d" else (Sin * Sin, Sout * Sout)) and len(batches) == p["f_nb"] + p["d_nb"] + p["w_nb"]
    g = np.random.Generator(np.random.PCG64(1000 * mode + 10 * Sin + Sout + (family == "2d")))
    x = g.integers(-4, 5, (Tin, CIN)).astype(np.float64)                  # small integers: every sum below is exact in float64
    w = g.integers(-4, 5, (ntaps, CIN, COUT)).astype(np.float64)
    dy = g.integers(-4, 5, (Tout, COUT)).astype(np.float64)
    xf, wf, dyf = x.reshape(-1), w.reshape(-1), dy.reshape(-1)

    def launch(b0, nb):
        return [(c, segs[s0:s1]) for c, s0, s1 in batches[b0:b0 + nb]]

    # forward: batch = one output, C[c_off : c_off + cout] = sum over its segments of X[a_off : + cin] . W[b_off : + cin cout]
    y = np.full(Tout * COUT, np.nan)
    for c_off, ss in launch(p["f_b0"], p["f_nb"]):
        y[c_off:c_off + COUT] = sum((xf[a:a + CIN] @ wf[b:b + wtap].reshape(CIN, COUT) for a, b in ss), np.zeros(COUT))
    ref = conv_def(family, mode, Sin, Sout, x, w)
    assert np.array_equal(y.reshape(Tout, COUT), ref)

    # the convolution is linear in x and in w: its two Jacobians from the definition alone, one basis vector at a time
    Jx = np.stack([conv_def(family, mode, Sin, Sout, e.reshape(Tin, CIN), w).reshape(-1) for e in np.eye(Tin * CIN)], axis=1)
    Jw = np.stack([conv_def(family, mode, Sin, Sout, x, e.reshape(ntaps, CIN, COUT)).reshape(-1) for e in np.eye(ntaps * wtap)], axis=1)

    # data gradient: batch = one input, C[c_off : + cin] = sum of dY[a_off : + cout] . W[b_off]^T; an input nothing reads is written as zero
    dx = np.full(Tin * CIN, np.nan)
    for c_off, ss in launch(p["d_b0"], p["d_nb"]):
        dx[c_off:c_off + CIN] = sum((dyf[a:a + COUT] @ wf[b:b + wtap].reshape(CIN, COUT).T for a, b in ss), np.zeros(CIN))
    assert np.array_equal(dx, Jx.T @ dyf)

    # weight gradient: batch = one live tap, C[c_off : + cin cout] = sum of X[a_off : + cin]^T dY[b_off : + cout]; nothing is written for a dead tap
    dw = np.full(ntaps * wtap, np.nan)
    for c_off, ss in launch(p["w_b0"], p["w_nb"]):
        assert ss and c_off % wtap == 0
        dw[c_off:c_off + wtap] = sum(np.outer(xf[a:a + CIN], dyf[b:b + COUT]) for a, b in ss).reshape(-1)
    live = np.array([np.abs(conv_def(family, mode, Sin, Sout, np.ones((Tin, CIN)), (np.arange(ntaps) == j)[:, None, None] * np.ones((ntaps, CIN, COUT)))).any()
                     for j in range(ntaps)])
    written = ~np.isnan(dw.reshape(ntaps, wtap)).any(axis=1)
    assert np.array_equal(written, live), (written, live)
    assert np.array_equal(np.where(np.isnan(dw), 0.0, dw), Jw.T @ dyf)
    assert p["w_nb"] == int(live.sum())
