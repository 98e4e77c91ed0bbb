"""csrc/t4pack.hpp on the host: the packing of the exact-fp32 k = 5 convs over four positions, built into a stand-alone program with the
address and undefined-behaviour sanitizers (the sanitizers live in that program only) and rebuilt here in numpy; then, in float64, the
nine-product recombination of the packed slots against the direct conv, which pins the slot order and every sign without a GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "latent_diffusion_planning_amd", "csrc")

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "t4pack.hpp"
// argv: cin cout cin_p cout_p proj w.bin out.bin ; w.bin = 5*cin*cout floats (+ cin*cout of the projection)
int main(int argc, char** argv) {
  if (argc != 8) return 2;
  const int cin = atoi(argv[1]), cout = atoi(argv[2]), cin_p = atoi(argv[3]), cout_p = atoi(argv[4]), proj = atoi(argv[5]);
  std::vector<float> w((size_t)(5 + proj) * cin * cout);
  FILE* f = fopen(argv[6], "rb");
  if (!f || fread(w.data(), 4, w.size(), f) != w.size()) return 3;
  fclose(f);
  const std::vector<float> p = ldp::pack_conv_t4(w.data(), proj ? w.data() + (size_t)5 * cin * cout : nullptr, cin, cout, cin_p, cout_p);
  f = fopen(argv[7], "wb");
  if (!f || fwrite(p.data(), 4, p.size(), f) != p.size()) return 4;
  fclose(f);
  printf("%zu\n", p.size());
  return 0;
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("t4pack")
    src = d / "main.cpp"
    src.write_text(MAIN)
    exe = d / "t4pack"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def combos(w):
    """The nine slots of t4pack.hpp from the fp32 taps w (5, cin, cout): float64 combinations, rounded once."""
    w0, w1, w2, w3, w4 = (w[j].astype(np.float64) for j in range(5))
    a, ap = w4 - w2, w0 - w2
    return [c.astype(np.float32) for c in (w2, w3 - w2, w1 - w2, a, -w3 - a, w3 - w1 - a, ap, w1 - w3 - ap, -w1 - ap)]


def expected(w, proj, cin, cout, cin_p, cout_p):
    """[chunk][slot][cout_p/16][lane = kq*16 + n][s] holding element (chunk*16 + 4*kq + s, nblk*16 + n) of the nine slots, then the projection."""
    slots = combos(w) + ([proj] if proj is not None else [])
    full = np.zeros((len(slots), cin_p, cout_p), np.float32)
    for i, s in enumerate(slots):
        full[i, :cin, :cout] = s
    # (slot, chunk, kq, s, nblk, n) -> (chunk, slot, nblk, kq, n, s)
    t = full.reshape(len(slots), cin_p // 16, 4, 4, cout_p // 16, 16).transpose(1, 0, 4, 2, 5, 3)
    return np.ascontiguousarray(t).reshape(-1)


def unpack(got, ns, cin_p, cout_p):
    """packed array -> (slot, cin_p, cout_p)"""
    v = got.reshape(cin_p // 16, ns, cout_p // 16, 4, 16, 4)      # [chunk][slot][nblk][kq][n][s]
    return v.transpose(1, 0, 3, 5, 2, 4).reshape(ns, cin_p, cout_p)


def run(prog, tmp_path, w, proj, cin, cout, cin_p, cout_p):
    wf, of = tmp_path / "w.bin", tmp_path / "out.bin"
    np.concatenate([w.reshape(-1)] + ([proj.reshape(-1)] if proj is not None else [])).tofile(wf)
    r = subprocess.run([str(prog), str(cin), str(cout), str(cin_p), str(cout_p), str(int(proj is not None)), str(wf), str(of)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    got = np.fromfile(of, np.float32)
    ns = 10 if proj is not None else 9
    assert int(r.stdout) == got.size == (cin_p // 16) * ns * (cout_p // 16) * 256
    return got, ns


@pytest.mark.parametrize("cin,cout,cin_p,cout_p", [(32, 32, 32, 32), (48, 16, 48, 16), (32, 32, 64, 48), (48, 16, 128, 32), (25, 16, 32, 16)])
@pytest.mark.parametrize("with_proj", [False, True])
def test_pack_conv_t4(prog, tmp_path, cin, cout, cin_p, cout_p, with_proj):
    g = np.random.Generator(np.random.PCG64(cin * 100 + cout + with_proj))
    w = (g.standard_normal((5, cin, cout)) / np.sqrt(5 * cin)).astype(np.float32)
    w[3, 0, 0] = w[2, 0, 0] * (1 + 2.0 ** -20)       # a difference far below either operand: one rounding, from the exact difference
    w[4, 0, 0] = w[2, 0, 0] * (1 - 2.0 ** -21)
    proj = g.standard_normal((cin, cout)).astype(np.float32) if with_proj else None
    got, ns = run(prog, tmp_path, w, proj, cin, cout, cin_p, cout_p)
    exp = expected(w, proj, cin, cout, cin_p, cout_p)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), "packed array differs bit for bit"
    # spelled out element by element: each slot is its float64 combination of the fp32 taps rounded once, the projection last, zero padding
    v = unpack(got, ns, cin_p, cout_p)
    f8 = np.float64
    for ci, co in [(0, 0), (cin - 1, cout - 1), (17 % cin, 5 % cout)]:
        w0, w1, w2, w3, w4 = (f8(w[j, ci, co]) for j in range(5))
        want = (w2, w3 - w2, w1 - w2, w4 - w2, -w3 - (w4 - w2), w3 - w1 - (w4 - w2), w0 - w2, w1 - w3 - (w0 - w2), -w1 - (w0 - w2))
        for sl in range(9):
            assert v[sl, ci, co] == np.float32(want[sl]), (sl, ci, co)
        if with_proj:
            assert v[9, ci, co] == proj[ci, co]
    assert not v[:, cin:, :].any() and not v[:, :, cout:].any()


@pytest.mark.parametrize("with_proj", [False, True])
def test_nine_products_of_the_packed_slots_are_the_conv(prog, tmp_path, with_proj):
    """In float64, on the slots as packed (fp32 values): s .. db1 recombined as the kernel does against the direct k = 5 conv over four
    zero-padded positions.  The slots' one rounding (2^-24 relative each) is all that separates the two; with weights that are exact in few
    bits the combinations are exact and the bound is float64 round-off, 1e-12."""
    cin, cout, cin_p, cout_p = 48, 32, 64, 32
    g = np.random.Generator(np.random.PCG64(77 + with_proj))
    w = (np.round(g.standard_normal((5, cin, cout)) * 64) / 256).astype(np.float32)      # multiples of 2^-8: every combination is exact in fp32
    proj = g.standard_normal((cin, cout)).astype(np.float32) if with_proj else None
    got, ns = run(prog, tmp_path, w, proj, cin, cout, cin_p, cout_p)
    v = unpack(got, ns, cin_p, cout_p).astype(np.float64)
    x = np.zeros((7, 4, cin_p))
    x[:, :, :cin] = g.standard_normal((7, 4, cin))
    x0, x1, x2, x3 = (x[:, t] for t in range(4))
    u0, u1 = x0 + x2, x1 + x3
    s, e0, e1 = (u0 + u1) @ v[0], u1 @ v[1], u0 @ v[2]
    p, dt0, dt1 = (x2 + x3) @ v[3], x3 @ v[4], x2 @ v[5]
    q, db0, db1 = (x0 + x1) @ v[6], x1 @ v[7], x0 @ v[8]
    y = np.stack([s + e0 + p + dt0, s + e1 + p + dt1, s + e0 + q + db0, s + e1 + q + db1], 1)[:, :, :cout]
    ref = np.zeros((7, 4, cout))
    w64 = w.astype(np.float64)
    for t in range(4):
        for j in range(5):
            ti = t + j - 2
            if 0 <= ti < 4:
                ref[:, t] += x[:, ti, :cin] @ w64[j]
    err = np.abs(y - ref).max()
    assert err < 1e-12, err
    if with_proj:
        assert np.array_equal(v[9, :cin, :cout], proj.astype(np.float64))
