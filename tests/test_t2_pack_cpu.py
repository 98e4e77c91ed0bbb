"""csrc/t2pack.hpp on the host: the packing of the exact-fp32 k = 5 convs over two positions, built into a stand-alone program with the
address and undefined-behaviour sanitizers (the sanitizers live in that program only) and rebuilt here in numpy."""
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
#include "t2pack.hpp"
// argv: cin cout cin_p cout_p proj w.bin out.bin ; w.bin = 5*cin*cout floats (+ cin*cout of the projection)
int main(int argc, char** argv) {
  if (argc != 8) return 2;
  const int cin = atoi(argv[1]), cout = atoi(argv[2]), cin_p = atoi(argv[3]), cout_p = atoi(argv[4]), proj = atoi(argv[5]);
  std::vector<float> w((size_t)(5 + proj) * cin * cout);
  FILE* f = fopen(argv[6], "rb");
  if (!f || fread(w.data(), 4, w.size(), f) != w.size()) return 3;
  fclose(f);
  const std::vector<float> p = ldp::pack_conv_t2(w.data(), proj ? w.data() + (size_t)5 * cin * cout : nullptr, cin, cout, cin_p, cout_p);
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
    d = tmp_path_factory.mktemp("t2pack")
    src = d / "main.cpp"
    src.write_text(MAIN)
    exe = d / "t2pack"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def expected(w, proj, cin, cout, cin_p, cout_p):
    """[chunk][slot][cout_p/16][lane = kq*16 + n][s] holding element (chunk*16 + 4*kq + s, nblk*16 + n) of W2, fl(W3 - W2), fl(W1 - W2), projection."""
    w64 = w.astype(np.float64)
    slots = [w[2], (w64[3] - w64[2]).astype(np.float32), (w64[1] - w64[2]).astype(np.float32)] + ([proj] if proj is not None else [])
    full = np.zeros((len(slots), cin_p, cout_p), np.float32)
    for i, s in enumerate(slots):
        full[i, :cin, :cout] = s
    # (slot, chunk, kq, s, nblk, n) -> (chunk, slot, nblk, kq, n, s)
    t = full.reshape(len(slots), cin_p // 16, 4, 4, cout_p // 16, 16).transpose(1, 0, 4, 2, 5, 3)
    return np.ascontiguousarray(t).reshape(-1)


@pytest.mark.parametrize("cin,cout,cin_p,cout_p", [(32, 32, 32, 32), (48, 16, 48, 16), (32, 32, 64, 48), (48, 16, 128, 32), (25, 16, 32, 16)])
@pytest.mark.parametrize("with_proj", [False, True])
def test_pack_conv_t2(prog, tmp_path, cin, cout, cin_p, cout_p, with_proj):
    g = np.random.Generator(np.random.PCG64(cin * 100 + cout + with_proj))
    w = (g.standard_normal((5, cin, cout)) / np.sqrt(5 * cin)).astype(np.float32)
    w[3, 0, 0] = w[2, 0, 0] * (1 + 2.0 ** -20)       # a difference far below either operand: one rounding, from the exact difference
    proj = g.standard_normal((cin, cout)).astype(np.float32) if with_proj else None
    wf, of = tmp_path / "w.bin", tmp_path / "out.bin"
    np.concatenate([w.reshape(-1)] + ([proj.reshape(-1)] if with_proj else [])).tofile(wf)
    r = subprocess.run([str(prog), str(cin), str(cout), str(cin_p), str(cout_p), str(int(with_proj)), str(wf), str(of)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    got = np.fromfile(of, np.float32)
    ns = 4 if with_proj else 3
    assert int(r.stdout) == got.size == (cin_p // 16) * ns * (cout_p // 16) * 256
    exp = expected(w, proj, cin, cout, cin_p, cout_p)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), "packed array differs bit for bit"
    # spelled out on the 6-d view: the middle tap as it is, the differences rounded once from float64, zero padding, the projection last
    v = got.reshape(cin_p // 16, ns, cout_p // 16, 4, 16, 4)      # [chunk][slot][nblk][kq][n][s]
    def elem(slot, ci, co):
        return v[ci // 16, slot, co // 16, (ci % 16) // 4, co % 16, ci % 4]
    for ci, co in [(0, 0), (cin - 1, cout - 1), (17 % cin, 5 % cout)]:
        assert elem(0, ci, co) == w[2, ci, co]
        assert elem(1, ci, co) == np.float32(np.float64(w[3, ci, co]) - np.float64(w[2, ci, co]))
        assert elem(2, ci, co) == np.float32(np.float64(w[1, ci, co]) - np.float64(w[2, ci, co]))
        if with_proj:
            assert elem(3, ci, co) == proj[ci, co]
    if cin_p > cin:
        assert not v.transpose(0, 3, 5, 1, 2, 4).reshape(cin_p, ns, cout_p)[cin:].any()
    if cout_p > cout:
        assert not v.transpose(2, 4, 0, 1, 3, 5).reshape(cout_p, -1)[cout:].any()
