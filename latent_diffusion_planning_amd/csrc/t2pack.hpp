// t2pack.hpp -- weight packing of the exact-fp32 k = 5 convs that run over two positions (tconv.hpp, t2_shared()).
// Plain C++: engine.hip includes it, and a host compiler builds it alone (tests/test_t2_pack_cpu.py).
#pragma once
#include <cstddef>
#include <vector>

namespace ldp {

// Flax kernel w (5, cin, cout), optional 1x1 projection proj (cin, cout) or nullptr
//   -> [chunk][slot][cout_p/16][lane = kq*16 + n][s],  element (ci, co) = (chunk*16 + 4*kq + s, nblk*16 + n)   (pack_conv's fragment order)
// slots: 0 = W2, 1 = fl(W3 - W2), 2 = fl(W1 - W2), 3 = the projection where there is one.  The differences are taken in double from the
// fp32 weights and rounded once; taps 0 and 4 only ever meet zero padding at two positions and are not stored.  Padding (ci >= cin,
// co >= cout) is zero.
inline std::vector<float> pack_conv_t2(const float* w, const float* proj, int cin, int cout, int cin_p, int cout_p) {
  const int nchunk = cin_p / 16, nblk = cout_p / 16, ns = proj ? 4 : 3;
  std::vector<float> p((size_t)nchunk * ns * nblk * 256, 0.0f);
  auto tap = [&](int j, int ci, int co) { return w[((size_t)j * cin + ci) * cout + co]; };
  for (int gc = 0; gc < nchunk; ++gc)
    for (int sl = 0; sl < ns; ++sl)
      for (int nb = 0; nb < nblk; ++nb) {
        float* dst = p.data() + (((size_t)gc * ns + sl) * nblk + nb) * 256;
        for (int lane = 0; lane < 64; ++lane) {
          const int kq = lane >> 4, n = lane & 15;
          const int co = nb * 16 + n;
          for (int s = 0; s < 4; ++s) {
            const int ci = gc * 16 + 4 * kq + s;
            if (ci >= cin || co >= cout) continue;
            float v;
            if (sl == 0) v = tap(2, ci, co);
            else if (sl == 1) v = (float)((double)tap(3, ci, co) - (double)tap(2, ci, co));
            else if (sl == 2) v = (float)((double)tap(1, ci, co) - (double)tap(2, ci, co));
            else v = proj[(size_t)ci * cout + co];
            dst[lane * 4 + s] = v;
          }
        }
      }
  return p;
}

}  // namespace ldp
