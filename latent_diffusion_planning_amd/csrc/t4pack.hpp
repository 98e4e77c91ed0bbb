// t4pack.hpp -- weight packing of the exact-fp32 k = 5 convs that run over four positions (tconv.hpp, t4_shared()).
// Plain C++: engine.hip includes it, and a host compiler builds it alone (tests/test_t4_pack_cpu.py).
#pragma once
#include <cstddef>
#include <vector>

namespace ldp {

// The nine weight combinations of the form, from the five fp32 taps of one (ci, co) element, each taken in double and rounded once.
// Slot order (the kernel's accumulator order; a = W4 - W2, a' = W0 - W2):
//   0  W2                 x (x0 + x1 + x2 + x3)   s        3  a                  x (x2 + x3)   p        6  a'                 x (x0 + x1)   q
//   1  W3 - W2            x (x1 + x3)             e0       4  -W3 - a            x x3          dt0      7  W1 - W3 - a'       x x1          db0
//   2  W1 - W2            x (x0 + x2)             e1       5  W3 - W1 - a        x x2          dt1      8  -W1 - a'           x x0          db1
//   y0 = s + e0 + p + dt0,   y1 = s + e1 + p + dt1,   y2 = s + e0 + q + db0,   y3 = s + e1 + q + db1
inline void t4_combine(const float w[5], float out[9]) {
  const double w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
  const double a = w4 - w2, ap = w0 - w2;
  out[0] = w[2];
  out[1] = (float)(w3 - w2);
  out[2] = (float)(w1 - w2);
  out[3] = (float)a;
  out[4] = (float)(-w3 - a);
  out[5] = (float)(w3 - w1 - a);
  out[6] = (float)ap;
  out[7] = (float)(w1 - w3 - ap);
  out[8] = (float)(-w1 - ap);
}

// Flax kernel w (5, cin, cout), optional 1x1 projection proj (cin, cout) or nullptr
//   -> [chunk][slot][cout_p/16][lane = kq*16 + n][s],  element (ci, co) = (chunk*16 + 4*kq + s, nblk*16 + n)   (pack_conv's fragment order)
// slots 0..8 as t4_combine orders them, slot 9 = the projection where there is one.  Padding (ci >= cin, co >= cout) is zero.
inline std::vector<float> pack_conv_t4(const float* w, const float* proj, int cin, int cout, int cin_p, int cout_p) {
  const int nchunk = cin_p / 16, nblk = cout_p / 16, ns = proj ? 10 : 9;
  std::vector<float> p((size_t)nchunk * ns * nblk * 256, 0.0f);
  for (int gc = 0; gc < nchunk; ++gc)
    for (int nb = 0; nb < nblk; ++nb)
      for (int lane = 0; lane < 64; ++lane) {
        const int kq = lane >> 4, n = lane & 15;
        const int co = nb * 16 + n;
        for (int s = 0; s < 4; ++s) {
          const int ci = gc * 16 + 4 * kq + s;
          if (ci >= cin || co >= cout) continue;
          float taps[5], v[9];
          for (int j = 0; j < 5; ++j) taps[j] = w[((size_t)j * cin + ci) * cout + co];
          t4_combine(taps, v);
          for (int sl = 0; sl < ns; ++sl)
            p[(((size_t)gc * ns + sl) * nblk + nb) * 256 + lane * 4 + s] = sl < 9 ? v[sl] : proj[(size_t)ci * cout + co];
        }
      }
  return p;
}

}  // namespace ldp
