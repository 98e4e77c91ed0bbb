// train_tables.hpp -- the launch tables of the training convolutions (csrc/train.hip's seg_gemm family).  Host only: standard headers, nothing
// from HIP, so that tests/test_train_tables_cpu.py can build it into a stand-alone program.
//
// A launch of the segmented GEMM runs a range of BATCHES; batch z accumulates its SEGMENTS in list order, each with its own operand offsets:
//     C_z = sum over segments s of z:  A(a_off(s)) . B(b_off(s))
// With rows = samples a convolution over Tin inputs (positions of the U-Net, pixels of the 2-D networks) and Tout outputs is three such tables:
//     forward   z = output,  segments = its live taps                          a_off = input * cin,   b_off = tap * cin * cout
//     dgrad     z = input,   segments = the (output, tap) pairs that read it   a_off = output * cout,  b_off = tap * cin * cout
//     wgrad     z = tap,     segments = the outputs where the tap is live      a_off = input * cin,   b_off = output * cout
// Taps that fall on padding are in no list; a tap that is live nowhere has no wgrad batch (its gradient stays zero).  The order of a batch's
// segments is the summation order of its split K, so it decides the bits of every gradient: forward tap-minor, dgrad output-major and tap-minor,
// wgrad by output.
#pragma once

#include <algorithm>
#include <vector>

namespace ldp {
namespace train_tables {

struct GemmSeg { long long a_off, b_off; };
struct GemmBatch { long long c_off; int seg_begin, seg_end; long long bias_off = 0; };      // bias_off: this batch's bias row = GemmArgs::bias + bias_off

struct LaunchTables {              // every launch's segments and batches, appended to as convolutions are planned (the Trainer uploads them)
  std::vector<GemmSeg> segs;
  std::vector<GemmBatch> batches;
};

struct ConvPlan {                  // launch tables of one convolution (indices into LaunchTables::batches)
  int Tin = 0, Tout = 0, cin = 0, cout = 0, ntaps = 0;
  int f_b0 = 0, f_nb = 0, d_b0 = 0, d_nb = 0, w_b0 = 0, w_nb = 0;      // first batch / batch count of the forward, dgrad, wgrad launches
  int f_minseg = 0, d_minseg = 0, w_minseg = 0;                       // fewest segments any batch of the forward / dgrad / wgrad launch has (split-K sizing)
};

// ---- tap sets: the input that tap j of output `to` reads, or -1 (padding, out of range, a tap that does not contribute there) ----------------
enum : int { CONV1_K5 = 0, CONV1_DOWN = 1, CONV1_UP = 2, CONV1_P1 = 3 };      // 1-D, numbered as csrc/tconv.hpp's MODE_K5 / MODE_DOWN / MODE_UP / MODE_P1
enum : int { VC_S1 = 0, VC_S2 = 1, VC_UP = 2, VC_P1 = 3, VC_P2 = 4 };         // 2-D: 3x3 pad 1, 3x3 stride 2 pad (0, 1), nearest x2 then 3x3, 1x1, 1x1 stride 2

inline int ntaps_1d(int mode) { return mode == CONV1_K5 ? 5 : mode == CONV1_DOWN ? 3 : mode == CONV1_UP ? 4 : 1; }
inline int tap_1d(int mode, int Tin, int to, int j) {
  int ti = to;
  switch (mode) {
    case CONV1_K5: ti = to + j - 2; break;
    case CONV1_DOWN: ti = 2 * to + j; break;                                 // XLA SAME on an even length: pads (0, 1)
    case CONV1_UP: {                                                         // out[2q] = x[q-1] K0 + x[q] K2; out[2q+1] = x[q] K1 + x[q+1] K3
      const int q = to >> 1;
      if ((to & 1) == 0) ti = j == 0 ? q - 1 : j == 2 ? q : -1;
      else ti = j == 1 ? q : j == 3 ? q + 1 : -1;
      break;
    }
    default: break;
  }
  return ti >= 0 && ti < Tin ? ti : -1;
}

inline int ntaps_2d(int mode) { return (mode == VC_P1 || mode == VC_P2) ? 1 : 9; }
// square images of side Sin / Sout, pixels row-major.  Stride 2 reads input (2y + dy, 2x + dx); the nearest x2 upsample is folded into its 3x3:
// tap (dy, dx) of output (y, x) reads input ((y + dy - 1) >> 1, (x + dx - 1) >> 1), so neither the upsampled tensor nor its gradient exists.
inline int tap_2d(int mode, int Sin, int Sout, int po, int j) {
  const int y = po / Sout, x = po % Sout, dy = j / 3, dx = j % 3;
  int iy = y, ix = x;
  switch (mode) {
    case VC_S1: iy = y + dy - 1; ix = x + dx - 1; break;
    case VC_S2: iy = 2 * y + dy; ix = 2 * x + dx; break;
    case VC_UP: {
      const int uy = y + dy - 1, ux = x + dx - 1;
      if (uy < 0 || ux < 0 || uy >= Sout || ux >= Sout) return -1;
      iy = uy >> 1; ix = ux >> 1;
      break;
    }
    case VC_P2: if (j != 0) return -1; iy = 2 * y; ix = 2 * x; break;
    default: if (j != 0) return -1; break;
  }
  return (iy < 0 || ix < 0 || iy >= Sin || ix >= Sin) ? -1 : iy * Sin + ix;
}

// ---- the builder -------------------------------------------------------------------------------------------------------------------
// One sweep over (output, tap), output-major and tap-minor: the segment list of every forward, dgrad and wgrad batch, in summation order.
struct TapWalk { std::vector<std::vector<GemmSeg>> fwd, dgrad, wgrad; };      // [output], [input], [tap]

template <class Tap>               // tap(to, j) -> input index, or -1
TapWalk walk_taps(int Tin, int Tout, int cin, int cout, int ntaps, Tap&& tap) {
  TapWalk w;
  w.fwd.resize(Tout); w.dgrad.resize(Tin); w.wgrad.resize(ntaps);
  const long long wtap = (long long)cin * cout;
  for (int to = 0; to < Tout; ++to)
    for (int j = 0; j < ntaps; ++j) {
      const int ti = tap(to, j);
      if (ti < 0 || ti >= Tin) continue;
      w.fwd[to].push_back(GemmSeg{(long long)ti * cin, j * wtap});
      w.dgrad[ti].push_back(GemmSeg{(long long)to * cout, j * wtap});
      w.wgrad[j].push_back(GemmSeg{(long long)ti * cin, (long long)to * cout});
    }
  return w;
}

// appends the three tables of one convolution (cin / cout as the arena pads them) and returns where they are
template <class Tap>
ConvPlan plan_taps(LaunchTables& tb, int Tin, int Tout, int cin, int cout, int ntaps, Tap&& tap) {
  const TapWalk w = walk_taps(Tin, Tout, cin, cout, ntaps, tap);
  ConvPlan c;
  c.Tin = Tin; c.Tout = Tout; c.cin = cin; c.cout = cout; c.ntaps = ntaps;
  // one launch: batch z writes C at z * c_stride; a wgrad batch without segments (a tap that is dead everywhere) is dropped
  auto launch = [&tb](const std::vector<std::vector<GemmSeg>>& lists, long long c_stride, bool drop_empty, int& b0, int& nb, int& minseg) {
    b0 = (int)tb.batches.size();
    for (size_t z = 0; z < lists.size(); ++z) {
      const int n = (int)lists[z].size(), s0 = (int)tb.segs.size();
      if (drop_empty && n == 0) continue;
      tb.segs.insert(tb.segs.end(), lists[z].begin(), lists[z].end());
      tb.batches.push_back(GemmBatch{(long long)z * c_stride, s0, s0 + n});
      minseg = nb == 0 ? n : std::min(minseg, n);
      ++nb;
    }
  };
  launch(w.fwd, cout, false, c.f_b0, c.f_nb, c.f_minseg);
  launch(w.dgrad, cin, false, c.d_b0, c.d_nb, c.d_minseg);
  launch(w.wgrad, (long long)cin * cout, true, c.w_b0, c.w_nb, c.w_minseg);
  return c;
}

inline ConvPlan plan_1d(LaunchTables& tb, int mode, int Tin, int Tout, int cin, int cout) {
  return plan_taps(tb, Tin, Tout, cin, cout, ntaps_1d(mode), [=](int to, int j) { return tap_1d(mode, Tin, to, j); });
}
inline ConvPlan plan_2d(LaunchTables& tb, int mode, int Sin, int Sout, int cin, int cout) {
  return plan_taps(tb, Sin * Sin, Sout * Sout, cin, cout, ntaps_2d(mode), [=](int po, int j) { return tap_2d(mode, Sin, Sout, po, j); });
}

}  // namespace train_tables
}  // namespace ldp
