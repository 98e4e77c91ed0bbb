// resnet_train.hpp -- the ResNet-18 image encoder of the diffusion-policy baseline (networks/resnet_v1.py:237-346, csrc/resnet.hip's forward)
// as a training tape: ResNetEncoder.apply with every activation kept, and its VJP w.r.t. all 60 leaves.
//
// Included by train.hip inside its anonymous namespace, after vae_train.hpp: an encoder slot is module bit 8 << slot of the same Trainer (flat
// arenas, Adam + EMA in one launch, read / write / publish by Flax path), its convolutions run through the VAE tape's 2-D launch tables
// (plan_2d of train_tables.hpp: rows = samples, z = pixel) on the exact-fp32 segmented GEMM.  The sixteen 3x3 convolutions are VC_S1 / VC_S2, the three conv_proj
// the stride-2 1x1 table VC_P2.  Nothing in this network has a bias, so the tape has no column sums besides the norms' scale / bias partials.
//
// Stem (7x7 stride 2 pad 3, 3 -> 64 channels).  Each output pixel's 147-value patch is gathered once, in the Flax leaf's own flattening
// k = dy * 21 + dx * 3 + c (rn_stem_kernel's virtual K index), K padded to 160: the stem and its weight gradient are plain 1x1 launches over
// (Bp, 1024, 160), and the arena holds conv_init/kernel as [160][64] with 13 zero rows (their gradient is the product with zero patch columns:
// exactly zero).  The image is not a parameter: there is no data gradient.
//
// The forward and the backward are two calls (the U-Net tape runs between them), so each slot owns a lane: the forward call sizes the lane's
// workspace for both walks, the backward call re-walks the forward's bump allocation without launching and appends its own buffers.
// Rows are padded to 32 with zero frames; their activations are not zero (the norms' biases), their feature gradient is, and so is everything the
// backward derives from it: padding contributes exactly nothing to a weight gradient.  No atomics; every sum has a fixed order.

constexpr int RNT_S = 64, RNT_F = 64, RNT_G = 4, RNT_BLOCKS = 8;
constexpr int RNT_K = 147, RNT_KP = 160;    // the stem's K = 7 * 7 * 3 and its padding to the GEMM's K step
constexpr int RNT_FEAT = 1024;              // [expected_x (512) | expected_y (512)]
constexpr int RNT_MAX_FRAMES = 1024;        // frames per forward: 256 samples x obs_horizon 2 x two cameras through a shared encoder
constexpr float RNT_EPS = 1e-5f;

// patches (Bp, 32 * 32, 160) <- img (N, 64, 64, 3): column k = dy * 21 + dx * 3 + c of output pixel (oy, ox) is img(2 oy + dy - 3, 2 ox + dx - 3, c);
// zero outside the frame, in columns 147 .. 159 and in the padding frames
__global__ void rnt_patch_kernel(const float* __restrict__ img, float* __restrict__ out, int N, long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int k = (int)(i % RNT_KP);
  const long long np = i / RNT_KP;
  const int pix = (int)(np % (32 * 32));
  const long long n = np / (32 * 32);
  float v = 0.0f;
  if (n < N && k < RNT_K) {
    const int dy = k / 21, r = k % 21, dx = r / 3, ch = r % 3;
    const int iy = 2 * (pix / 32) + dy - 3, ix = 2 * (pix % 32) + dx - 3;
    if (iy >= 0 && iy < RNT_S && ix >= 0 && ix < RNT_S) v = img[((n * RNT_S + iy) * RNT_S + ix) * 3 + ch];
  }
  out[i] = v;
}

// GroupNorm(4, eps 1e-5) over (Bp, T, C) channels-last, one work-group per (sample, group); thread tid owns elements e = tid + 256 i of the block
// (pixel e / cg, channel e % cg; cg = C / 4 divides 256, so a thread always sees the same channel).  Two-pass statistics (mean, then centred squares).
//   mode 0: y = [relu](GN(x));  1: y = [relu](GN(x) + res);  2: y = [relu](GN(x) + GN'(res)), res the raw conv_proj output with (gamma2, beta2)
// stats / stats2 [wg * 2] = {mean, rstd} of x / of res.
__device__ __forceinline__ void rnt_group_stats(const float* __restrict__ x, size_t base, int cg, int C, int cnt, float* red, float& mean, float& rstd) {
  const int tid = threadIdx.x;
  float s = 0.0f;
  for (int e = tid; e < cnt; e += 256) s += x[base + (size_t)(e / cg) * C + e % cg];
  mean = vae_block_sum(s, red) / (float)cnt;
  float q = 0.0f;
  for (int e = tid; e < cnt; e += 256) {
    const float d = x[base + (size_t)(e / cg) * C + e % cg] - mean;
    q += d * d;
  }
  rstd = 1.0f / sqrtf(vae_block_sum(q, red) / (float)cnt + RNT_EPS);
}
__global__ __launch_bounds__(256) void rnt_gn_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         const float* __restrict__ res, const float* __restrict__ gamma2, const float* __restrict__ beta2,
                                                         float* __restrict__ y, float* __restrict__ stats, float* __restrict__ stats2, int T, int C, int relu,
                                                         int mode) {
  __shared__ float red[4];
  const int n = blockIdx.x / RNT_G, g = blockIdx.x % RNT_G, cg = C / RNT_G, cnt = T * cg, tid = threadIdx.x;
  const size_t base = (size_t)n * T * C + (size_t)g * cg;
  float mean, rstd, mean2 = 0.0f, rstd2 = 0.0f;
  rnt_group_stats(x, base, cg, C, cnt, red, mean, rstd);
  if (mode == 2) rnt_group_stats(res, base, cg, C, cnt, red, mean2, rstd2);
  if (tid == 0) {
    stats[(size_t)blockIdx.x * 2] = mean;
    stats[(size_t)blockIdx.x * 2 + 1] = rstd;
    if (mode == 2) {
      stats2[(size_t)blockIdx.x * 2] = mean2;
      stats2[(size_t)blockIdx.x * 2 + 1] = rstd2;
    }
  }
  const int ch = g * cg + tid % cg;
  const float ga = gamma[ch], be = beta[ch];
  const float ga2 = mode == 2 ? gamma2[ch] : 0.0f, be2 = mode == 2 ? beta2[ch] : 0.0f;
  for (int e = tid; e < cnt; e += 256) {
    const size_t o = base + (size_t)(e / cg) * C + e % cg;
    float v = (x[o] - mean) * rstd * ga + be;
    if (mode == 1) v = res[o] + v;
    else if (mode == 2) v = ((res[o] - mean2) * rstd2 * ga2 + be2) + v;
    y[o] = relu ? fmaxf(v, 0.0f) : v;
  }
}
// backward: du = dy through the ReLU mask of the saved output y;  dxh = du gamma;  dx = rstd (dxh - mean(dxh) - xh mean(dxh xh)).
// dres: mode 1 the residual's gradient du; mode 2 the raw projection's, through its own normalisation.
// part (Bp, 2C): per sample and channel  sum_t du xh | sum_t du (scale / bias of the norm; bias of norm_proj too);  part2 (Bp, C): sum_t du rh (mode 2).
__global__ __launch_bounds__(256) void rnt_gn_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ x,
                                                         const float* __restrict__ stats, const float* __restrict__ gamma, const float* __restrict__ res,
                                                         const float* __restrict__ stats2, const float* __restrict__ gamma2, float* __restrict__ dx,
                                                         float* __restrict__ dres, float* __restrict__ part, float* __restrict__ part2, int T, int C, int relu,
                                                         int mode) {
  __shared__ float red[4];
  __shared__ float ps[3][256];
  const int n = blockIdx.x / RNT_G, g = blockIdx.x % RNT_G, cg = C / RNT_G, cnt = T * cg, tid = threadIdx.x;
  const size_t base = (size_t)n * T * C + (size_t)g * cg;
  const float mean = stats[(size_t)blockIdx.x * 2], rstd = stats[(size_t)blockIdx.x * 2 + 1];
  const float mean2 = mode == 2 ? stats2[(size_t)blockIdx.x * 2] : 0.0f, rstd2 = mode == 2 ? stats2[(size_t)blockIdx.x * 2 + 1] : 0.0f;
  const int ch = g * cg + tid % cg;
  const float ga = gamma[ch], ga2 = mode == 2 ? gamma2[ch] : 0.0f;
  float a1 = 0.0f, a2 = 0.0f, b1 = 0.0f, b2 = 0.0f, sg = 0.0f, sb = 0.0f, sg2 = 0.0f;
  for (int e = tid; e < cnt; e += 256) {
    const size_t o = base + (size_t)(e / cg) * C + e % cg;
    const float du = (!relu || y[o] > 0.0f) ? dy[o] : 0.0f;
    const float xh = (x[o] - mean) * rstd;
    const float dxh = du * ga;
    a1 += dxh;
    a2 += dxh * xh;
    sg += du * xh;
    sb += du;
    if (mode == 2) {
      const float rh = (res[o] - mean2) * rstd2;
      const float drh = du * ga2;
      b1 += drh;
      b2 += drh * rh;
      sg2 += du * rh;
    }
  }
  const float m1 = vae_block_sum(a1, red) / (float)cnt;
  const float m2 = vae_block_sum(a2, red) / (float)cnt;
  float n1 = 0.0f, n2 = 0.0f;
  if (mode == 2) {                                    // (uniform over the launch)
    n1 = vae_block_sum(b1, red) / (float)cnt;
    n2 = vae_block_sum(b2, red) / (float)cnt;
  }
  for (int e = tid; e < cnt; e += 256) {
    const size_t o = base + (size_t)(e / cg) * C + e % cg;
    const float du = (!relu || y[o] > 0.0f) ? dy[o] : 0.0f;
    const float xh = (x[o] - mean) * rstd;
    dx[o] = rstd * ((du * ga - m1) - xh * m2);
    if (mode == 1) dres[o] = du;
    else if (mode == 2) {
      const float rh = (res[o] - mean2) * rstd2;
      dres[o] = rstd2 * ((du * ga2 - n1) - rh * n2);
    }
  }
  ps[0][tid] = sg;
  ps[1][tid] = sb;
  ps[2][tid] = sg2;
  __syncthreads();
  if (tid < cg) {
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (int t2 = tid; t2 < 256; t2 += cg) {
      s0 += ps[0][t2];
      s1 += ps[1][t2];
      s2 += ps[2][t2];
    }
    part[(size_t)n * 2 * C + g * cg + tid] = s0;
    part[(size_t)n * 2 * C + C + g * cg + tid] = s1;
    if (mode == 2) part2[(size_t)n * C + g * cg + tid] = s2;
  }
}

// nn.max_pool(x, (3, 3), strides (2, 2), 'SAME') on an even side: pads (0, 1) with -inf.  x (Bp, H, H, C) -> y (Bp, H / 2, H / 2, C); one thread
// per output element.
__global__ void rnt_maxpool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long long total, int H, int C) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int Ho = H / 2, c = (int)(i % C);
  const long long p = i / C;
  const int ox = (int)(p % Ho), oy = (int)((p / Ho) % Ho);
  const long long n = p / ((long long)Ho * Ho);
  const int h1 = min(2 * oy + 2, H - 1), w1 = min(2 * ox + 2, H - 1);
  float m = -INFINITY;
  for (int hh = 2 * oy; hh <= h1; ++hh)
    for (int ww = 2 * ox; ww <= w1; ++ww) m = fmaxf(m, x[((n * H + hh) * H + ww) * C + c]);
  y[i] = m;
}
// backward, gather-style: one thread per INPUT element sums the dy of the (at most four) windows that chose it.  A window chooses the first
// position in row-major order that holds its maximum.
__global__ void rnt_maxpool_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ dx,
                                       long long total, int H, int C) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int Ho = H / 2, c = (int)(i % C);
  const long long p = i / C;
  const int ix = (int)(p % H), iy = (int)((p / H) % H);
  const long long n = p / ((long long)H * H);
  const float v = x[i];
  float g = 0.0f;
  for (int oy = (iy - 1) / 2; oy <= min(iy / 2, Ho - 1); ++oy)
    for (int ox = (ix - 1) / 2; ox <= min(ix / 2, Ho - 1); ++ox) {
      const long long o = ((n * Ho + oy) * Ho + ox) * C + c;
      if (v != y[o]) continue;
      const int ww = min(2 * ox + 2, H - 1) - 2 * ox + 1;                       // the window's width inside the map
      const int me = (iy - 2 * oy) * ww + (ix - 2 * ox);                       // this element's place in the window's row-major order
      bool first = true;
      for (int k = 0; k < me && first; ++k) first = x[((n * H + 2 * oy + k / ww) * H + 2 * ox + k % ww) * C + c] != v;
      if (first) g += dy[o];
    }
  dx[i] = g;
}

// SpatialSoftmax at temperature 1 (csrc/resnet.hip rn_ssm_kernel): x (Bp, H, W, C) -> featp (Bp, 2C) = [expected_x | expected_y], and the first
// N rows into the caller's feat_out.  One thread per (sample, channel).
__global__ void rnt_ssm_fwd_kernel(const float* __restrict__ x, float* __restrict__ featp, float* __restrict__ feat_out, int N, int Bp, int H, int W, int C) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)Bp * C) return;
  const int c = (int)(i % C);
  const long long n = i / C;
  const float* p = x + n * H * W * C + c;
  float m = p[0];
  for (int j = 1; j < H * W; ++j) m = fmaxf(m, p[(size_t)j * C]);
  float den = 0.0f;
  for (int j = 0; j < H * W; ++j) den += expf(p[(size_t)j * C] - m);
  const float sx = W > 1 ? 2.0f / (float)(W - 1) : 0.0f, sy = H > 1 ? 2.0f / (float)(H - 1) : 0.0f;
  float ex = 0.0f, ey = 0.0f;
  for (int hh = 0; hh < H; ++hh)
    for (int ww = 0; ww < W; ++ww) {
      const float pr = expf(p[(size_t)(hh * W + ww) * C] - m) / den;
      ex += (-1.0f + sx * (float)ww) * pr;
      ey += (-1.0f + sy * (float)hh) * pr;
    }
  featp[n * 2 * C + c] = ex;
  featp[n * 2 * C + C + c] = ey;
  if (n < N) {
    feat_out[n * 2 * C + c] = ex;
    feat_out[n * 2 * C + C + c] = ey;
  }
}
// backward: s = softmax(x) recomputed with the maximum subtracted;  dx_p = s_p (pos_x(p) dfx + pos_y(p) dfy - (E_x dfx + E_y dfy)).
// dfeat (N, 2C) is the caller's; the padding rows' gradient is zero.
__global__ void rnt_ssm_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dfeat, float* __restrict__ dx, int N, int Bp, int H, int W, int C) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)Bp * C) return;
  const int c = (int)(i % C);
  const long long n = i / C;
  const float* p = x + n * H * W * C + c;
  float* q = dx + n * H * W * C + c;
  if (n >= N) {
    for (int j = 0; j < H * W; ++j) q[(size_t)j * C] = 0.0f;
    return;
  }
  const float dfx = dfeat[n * 2 * C + c], dfy = dfeat[n * 2 * C + C + c];
  float m = p[0];
  for (int j = 1; j < H * W; ++j) m = fmaxf(m, p[(size_t)j * C]);
  float den = 0.0f;
  for (int j = 0; j < H * W; ++j) den += expf(p[(size_t)j * C] - m);
  const float sx = W > 1 ? 2.0f / (float)(W - 1) : 0.0f, sy = H > 1 ? 2.0f / (float)(H - 1) : 0.0f;
  float ex = 0.0f, ey = 0.0f;
  for (int hh = 0; hh < H; ++hh)
    for (int ww = 0; ww < W; ++ww) {
      const float pr = expf(p[(size_t)(hh * W + ww) * C] - m) / den;
      ex += (-1.0f + sx * (float)ww) * pr;
      ey += (-1.0f + sy * (float)hh) * pr;
    }
  const float mid = ex * dfx + ey * dfy;
  for (int hh = 0; hh < H; ++hh)
    for (int ww = 0; ww < W; ++ww) {
      const float pr = expf(p[(size_t)(hh * W + ww) * C] - m) / den;
      q[(size_t)(hh * W + ww) * C] = pr * (((-1.0f + sx * (float)ww) * dfx + (-1.0f + sy * (float)hh) * dfy) - mid);
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------
struct RntBlockDesc { int cin, cout, stride; bool proj; };
inline RntBlockDesc rnt_block(int b) {
  const int stage = b / 2, cout = RNT_F << stage, cin = b == 0 ? RNT_F : RNT_F << ((b - 1) / 2);
  const int stride = (stage > 0 && b % 2 == 0) ? 2 : 1;
  return {cin, cout, stride, stride != 1 || cin != cout};
}

// the Flax tree of weights.py resnet_shapes, in its order (60 leaves); conv_init/kernel (7, 7, 3, 64) lies as [147 -> 160][64]
void describe_encoder(Module& m) {
  m.add("conv_init/kernel", {7, 7, 3, RNT_F});
  {
    Leaf& l = m.leaves.back();
    l.taps = 1; l.rows = RNT_K; l.rows_p = RNT_KP;
    m.total = l.off + (l.size_p() + 63) / 64 * 64;
  }
  m.add("norm_init/scale", {RNT_F});
  m.add("norm_init/bias", {RNT_F});
  for (int b = 0; b < RNT_BLOCKS; ++b) {
    const RntBlockDesc d = rnt_block(b);
    const std::string p = "ResNetBlock_" + std::to_string(b);
    m.add(p + "/Conv_0/kernel", {3, 3, d.cin, d.cout});
    m.add(p + "/MyGroupNorm_0/scale", {d.cout});
    m.add(p + "/MyGroupNorm_0/bias", {d.cout});
    m.add(p + "/Conv_1/kernel", {3, 3, d.cout, d.cout});
    m.add(p + "/MyGroupNorm_1/scale", {d.cout});
    m.add(p + "/MyGroupNorm_1/bias", {d.cout});
    if (d.proj) {
      m.add(p + "/conv_proj/kernel", {1, 1, d.cin, d.cout});
      m.add(p + "/norm_proj/scale", {d.cout});
      m.add(p + "/norm_proj/bias", {d.cout});
    }
  }
}

int rnt_gn_fwd(const Ctx& c, const float* x, const float* gamma, const float* beta, const float* res, const float* gamma2, const float* beta2, float* y,
               float* stats, float* stats2, int Bp, int T, int C, int mode) {
  TK(rnt_gn_fwd_kernel, dim3(Bp * RNT_G), dim3(256), x, gamma, beta, res, gamma2, beta2, y, stats, stats2, T, C, 1, mode);
  return LDP_OK;
}
int rnt_gn_bwd(const Ctx& c, const float* dy, const float* y, const float* x, const float* stats, const float* gamma, const float* res, const float* stats2,
               const float* gamma2, float* dx, float* dres, float* part, float* part2, int Bp, int T, int C, int mode) {
  TK(rnt_gn_bwd_kernel, dim3(Bp * RNT_G), dim3(256), dy, y, x, stats, gamma, res, stats2, gamma2, dx, dres, part, part2, T, C, 1, mode);
  return LDP_OK;
}

struct RntSave {                    // what a ResNetBlock keeps for its backward
  RntBlockDesc d{};
  int Sin = 0, S = 0;
  const ConvPlan *cv1 = nullptr, *cv2 = nullptr, *cvp = nullptr;
  const float* x = nullptr;
  float *c1 = nullptr, *a1 = nullptr, *c2 = nullptr, *pr = nullptr, *y = nullptr, *st1 = nullptr, *st2 = nullptr, *stp = nullptr;
};

// One slot's tape.  backward = false: the forward is enqueued (the dry walk goes on through the backward, to size the workspace for both);
// backward = true: the forward is walked without launching (the same bump allocation: the same pointers), the backward is enqueued.
int encoder_tape(Ctx& c, const float* img, float* feat_out, const float* dfeat, int N, bool backward) {
  Trainer& t = *c.t;
  Module& m = *c.M;
  const bool real = !c.dry;
  const int Bp = rup(N, RP), CL = RNT_F << 3;                 // CL: channels of the last feature map (512)
  c.L->ws_used = 0;
  auto P = [&](const std::string& path) { return m.P.f() + m.leaf(path).off; };
  auto Gd = [&](const std::string& path) { return m.G.f() + m.leaf(path).off; };
  auto take = [&](size_t n) { return ws_take(*c.L, n); };
  int rc = LDP_OK;
#define RNT_TRY(expr) do { if ((rc = (expr)) != LDP_OK) { c.dry = !real; return rc; } } while (0)

  // ---- forward ------------------------------------------------------------------------------------------------------------------------
  c.dry = !real || backward;
  const ConvPlan& stem = vae_plan(t, VC_P1, 32, 32, RNT_KP, RNT_F);
  const long long npatch = (long long)Bp * 32 * 32 * RNT_KP;
  float* patches = take((size_t)npatch);
  TK(rnt_patch_kernel, g1(npatch), dim3(256), img, patches, N, npatch);
  const size_t n0 = (size_t)Bp * 32 * 32 * RNT_F;
  float* c0 = take(n0);
  float* a0 = take(n0);
  float* st0 = take((size_t)Bp * RNT_G * 2);
  RNT_TRY(conv_fwd(c, stem, patches, P("conv_init/kernel"), nullptr, nullptr, c0, Bp));
  RNT_TRY(rnt_gn_fwd(c, c0, P("norm_init/scale"), P("norm_init/bias"), nullptr, nullptr, nullptr, a0, st0, nullptr, Bp, 32 * 32, RNT_F, 0));
  const long long npool = (long long)Bp * 16 * 16 * RNT_F;
  float* p0 = take((size_t)npool);
  TK(rnt_maxpool_fwd_kernel, g1(npool), dim3(256), a0, p0, npool, 32, RNT_F);
  RntSave sv[RNT_BLOCKS];
  const float* x = p0;
  int S = 16;
  for (int b = 0; b < RNT_BLOCKS; ++b) {
    RntSave& B = sv[b];
    B.d = rnt_block(b);
    B.Sin = S; B.S = S / B.d.stride; B.x = x;
    const std::string p = "ResNetBlock_" + std::to_string(b);
    const int T = B.S * B.S, C = B.d.cout;
    const size_t ny = (size_t)Bp * T * C;
    B.cv1 = &vae_plan(t, B.d.stride == 1 ? VC_S1 : VC_S2, B.Sin, B.S, B.d.cin, C);
    B.cv2 = &vae_plan(t, VC_S1, B.S, B.S, C, C);
    B.c1 = take(ny); B.a1 = take(ny); B.c2 = take(ny); B.y = take(ny);
    B.st1 = take((size_t)Bp * RNT_G * 2); B.st2 = take((size_t)Bp * RNT_G * 2);
    RNT_TRY(conv_fwd(c, *B.cv1, x, P(p + "/Conv_0/kernel"), nullptr, nullptr, B.c1, Bp));
    RNT_TRY(rnt_gn_fwd(c, B.c1, P(p + "/MyGroupNorm_0/scale"), P(p + "/MyGroupNorm_0/bias"), nullptr, nullptr, nullptr, B.a1, B.st1, nullptr, Bp, T, C, 0));
    RNT_TRY(conv_fwd(c, *B.cv2, B.a1, P(p + "/Conv_1/kernel"), nullptr, nullptr, B.c2, Bp));
    if (B.d.proj) {
      B.cvp = &vae_plan(t, VC_P2, B.Sin, B.S, B.d.cin, C);
      B.pr = take(ny); B.stp = take((size_t)Bp * RNT_G * 2);
      RNT_TRY(conv_fwd(c, *B.cvp, x, P(p + "/conv_proj/kernel"), nullptr, nullptr, B.pr, Bp));
      RNT_TRY(rnt_gn_fwd(c, B.c2, P(p + "/MyGroupNorm_1/scale"), P(p + "/MyGroupNorm_1/bias"), B.pr, P(p + "/norm_proj/scale"), P(p + "/norm_proj/bias"),
                         B.y, B.st2, B.stp, Bp, T, C, 2));
    } else {
      RNT_TRY(rnt_gn_fwd(c, B.c2, P(p + "/MyGroupNorm_1/scale"), P(p + "/MyGroupNorm_1/bias"), x, nullptr, nullptr, B.y, B.st2, nullptr, Bp, T, C, 1));
    }
    x = B.y;
    S = B.S;
  }
  float* featp = take((size_t)Bp * 2 * CL);
  TK(rnt_ssm_fwd_kernel, g1((long long)Bp * CL), dim3(256), x, featp, feat_out, N, Bp, S, S, CL);
  if (real && !backward) {
    LDP_HIP(hipGetLastError());
    return LDP_OK;
  }

  // ---- backward: last block first; weight-gradient work on the side streams ----------------------------------------------------------------
  c.dry = !real;
  Ctx w;
  float* d = take((size_t)Bp * S * S * CL);
  TK(rnt_ssm_bwd_kernel, g1((long long)Bp * CL), dim3(256), x, dfeat, d, N, Bp, S, S, CL);
  for (int b = RNT_BLOCKS - 1; b >= 0; --b) {
    const RntSave& B = sv[b];
    const std::string p = "ResNetBlock_" + std::to_string(b);
    const int T = B.S * B.S, C = B.d.cout;
    const size_t ny = (size_t)Bp * T * C, nx = (size_t)Bp * B.Sin * B.Sin * B.d.cin;
    float* dc2 = take(ny);
    float* dres = take(ny);                                     // d x (identity residual) or d conv_proj output
    float* part2 = take((size_t)Bp * 2 * C);
    float* partp = B.d.proj ? take((size_t)Bp * C) : nullptr;
    RNT_TRY(rnt_gn_bwd(c, d, B.y, B.c2, B.st2, P(p + "/MyGroupNorm_1/scale"), B.d.proj ? B.pr : nullptr, B.stp, B.d.proj ? P(p + "/norm_proj/scale") : nullptr,
                       dc2, dres, part2, partp, Bp, T, C, B.d.proj ? 2 : 1));
    RNT_TRY(fork(c, &w));                                        // dc2, dres and the partials exist
    RNT_TRY(colsum_to(w, part2, 2 * C, Bp, 2 * C, ColOut{{Gd(p + "/MyGroupNorm_1/scale"), Gd(p + "/MyGroupNorm_1/bias"), nullptr}, C}));
    RNT_TRY(conv_wgrad(w, *B.cv2, B.a1, dc2, Gd(p + "/Conv_1/kernel"), Bp));
    if (B.d.proj) {
      RNT_TRY(colsum(w, partp, C, Bp, C, Gd(p + "/norm_proj/scale")));
      RNT_TRY(colsum(w, part2 + C, 2 * C, Bp, C, Gd(p + "/norm_proj/bias")));      // the two norms share the pre-activation: the same bias gradient
      RNT_TRY(conv_wgrad(w, *B.cvp, B.x, dres, Gd(p + "/conv_proj/kernel"), Bp));
    }
    float* da1 = take(ny);
    RNT_TRY(conv_dgrad(c, *B.cv2, dc2, P(p + "/Conv_1/kernel"), nullptr, da1, Bp));
    float* dc1 = take(ny);
    float* part1 = take((size_t)Bp * 2 * C);
    RNT_TRY(rnt_gn_bwd(c, da1, B.a1, B.c1, B.st1, P(p + "/MyGroupNorm_0/scale"), nullptr, nullptr, nullptr, dc1, nullptr, part1, nullptr, Bp, T, C, 0));
    RNT_TRY(fork(c, &w));
    RNT_TRY(colsum_to(w, part1, 2 * C, Bp, 2 * C, ColOut{{Gd(p + "/MyGroupNorm_0/scale"), Gd(p + "/MyGroupNorm_0/bias"), nullptr}, C}));
    RNT_TRY(conv_wgrad(w, *B.cv1, B.x, dc1, Gd(p + "/Conv_0/kernel"), Bp));
    float* dx = take(nx);
    if (B.d.proj) {
      RNT_TRY(conv_dgrad(c, *B.cvp, dres, P(p + "/conv_proj/kernel"), nullptr, dx, Bp));      // (zero at the pixels the stride skips)
      RNT_TRY(conv_dgrad(c, *B.cv1, dc1, P(p + "/Conv_0/kernel"), dx, dx, Bp));
    } else {
      RNT_TRY(conv_dgrad(c, *B.cv1, dc1, P(p + "/Conv_0/kernel"), dres, dx, Bp));
    }
    d = dx;
  }
  float* da0 = take(n0);
  TK(rnt_maxpool_bwd_kernel, g1((long long)n0), dim3(256), d, a0, p0, da0, (long long)n0, 32, RNT_F);
  float* dc0 = take(n0);
  float* part0 = take((size_t)Bp * 2 * RNT_F);
  RNT_TRY(rnt_gn_bwd(c, da0, a0, c0, st0, P("norm_init/scale"), nullptr, nullptr, nullptr, dc0, nullptr, part0, nullptr, Bp, 32 * 32, RNT_F, 0));
  RNT_TRY(fork(c, &w, 1, 1));
  RNT_TRY(colsum_to(w, part0, 2 * RNT_F, Bp, 2 * RNT_F, ColOut{{Gd("norm_init/scale"), Gd("norm_init/bias"), nullptr}, RNT_F}));
  RNT_TRY(conv_wgrad(w, stem, patches, dc0, Gd("conv_init/kernel"), Bp));
  RNT_TRY(flush_colsums(w));
#undef RNT_TRY
  if (real) LDP_HIP(hipGetLastError());
  return LDP_OK;
}
