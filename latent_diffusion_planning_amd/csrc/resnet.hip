// resnet.hip -- the image encoder of the diffusion-policy baseline (DPAgent): ResNetEncoder (networks/resnet_v1.py:237-346) as configured by
// agent/encoder/bridge_resnet.yaml -- ResNet-18, GroupNorm(4, eps 1e-5), ReLU, spatial-softmax pooling, no bias anywhere:
//   ldp_resnet_encode: img (N, 64, 64, 3) NHWC in [-1, 1] -> (N, 1024) = [expected_x (512) | expected_y (512)]
// Every product is exact fp32: the features are the condition of a 100-step recurrence.  The 7x7 stride-2 stem and the 1x1 stride-2
// projections are implicit GEMMs on v_mfma_f32_16x16x4f32 written here; the sixteen 3x3 convolutions have the tap geometry of the
// StableVAE's (stride 1 pad 1; stride 2 pad (0, 1)) and run on its tiles (tconv.hpp MODE_K3H / MODE_K3S) with a zero bias.  GroupNorm is
// one work-group per (sample, group), two passes (mean, then centred squares: a group with a large mean keeps its variance), with ReLU,
// the residual add and -- for the projected blocks -- the residual's own GroupNorm fused: a block is four launches plus its projection
// conv.  No atomics; every reduction has a fixed order, so two runs give the same bits.
#include "engine.hpp"

#include <algorithm>

namespace ldp {

namespace {

constexpr int RN_SLOTS = 4;             // encoders per handle (weight modules encoder0 .. encoder3)
constexpr int RN_CHUNK = 64;            // frames per pass: bounds the workspace (two buffers of 256 KB and three of 64 KB per frame: 44 MB)
constexpr int RN_S = 64, RN_F = 64;     // frame side, n_filters
constexpr int RN_GROUPS = 4;
constexpr float RN_EPS = 1e-5f;
constexpr int RN_STAGES = 4, RN_BLOCKS = 8;

// ---------------------------------------------------------------------------------------------
// conv_init: 7x7, stride 2, pad 3, 3 -> 64 channels, 64 -> 32 pixels.  Implicit GEMM with K = 7 * 7 * 3 = 147 (padded to 148 = 37 MFMA k
// steps): a work-group (4 waves) owns ST_ROWS output rows of one frame and stages their 2 ST_ROWS + 5 input rows (3 zero pixels either
// side) in LDS once; wave w owns output channels 16 w .. 16 w + 15 and keeps its 37 B fragments in registers for the whole work-group.
// The virtual K index is the Flax kernel's own flattening k = (dy * 7 + dx) * 3 + c = dy * 21 + (dx * 3 + c), and dx * 3 + c is
// contiguous in a staged row: the A element of (output pixel ox, k) is rows[2 r + dy][6 ox + k % 21].
constexpr int ST_ROWS = 4, ST_KS = 37, ST_K = 147;
constexpr int ST_RW = (RN_S + 6) * 3;               // floats per staged row
constexpr int ST_NR = 2 * ST_ROWS + 5;              // staged input rows
__global__ __launch_bounds__(256) void rn_stem_kernel(const float* __restrict__ img, const float* __restrict__ wp,
                                                       float* __restrict__ y, int N) {
  __shared__ float rows[(ST_NR + 1) * ST_RW];       // one more (zero) row: the padded k = 147 of the last output row points into it
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  const int bpf = (RN_S / 2) / ST_ROWS;             // work-groups per frame
  const int64_t n = blockIdx.x / bpf;
  const int oy0 = (blockIdx.x % bpf) * ST_ROWS;
  for (int i = tid; i < (ST_NR + 1) * ST_RW; i += 256) {
    const int r = i / ST_RW, j = i % ST_RW, ix = j / 3 - 3, iy = 2 * oy0 - 3 + r;
    float v = 0.0f;
    if (r < ST_NR && iy >= 0 && iy < RN_S && ix >= 0 && ix < RN_S) v = img[((n * RN_S + iy) * RN_S + ix) * 3 + j % 3];
    rows[i] = v;
  }
  float breg[ST_KS];
  int aoff[ST_KS];
#pragma unroll
  for (int ks = 0; ks < ST_KS; ++ks) {
    breg[ks] = wp[((size_t)wave * ST_KS + ks) * 64 + lane];
    const int k = 4 * ks + fk;
    aoff[ks] = (k / 21) * ST_RW + k % 21;
  }
  __syncthreads();
  for (int rr = 0; rr < ST_ROWS; ++rr) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const float* ap = rows + 2 * rr * ST_RW + 6 * (mt * 16 + fr);
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < ST_KS; ++ks) {
        float a = ap[aoff[ks]];
        if (ks == ST_KS - 1 && 4 * ks + fk >= ST_K) a = 0.0f;           // the padded k: whatever the staged pixel holds, the product is 0
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, breg[ks], acc, 0, 0, 0);
      }
      float* o = y + ((n * (RN_S / 2) + oy0 + rr) * (RN_S / 2) + mt * 16 + 4 * fk) * RN_F + wave * 16 + fr;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[(size_t)e * RN_F] = acc[e];
    }
  }
}

// Flax (7, 7, 3, 64) -> [wave][k step][lane]: lane (fr, fk) of wave w holds W[k = 4 ks + fk][16 w + fr], zero at k = 147
std::vector<float> pack_stem(const float* k) {
  std::vector<float> p((size_t)4 * ST_KS * 64, 0.f);
  for (int w = 0; w < 4; ++w)
    for (int ks = 0; ks < ST_KS; ++ks)
      for (int l = 0; l < 64; ++l) {
        const int kk = 4 * ks + (l >> 4);
        if (kk < ST_K) p[((size_t)w * ST_KS + ks) * 64 + l] = k[(size_t)kk * RN_F + w * 16 + (l & 15)];
      }
  return p;
}

int stem_launch(const float* img, const float* wp, float* y, int N, hipStream_t s) {
  hipLaunchKernelGGL(rn_stem_kernel, dim3((unsigned)(N * ((RN_S / 2) / ST_ROWS))), dim3(256), 0, s, img, wp, y, N);
  LDP_HIP(hipGetLastError());
  return LDP_OK;
}

// ---------------------------------------------------------------------------------------------
// conv_proj: 1x1, stride 2, no padding: y(n, oy, ox, :) = x(n, 2 oy, 2 ox, :) @ W (Cin, Cout).  A work-group owns 16 MT output pixels x 64
// columns: the gathered pixel rows are staged in LDS (row stride Cin + 1: the 16 rows of a fragment fall into 16 banks), wave w owns columns
// 16 w .. 16 w + 15 and reads its B fragments from the Flax kernel as it lies (16 lanes = 64 contiguous bytes).  Rows past M are staged as
// zeros and not stored.
template <int MT>
__global__ __launch_bounds__(256) void rn_proj_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y,
                                                       int M, int Ho, int Wo, int Cin, int Cout) {
  extern __shared__ float As[];                     // [16 MT][Cin + 1]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  const int lds = Cin + 1;
  const int m0 = blockIdx.x * 16 * MT, col = blockIdx.y * 64 + wave * 16 + fr;
  for (int i = tid; i < 16 * MT * Cin; i += 256) {
    const int r = i / Cin, k = i - r * Cin, m = m0 + r;
    float v = 0.0f;
    if (m < M) {
      const int ox = m % Wo, oy = (m / Wo) % Ho;
      const int64_t n = m / (Wo * Ho);
      v = x[((n * 2 * Ho + 2 * oy) * 2 * Wo + 2 * ox) * Cin + k];
    }
    As[r * lds + k] = v;
  }
  __syncthreads();
  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k = fk; k < Cin; k += 4) {
    const float b = w[(size_t)k * Cout + col];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(As[(mt * 16 + fr) * lds + k], b, acc[mt], 0, 0, 0);
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int m = m0 + mt * 16 + 4 * fk + e;
      if (m < M) y[(size_t)m * Cout + col] = acc[mt][e];
    }
}

// x (N, H, W, Cin) -> y (N, H / 2, W / 2, Cout); w: the Flax (1, 1, Cin, Cout) kernel on the device
int proj_launch(const float* x, const float* w, float* y, int N, int H, int W, int Cin, int Cout, hipStream_t s) {
  if (H % 2 || W % 2 || Cin % 4 || Cout % 64 || Cin > 512 || Cin < 4)
    return fail(LDP_EINVAL, "1x1 stride-2 conv: even sides, Cin a multiple of 4 up to 512 and Cout a multiple of 64 (got %d x %d, %d -> %d)", H, W, Cin, Cout);
  const int Ho = H / 2, Wo = W / 2;
  const int64_t M64 = (int64_t)N * Ho * Wo;
  if (M64 > (1 << 30)) return fail(LDP_EINVAL, "1x1 stride-2 conv: %lld output pixels", (long long)M64);
  const int M = (int)M64;
  if (Cin <= 256) {
    hipLaunchKernelGGL(rn_proj_kernel<2>, dim3((M + 31) / 32, Cout / 64), dim3(256), (size_t)32 * (Cin + 1) * 4, s, x, w, y, M, Ho, Wo, Cin, Cout);
  } else {
    hipLaunchKernelGGL(rn_proj_kernel<1>, dim3((M + 15) / 16, Cout / 64), dim3(256), (size_t)16 * (Cin + 1) * 4, s, x, w, y, M, Ho, Wo, Cin, Cout);
  }
  LDP_HIP(hipGetLastError());
  return LDP_OK;
}

// ---------------------------------------------------------------------------------------------
// nn.max_pool(x, (3, 3), strides (2, 2), 'SAME') on an even side: pads (0, 1) with -inf, i.e. output (y, x) is the maximum over rows
// 2y .. min(2y + 2, H - 1) and columns 2x .. min(2x + 2, W - 1).  One thread per (pixel, channel quad).
__global__ void rn_maxpool_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t total4, int H, int W, int C) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total4) return;
  const int cq = C / 4, Ho = H / 2, Wo = W / 2;
  const int q = (int)(i % cq);
  const int64_t p = i / cq;
  const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho);
  const int64_t n = p / ((int64_t)Wo * Ho);
  const int h1 = min(2 * oy + 2, H - 1), w1 = min(2 * ox + 2, W - 1);
  float4 m = *reinterpret_cast<const float4*>(x + ((n * H + 2 * oy) * W + 2 * ox) * C + q * 4);
  for (int hh = 2 * oy; hh <= h1; ++hh)
    for (int ww = 2 * ox; ww <= w1; ++ww) {
      const float4 v = *reinterpret_cast<const float4*>(x + ((n * H + hh) * W + ww) * C + q * 4);
      m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
    }
  reinterpret_cast<float4*>(y)[i] = m;
}

int maxpool_launch(const float* x, float* y, int N, int H, int W, int C, hipStream_t s) {
  if (H % 2 || W % 2 || C % 4 || H < 2 || W < 2) return fail(LDP_EINVAL, "max-pool: even sides and a multiple of 4 channels (got %d x %d x %d)", H, W, C);
  const int64_t t4 = (int64_t)N * (H / 2) * (W / 2) * (C / 4);
  hipLaunchKernelGGL(rn_maxpool_kernel, dim3((unsigned)((t4 + 255) / 256)), dim3(256), 0, s, x, y, t4, H, W, C);
  LDP_HIP(hipGetLastError());
  return LDP_OK;
}

// ---------------------------------------------------------------------------------------------
// GroupNorm: one work-group per (sample, group).  Sum over the work-group in a fixed order: lanes by xor-shuffle, waves in order.
__device__ __forceinline__ float rn_block_sum(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();                                  // `red` may still be read from the sum before
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.0f;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
  return t;
}

// (mean, 1 / sqrt(var + eps)) of one group: base = first element of (sample, group), tot4 float4s at (pixel e / c4, quad e % c4)
__device__ __forceinline__ void rn_group_stats(const float* base, int tot4, int c4, int C, float eps, float* red, float& mean, float& rstd) {
  float s = 0.0f;
  for (int e = threadIdx.x; e < tot4; e += blockDim.x) {
    const float4 v = *reinterpret_cast<const float4*>(base + (size_t)(e / c4) * C + (e % c4) * 4);
    s += (v.x + v.y) + (v.z + v.w);
  }
  const float inv = 1.0f / (4.0f * (float)tot4);
  mean = rn_block_sum(s, red) * inv;
  float s2 = 0.0f;
  for (int e = threadIdx.x; e < tot4; e += blockDim.x) {
    const float4 v = *reinterpret_cast<const float4*>(base + (size_t)(e / c4) * C + (e % c4) * 4);
    const float a = v.x - mean, b = v.y - mean, c = v.z - mean, d = v.w - mean;
    s2 += (a * a + b * b) + (c * c + d * d);
  }
  rstd = 1.0f / sqrtf(rn_block_sum(s2, red) * inv + eps);
}

// y = [relu]( GN(x) [+ res | + GN'(res)] ); mode 0: no residual, 1: res added as it is, 2: res normalised with (scale2, bias2) first.
// y may be x (every element is read and written by the same thread, after the statistics).
__global__ __launch_bounds__(256) void rn_gn_kernel(const float* x, const float* res, float* y, const float* __restrict__ scale,
                                                     const float* __restrict__ bias, const float* __restrict__ scale2,
                                                     const float* __restrict__ bias2, int HW, int C, int G, float eps, int relu, int mode) {
  __shared__ float red[4];
  const int n = blockIdx.x / G, g = blockIdx.x % G, cpg = C / G, c4 = cpg / 4, tot4 = HW * c4;
  const size_t off = (size_t)n * HW * C + (size_t)g * cpg;
  float mean, rstd, mean2 = 0.0f, rstd2 = 0.0f;
  rn_group_stats(x + off, tot4, c4, C, eps, red, mean, rstd);
  if (mode == 2) rn_group_stats(res + off, tot4, c4, C, eps, red, mean2, rstd2);
  for (int e = threadIdx.x; e < tot4; e += blockDim.x) {
    const int q = e % c4;
    const size_t at = off + (size_t)(e / c4) * C + q * 4;
    const int c = g * cpg + q * 4;
    const float4 v = *reinterpret_cast<const float4*>(x + at);
    const float4 sc = *reinterpret_cast<const float4*>(scale + c), bi = *reinterpret_cast<const float4*>(bias + c);
    float4 o;
    o.x = (v.x - mean) * (rstd * sc.x) + bi.x; o.y = (v.y - mean) * (rstd * sc.y) + bi.y;
    o.z = (v.z - mean) * (rstd * sc.z) + bi.z; o.w = (v.w - mean) * (rstd * sc.w) + bi.w;
    if (mode != 0) {
      float4 r = *reinterpret_cast<const float4*>(res + at);
      if (mode == 2) {
        const float4 s2 = *reinterpret_cast<const float4*>(scale2 + c), b2 = *reinterpret_cast<const float4*>(bias2 + c);
        r.x = (r.x - mean2) * (rstd2 * s2.x) + b2.x; r.y = (r.y - mean2) * (rstd2 * s2.y) + b2.y;
        r.z = (r.z - mean2) * (rstd2 * s2.z) + b2.z; r.w = (r.w - mean2) * (rstd2 * s2.w) + b2.w;
      }
      o.x = r.x + o.x; o.y = r.y + o.y; o.z = r.z + o.z; o.w = r.w + o.w;
    }
    if (relu) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
    *reinterpret_cast<float4*>(y + at) = o;
  }
}

int gn_launch(const float* x, const float* res, float* y, const float* scale, const float* bias, const float* scale2, const float* bias2,
              int N, int HW, int C, int G, float eps, int relu, hipStream_t s) {
  if (G < 1 || C % (4 * G) != 0 || HW < 1) return fail(LDP_EINVAL, "GroupNorm: %d channels in %d groups (a group must be a multiple of 4 channels)", C, G);
  if ((int64_t)N * G > (1 << 30) || (int64_t)HW * (C / G) > (1 << 30)) return fail(LDP_EINVAL, "GroupNorm: too large");
  if (scale2 && !res) return fail(LDP_EINVAL, "GroupNorm: a second scale / bias pair needs the raw residual");
  const int mode = !res ? 0 : scale2 ? 2 : 1;
  hipLaunchKernelGGL(rn_gn_kernel, dim3((unsigned)(N * G)), dim3(256), 0, s, x, res, y, scale, bias, scale2, bias2, HW, C, G, eps, relu, mode);
  LDP_HIP(hipGetLastError());
  return LDP_OK;
}

// ---------------------------------------------------------------------------------------------
// SpatialSoftmax (temperature 1): per (sample, channel) a softmax over the H W positions (maximum subtracted first), then
// expected_x = sum pos_x p with pos_x = linspace(-1, 1)[column w], expected_y = sum pos_y p with pos_y = linspace(-1, 1)[row h]
// (jnp.meshgrid's 'xy' indexing over the h W + w flattening).  out (N, 2 C) = [expected_x | expected_y].  One thread per (sample, channel).
__global__ void rn_ssm_kernel(const float* __restrict__ x, float* __restrict__ out, int N, int H, int W, int C) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)N * C) return;
  const int c = (int)(i % C);
  const int64_t n = i / C;
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
  out[n * 2 * C + c] = ex;
  out[n * 2 * C + C + c] = ey;
}

int ssm_launch(const float* x, float* out, int N, int H, int W, int C, hipStream_t s) {
  if (H < 1 || W < 1 || C < 1 || (int64_t)H * W > 4096) return fail(LDP_EINVAL, "spatial softmax: %d x %d x %d", H, W, C);
  const int64_t t = (int64_t)N * C;
  hipLaunchKernelGGL(rn_ssm_kernel, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, s, x, out, N, H, W, C);
  LDP_HIP(hipGetLastError());
  return LDP_OK;
}

// ---------------------------------------------------------------------------------------------
// state
// ---------------------------------------------------------------------------------------------
struct RnGn { DevBuf scale, bias; };
struct RnBlock {
  DevBuf w1, w2, wp;                 // 3x3 kernels in the Toeplitz packing of the StableVAE's convs; conv_proj in Flax layout
  RnGn n1, n2, np;
  bool proj = false;
  int cin = 0, cout = 0, stride = 1;
};
struct RnSlot {
  bool ready = false;
  DevBuf stem;
  RnGn n0;
  RnBlock blk[RN_BLOCKS];
};
struct RnState {
  RnSlot slot[RN_SLOTS];
  DevBuf zero;                       // the 3x3 tiles add a bias: 512 zeros
  int ws_n = 0;
  DevBuf big0, big1, sm0, sm1, sm2;  // ping-pong buffers of one chunk
};

RnState* R(ldp_handle* h) { return static_cast<RnState*>(h->resnet); }

int load_vec(ldp_handle* h, const std::string& path, int n, DevBuf& out) {
  const HostTensor* t = nullptr;
  LDP_TRY(get_weight(h, path, &t, {n}));
  return upload(out, t->data.data(), (size_t)n * 4, nullptr);
}
int load_gn(ldp_handle* h, const std::string& p, int c, RnGn& g) {
  LDP_TRY(load_vec(h, p + "/scale", c, g.scale));
  return load_vec(h, p + "/bias", c, g.bias);
}
// (3, 3, Cin, Cout) -> taps along W, the three image rows folded into K: W'[dw][dh * Cin + c][co] = W[dh][dw][c][co]
std::vector<float> pack3(const float* k, int cin, int cout) {
  std::vector<float> tmp((size_t)9 * cin * cout);
  for (int dh = 0; dh < 3; ++dh)
    for (int dw = 0; dw < 3; ++dw)
      std::copy(k + ((size_t)dh * 3 + dw) * cin * cout, k + ((size_t)dh * 3 + dw + 1) * cin * cout, tmp.begin() + ((size_t)dw * 3 + dh) * cin * cout);
  return pack_conv(tmp.data(), 3, 3 * cin, cout, 3 * cin, cout);
}
int load_conv3(ldp_handle* h, const std::string& p, int cin, int cout, DevBuf& out) {
  const HostTensor* k = nullptr;
  LDP_TRY(get_weight(h, p + "/kernel", &k, {3, 3, cin, cout}));
  const std::vector<float> packed = pack3(k->data.data(), cin, cout);
  return upload(out, packed.data(), packed.size() * 4, nullptr);
}

int load_slot(ldp_handle* h, int i, RnSlot& S) {
  const std::string e = "encoder" + std::to_string(i) + "/";
  S.ready = false;
  {
    const HostTensor* k = nullptr;
    LDP_TRY(get_weight(h, e + "conv_init/kernel", &k, {7, 7, 3, RN_F}));
    const std::vector<float> p = pack_stem(k->data.data());
    LDP_TRY(upload(S.stem, p.data(), p.size() * 4, nullptr));
  }
  LDP_TRY(load_gn(h, e + "norm_init", RN_F, S.n0));
  int cin = RN_F;
  for (int b = 0; b < RN_BLOCKS; ++b) {
    RnBlock& B = S.blk[b];
    const int stage = b / 2;
    B.cin = cin; B.cout = RN_F << stage; B.stride = (stage > 0 && b % 2 == 0) ? 2 : 1;
    B.proj = B.stride != 1 || B.cin != B.cout;
    const std::string p = e + "ResNetBlock_" + std::to_string(b);
    LDP_TRY(load_conv3(h, p + "/Conv_0", B.cin, B.cout, B.w1));
    LDP_TRY(load_gn(h, p + "/MyGroupNorm_0", B.cout, B.n1));
    LDP_TRY(load_conv3(h, p + "/Conv_1", B.cout, B.cout, B.w2));
    LDP_TRY(load_gn(h, p + "/MyGroupNorm_1", B.cout, B.n2));
    if (B.proj) {
      const HostTensor* k = nullptr;
      LDP_TRY(get_weight(h, p + "/conv_proj/kernel", &k, {1, 1, B.cin, B.cout}));
      LDP_TRY(upload(B.wp, k->data.data(), k->data.size() * 4, nullptr));
      LDP_TRY(load_gn(h, p + "/norm_proj", B.cout, B.np));
    }
    cin = B.cout;
  }
  S.ready = true;
  return LDP_OK;
}

int workspace(RnState& S, int n) {
  if (n <= S.ws_n) return LDP_OK;
  const size_t big = (size_t)n * (RN_S / 2) * (RN_S / 2) * RN_F * 4, sm = big / 4;     // the stem's output; everything from the max-pool on
  LDP_TRY(S.big0.alloc(big)); LDP_TRY(S.big1.alloc(big));
  LDP_TRY(S.sm0.alloc(sm)); LDP_TRY(S.sm1.alloc(sm)); LDP_TRY(S.sm2.alloc(sm));
  S.ws_n = n;
  return LDP_OK;
}

// 3x3 conv without bias on the StableVAE's exact-fp32 tiles: (N, H, H, cin) -> (N, H / stride, H / stride, cout)
int conv3(ldp_handle* h, const float* w, const float* zero, const float* x, float* y, int N, int H, int cin, int cout, int stride, hipStream_t s) {
  const int Ho = H / stride;
  const int to = Ho % 8 == 0 ? 8 : Ho % 4 == 0 ? 4 : Ho % 2 == 0 ? 2 : 0;
  if (to == 0) return fail(LDP_EINVAL, "unsupported image width %d for the 3x3 conv tiles", Ho);
  ConvPlan p{stride == 1 ? MODE_K3H : MODE_K3S, to, 2, 4, 1, 0};
  if (to == 8) { p.nwn = 4; p.ks = 1; p.cpi = 2; }           // 64-column four-wave tiles (cin and cout are multiples of 64 here)
  if (cin % p.chunk() != 0 || cout % p.bn() != 0)
    return fail(LDP_EINVAL, "3x3 conv %d->%d does not tile (chunk %d, block %d)", cin, cout, p.chunk(), p.bn());
  ConvArgs a{};
  a.xa = x; a.ca = cin; a.w = w; a.bias = zero; a.out = y; a.cout = cout;
  a.h_out = Ho; a.w_tiles = Ho / to; a.h_in = H; a.w_in = H;
  a.B = N * Ho * a.w_tiles; a.rows_valid = a.B * to;
  const int r = tconv_launch(p, a, s);
  if (r != 0) return fail(r == -100 ? LDP_EINVAL : LDP_EHIP, "3x3 conv launch failed (%d)", r);
  return LDP_OK;
}

// One chunk.  Launches: stem, GroupNorm + ReLU, max-pool; per block conv, GroupNorm + ReLU, conv, [projection conv,] GroupNorm + residual
// (+ its GroupNorm) + ReLU; spatial softmax: 3 + 8 * 4 + 3 + 1 = 39.
int encode_chunk(ldp_handle* h, RnState& S, const RnSlot& E, const float* img, float* out, int n, hipStream_t s) {
  LDP_TRY(workspace(S, n));
  const float* zero = S.zero.f();
  LDP_TRY(stem_launch(img, E.stem.f(), S.big0.f(), n, s));
  LDP_TRY(gn_launch(S.big0.f(), nullptr, S.big1.f(), E.n0.scale.f(), E.n0.bias.f(), nullptr, nullptr, n, 32 * 32, RN_F, RN_GROUPS, RN_EPS, 1, s));
  float *cur = S.sm0.f(), *t0 = S.sm1.f(), *t1 = S.sm2.f();
  LDP_TRY(maxpool_launch(S.big1.f(), cur, n, 32, 32, RN_F, s));
  int H = 16;
  for (int b = 0; b < RN_BLOCKS; ++b) {
    const RnBlock& B = E.blk[b];
    const int Ho = H / B.stride, HW = Ho * Ho;
    LDP_TRY(conv3(h, B.w1.f(), zero, cur, t0, n, H, B.cin, B.cout, B.stride, s));
    LDP_TRY(gn_launch(t0, nullptr, t0, B.n1.scale.f(), B.n1.bias.f(), nullptr, nullptr, n, HW, B.cout, RN_GROUPS, RN_EPS, 1, s));
    LDP_TRY(conv3(h, B.w2.f(), zero, t0, t1, n, Ho, B.cout, B.cout, 1, s));
    if (B.proj) {
      float* pr = S.big0.f();                                 // the stem's buffer is free from the max-pool on
      LDP_TRY(proj_launch(cur, B.wp.f(), pr, n, H, H, B.cin, B.cout, s));
      LDP_TRY(gn_launch(t1, pr, t1, B.n2.scale.f(), B.n2.bias.f(), B.np.scale.f(), B.np.bias.f(), n, HW, B.cout, RN_GROUPS, RN_EPS, 1, s));
    } else {
      LDP_TRY(gn_launch(t1, cur, t1, B.n2.scale.f(), B.n2.bias.f(), nullptr, nullptr, n, HW, B.cout, RN_GROUPS, RN_EPS, 1, s));
    }
    std::swap(cur, t1);
    H = Ho;
  }
  return ssm_launch(cur, out, n, H, H, RN_F << (RN_STAGES - 1), s);
}

}  // namespace

int resnet_finalize(ldp_handle* h, hipStream_t s) {
  if (!h->resnet) h->resnet = new RnState();
  RnState& S = *R(h);
  if (!S.zero.p) {
    LDP_TRY(S.zero.alloc(512 * 4));
    LDP_HIP(hipMemset(S.zero.p, 0, 512 * 4));
  }
  int loaded = 0;
  for (int i = 0; i < RN_SLOTS; ++i) {
    const std::string pre = "encoder" + std::to_string(i) + "/";
    auto it = h->weights.lower_bound(pre);
    if (it == h->weights.end() || it->first.compare(0, pre.size(), pre) != 0) continue;      // a slot without leaves stays empty
    ++loaded;
    if (S.slot[i].ready) continue;                      // no leaf of it was set since it was packed (ldp_set_weight un-readies a slot)
    LDP_TRY(load_slot(h, i, S.slot[i]));
  }
  if (!loaded) return fail(LDP_ESTATE, "no encoder<i>/... weight was ever set");
  LDP_HIP(hipStreamSynchronize(s));
  return LDP_OK;
}

void resnet_invalidate(ldp_handle* h, int slot) {
  if (h->resnet && slot >= 0 && slot < RN_SLOTS) R(h)->slot[slot].ready = false;
}

void resnet_destroy(ldp_handle* h) {
  delete R(h);
  h->resnet = nullptr;
}

}  // namespace ldp

using namespace ldp;

extern "C" {

int ldp_resnet_encode(ldp_handle* h, int32_t slot, const float* img, float* feat_out, int32_t N, void* stream) {
  if (!h || !img || !feat_out || N <= 0) return fail(LDP_EINVAL, "bad argument");
  if (slot < 0 || slot >= RN_SLOTS) return fail(LDP_EINVAL, "encoder slot %d: a handle has slots 0..%d", slot, RN_SLOTS - 1);
  if (!h->resnet || !R(h)->slot[slot].ready) return fail(LDP_ESTATE, "encoder%d weights not finalized", slot);
  LDP_TRY(entry_fault_check(h));
  RnState& S = *R(h);
  const int FO = 2 * (RN_F << (RN_STAGES - 1));
  for (int n0 = 0; n0 < N; n0 += RN_CHUNK)
    LDP_TRY(encode_chunk(h, S, S.slot[slot], img + (size_t)n0 * RN_S * RN_S * 3, feat_out + (size_t)n0 * FO, std::min(RN_CHUNK, N - n0),
                         (hipStream_t)stream));
  return LDP_OK;
}

// ---- unit-testable primitives: host weights in Flax layout, device tensors; each synchronises `stream` ----
int ldp_resnet_conv7x7_s2_f32(const float* x, const float* kernel_host, float* y, int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                              void* stream) {
  if (!x || !kernel_host || !y || N <= 0) return fail(LDP_EINVAL, "bad argument");
  if (H != RN_S || W != RN_S || Cin != 3 || Cout != RN_F)
    return fail(LDP_EINVAL, "the stem is built for (N, 64, 64, 3) frames and 64 output channels (got %d x %d x %d -> %d)", H, W, Cin, Cout);
  hipStream_t s = (hipStream_t)stream;
  const std::vector<float> p = pack_stem(kernel_host);
  DevBuf w;
  LDP_TRY(upload(w, p.data(), p.size() * 4, s));
  LDP_TRY(stem_launch(x, w.f(), y, N, s));
  LDP_HIP(hipStreamSynchronize(s));
  return LDP_OK;
}

int ldp_resnet_conv1x1_s2_f32(const float* x, const float* kernel_host, float* y, int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                              void* stream) {
  if (!x || !kernel_host || !y || N <= 0 || Cin <= 0 || Cout <= 0) return fail(LDP_EINVAL, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  DevBuf w;
  LDP_TRY(upload(w, kernel_host, (size_t)Cin * Cout * 4, s));
  LDP_TRY(proj_launch(x, w.f(), y, N, H, W, Cin, Cout, s));
  LDP_HIP(hipStreamSynchronize(s));
  return LDP_OK;
}

int ldp_resnet_maxpool3x3_s2_f32(const float* x, float* y, int32_t N, int32_t H, int32_t W, int32_t C, void* stream) {
  if (!x || !y || N <= 0) return fail(LDP_EINVAL, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  LDP_TRY(maxpool_launch(x, y, N, H, W, C, s));
  LDP_HIP(hipStreamSynchronize(s));
  return LDP_OK;
}

int ldp_resnet_gn_f32(const float* x, const float* res, float* y, const float* scale_host, const float* bias_host, const float* scale2_host,
                      const float* bias2_host, int32_t N, int32_t HW, int32_t C, int32_t groups, float eps, int32_t relu, void* stream) {
  if (!x || !y || !scale_host || !bias_host || N <= 0 || C <= 0) return fail(LDP_EINVAL, "bad argument");
  if ((scale2_host == nullptr) != (bias2_host == nullptr)) return fail(LDP_EINVAL, "the second scale and bias come as a pair");
  hipStream_t s = (hipStream_t)stream;
  DevBuf sc, bi, sc2, bi2;
  LDP_TRY(upload(sc, scale_host, (size_t)C * 4, s));
  LDP_TRY(upload(bi, bias_host, (size_t)C * 4, s));
  if (scale2_host) {
    LDP_TRY(upload(sc2, scale2_host, (size_t)C * 4, s));
    LDP_TRY(upload(bi2, bias2_host, (size_t)C * 4, s));
  }
  LDP_TRY(gn_launch(x, res, y, sc.f(), bi.f(), scale2_host ? sc2.f() : nullptr, scale2_host ? bi2.f() : nullptr, N, HW, C, groups, eps,
                    relu != 0, s));
  LDP_HIP(hipStreamSynchronize(s));
  return LDP_OK;
}

int ldp_resnet_spatial_softmax_f32(const float* x, float* out, int32_t N, int32_t H, int32_t W, int32_t C, void* stream) {
  if (!x || !out || N <= 0) return fail(LDP_EINVAL, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  LDP_TRY(ssm_launch(x, out, N, H, W, C, s));
  LDP_HIP(hipStreamSynchronize(s));
  return LDP_OK;
}

}  // extern "C"
