// vae_train.hpp -- StableVAEModel.update's loss and gradients (model/stable_vae_model.py:57-73) on the training machinery of train.hip.
//
// Included by train.hip inside its anonymous namespace: the VAE is module bit 4 of the same Trainer (flat arenas, Adam + EMA in one launch,
// read / write / publish by Flax path) and its tape runs on the same exact-fp32 segmented GEMM (`seg_gemm`, v_mfma_f32_16x16x4_f32), the same
// deferred column sums and the same side-stream split of weight-gradient work.  What is new here is the 2-D view of the convolutions and the
// element-wise pieces of the StableVAE.
//
// Convolutions.  Rows = samples, as for the planner (csrc/train.hip header), with z = PIXEL instead of z = position; activations are NHWC with
// channels zero-padded to multiples of 32 (the image's 3, the latent's LC and 2 LC), so one conv is one seg_gemm launch per direction:
//     forward   z = output pixel,  segments = its live taps                         A = X (lda = H W Cin),  B = W[tap] (the Flax leaf, row-major)
//     dgrad     z = input pixel,   segments = the (output pixel, tap) pairs that read it
//     wgrad     z = tap,           segments = the output pixels where it is live,    K = the batch
// Taps that fall on padding are not in any list.  Stride 2 reads input (2y + dy, 2x + dx) (XLA SAME on an even side pads (0, 1)); the decoder's
// nearest x2 upsample is folded into its 3x3: tap (dy, dx) of output (y, x) reads input ((y + dy - 1) >> 1, (x + dx - 1) >> 1), so neither the
// upsampled tensor nor its gradient exists.  The tap sets and the table builder are train_tables.hpp's (VC_*, tap_2d, plan_2d); the tables are
// built on the first call for a frame size and appended to the Trainer's.
//
// GroupNorm(32) (+ SiLU) runs on (sample, group) work-groups: at 64 px a block holds 16 384 values, so the statistics take two passes (mean, then
// the centred sum of squares).  The mid-block attention's Dense layers are plain GEMMs over rows = N * tokens, its softmax one work-group per
// sample.  The posterior, the KL term and the loss statistics reuse ldp_vae_metrics's kernels (vae_posterior_kernel, vae_loss_stats_kernel,
// vae_metrics_final_kernel): the eleven metrics come out of the forward pass that the gradients belong to.  No atomics: two calls on the same
// state and batch give the same gradient arena bit for bit.

constexpr int VAE_NG = 32;                  // norm_num_groups
constexpr int VAE_ATT_T = 16;               // most mid-block attention tokens a work-group holds (4 / 9 / 16 at 64 / 96 / 128 px)
constexpr int VAE_TRAIN_MAX_FRAMES = 256;   // frames per ldp_train_vae_grad call (the tape keeps every activation: ~175 MB per 64-px frame)

__device__ __forceinline__ float vae_silu(float x) { return x / (1.0f + expf(-x)); }
__device__ __forceinline__ float vae_silu_dx(float x) {
  const float s = 1.0f / (1.0f + expf(-x));
  return s * (1.0f + x * (1.0f - s));
}
// sum over the 256 threads of a work-group, fixed order (the thread's value, the wave's DPP chain, the four waves in order); red: 4 floats of LDS
__device__ __forceinline__ float vae_block_sum(float v, float* red) {
  v = wsum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// x (Bp, HW, CP) <- img (B, HW, 3) NHWC as the caller holds the frames; padding channels and frames are zero
__global__ void vae_pad_img_kernel(const float* __restrict__ img, float* __restrict__ x, int B, int Bp, int HW, int CP) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)Bp * HW * CP) return;
  const int c = (int)(i % CP);
  const long long np = i / CP;
  const int n = (int)(np / HW);
  x[i] = (n < B && c < 3) ? img[np * 3 + c] : 0.0f;
}

// GroupNorm(32) (+ SiLU) over (Bp, T, C) channels-last: one work-group per (sample, group); thread tid owns elements e = tid + 256 i of the
// block (pixel e / cg, channel e % cg; cg = C / 32 divides 256, so a thread always sees the same channel).  stats[wg * 2] = {mean, rstd}.
__global__ __launch_bounds__(256) void vae_gn_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         float* __restrict__ y, float* __restrict__ stats, int T, int C, int silu) {
  __shared__ float red[4];
  const int n = blockIdx.x / VAE_NG, g = blockIdx.x % VAE_NG, cg = C / VAE_NG, cnt = T * cg, tid = threadIdx.x;
  const size_t base = (size_t)n * T * C + (size_t)g * cg;
  float s = 0.0f;
  for (int e = tid; e < cnt; e += 256) s += x[base + (size_t)(e / cg) * C + e % cg];
  const float mean = vae_block_sum(s, red) / (float)cnt;
  float q = 0.0f;
  for (int e = tid; e < cnt; e += 256) {
    const float d = x[base + (size_t)(e / cg) * C + e % cg] - mean;
    q += d * d;
  }
  const float var = vae_block_sum(q, red) / (float)cnt;
  const float rstd = 1.0f / sqrtf(var + 1e-6f);
  if (tid == 0) {
    stats[(size_t)blockIdx.x * 2] = mean;
    stats[(size_t)blockIdx.x * 2 + 1] = rstd;
  }
  const int ch = g * cg + tid % cg;
  const float ga = gamma[ch], be = beta[ch];
  for (int e = tid; e < cnt; e += 256) {
    const size_t o = base + (size_t)(e / cg) * C + e % cg;
    const float v = (x[o] - mean) * rstd * ga + be;
    y[o] = silu ? vae_silu(v) : v;
  }
}
// backward: u = xh gamma + beta, y = silu(u) (or u);  du = dy y'(u);  dxh = du gamma;  dx = rstd (dxh - mean(dxh) - xh mean(dxh xh)) (+ dres)
// part (Bp, 3C): per sample and channel  sum_t du xh | sum_t du | sum_t dx without dres (the bias gradient of the conv that feeds the norm)
__global__ __launch_bounds__(256) void vae_gn_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ stats,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta, const float* dres,
                                                         float* dx, float* __restrict__ part, int T, int C, int silu) {
  __shared__ float red[4];
  __shared__ float ps[3][256];
  const int n = blockIdx.x / VAE_NG, g = blockIdx.x % VAE_NG, cg = C / VAE_NG, cnt = T * cg, tid = threadIdx.x;
  const size_t base = (size_t)n * T * C + (size_t)g * cg;
  const float mean = stats[(size_t)blockIdx.x * 2], rstd = stats[(size_t)blockIdx.x * 2 + 1];
  const int ch = g * cg + tid % cg;
  const float ga = gamma[ch], be = beta[ch];
  float a1 = 0.0f, a2 = 0.0f, sg = 0.0f, sb = 0.0f;
  for (int e = tid; e < cnt; e += 256) {
    const size_t o = base + (size_t)(e / cg) * C + e % cg;
    const float xh = (x[o] - mean) * rstd;
    const float u = xh * ga + be;
    const float du = silu ? dy[o] * vae_silu_dx(u) : dy[o];
    const float dxh = du * ga;
    a1 += dxh;
    a2 += dxh * xh;
    sg += du * xh;
    sb += du;
  }
  const float m1 = vae_block_sum(a1, red) / (float)cnt;
  const float m2 = vae_block_sum(a2, red) / (float)cnt;
  float sc = 0.0f;
  for (int e = tid; e < cnt; e += 256) {
    const size_t o = base + (size_t)(e / cg) * C + e % cg;
    const float xh = (x[o] - mean) * rstd;
    const float u = xh * ga + be;
    const float du = silu ? dy[o] * vae_silu_dx(u) : dy[o];
    const float v = rstd * ((du * ga - m1) - xh * m2);
    sc += v;
    dx[o] = dres ? v + dres[o] : v;
  }
  ps[0][tid] = sg;
  ps[1][tid] = sb;
  ps[2][tid] = sc;
  __syncthreads();
  if (tid < cg) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float s = 0.0f;
      for (int t2 = tid; t2 < 256; t2 += cg) s += ps[k][t2];
      part[(size_t)n * 3 * C + (size_t)k * C + g * cg + tid] = s;
    }
  }
}

// mid-block attention core, one work-group per sample: s = scale q k^T (scale = (C^-1/4)^2), w = softmax over keys, o = w v.
// q / k / v / o (Bp, T, C) rows, w (Bp, T, T).  Scores: one wave per (query, key) pair, fixed-order sums.
__global__ __launch_bounds__(256) void vae_attn_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                           float* __restrict__ o, float* __restrict__ w, int T, int C, float scale) {
  __shared__ float sw[VAE_ATT_T * VAE_ATT_T];
  const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t base = (size_t)n * T * C;
  for (int p = wave; p < T * T; p += 4) {
    const int i = p / T, j = p % T;
    float s = 0.0f;
    for (int c = lane; c < C; c += 64) s += q[base + (size_t)i * C + c] * k[base + (size_t)j * C + c];
    s = wsum(s);
    if (lane == 0) sw[p] = s * scale;
  }
  __syncthreads();
  if ((int)threadIdx.x < T) {
    const int i = threadIdx.x;
    float mx = -INFINITY;
    for (int j = 0; j < T; ++j) mx = fmaxf(mx, sw[i * T + j]);
    float sum = 0.0f;
    for (int j = 0; j < T; ++j) {
      const float e = expf(sw[i * T + j] - mx);
      sw[i * T + j] = e;
      sum += e;
    }
    for (int j = 0; j < T; ++j) {
      const float wv = sw[i * T + j] / sum;
      sw[i * T + j] = wv;
      w[(size_t)n * T * T + i * T + j] = wv;
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256)
    for (int i = 0; i < T; ++i) {
      float acc = 0.0f;
      for (int j = 0; j < T; ++j) acc += sw[i * T + j] * v[base + (size_t)j * C + c];
      o[base + (size_t)i * C + c] = acc;
    }
}
// backward: dv_j = sum_i w_ij do_i;  dw_ij = do_i . v_j;  ds_ij = w_ij (dw_ij - sum_j' w_ij' dw_ij');  dq_i = scale sum_j ds_ij k_j;
// dk_j = scale sum_i ds_ij q_i.  (sum_j ds_ij = 0 for every query: the column sums of dk -- key/bias's gradient -- vanish; the tape writes 0.)
__global__ __launch_bounds__(256) void vae_attn_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ q, const float* __restrict__ k,
                                                           const float* __restrict__ v, const float* __restrict__ w, float* __restrict__ dq,
                                                           float* __restrict__ dk, float* __restrict__ dv, int T, int C, float scale) {
  __shared__ float sw[VAE_ATT_T * VAE_ATT_T], sd[VAE_ATT_T * VAE_ATT_T];
  const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t base = (size_t)n * T * C;
  for (int p = threadIdx.x; p < T * T; p += 256) sw[p] = w[(size_t)n * T * T + p];
  for (int p = wave; p < T * T; p += 4) {
    const int i = p / T, j = p % T;
    float s = 0.0f;
    for (int c = lane; c < C; c += 64) s += dout[base + (size_t)i * C + c] * v[base + (size_t)j * C + c];
    s = wsum(s);
    if (lane == 0) sd[p] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < T) {
    const int i = threadIdx.x;
    float dot = 0.0f;
    for (int j = 0; j < T; ++j) dot += sw[i * T + j] * sd[i * T + j];
    for (int j = 0; j < T; ++j) sd[i * T + j] = sw[i * T + j] * (sd[i * T + j] - dot) * scale;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    for (int j = 0; j < T; ++j) {
      float av = 0.0f, ak = 0.0f;
      for (int i = 0; i < T; ++i) {
        av += sw[i * T + j] * dout[base + (size_t)i * C + c];
        ak += sd[i * T + j] * q[base + (size_t)i * C + c];
      }
      dv[base + (size_t)j * C + c] = av;
      dk[base + (size_t)j * C + c] = ak;
    }
    for (int i = 0; i < T; ++i) {
      float aq = 0.0f;
      for (int j = 0; j < T; ++j) aq += sd[i * T + j] * k[base + (size_t)j * C + c];
      dq[base + (size_t)i * C + c] = aq;
    }
  }
}

// rec (Bp, HW, CP) channels-last -> (B, 3, HW) NCHW, the layout vae_loss_stats_kernel reads
__global__ void vae_rec_nchw_kernel(const float* __restrict__ rec, float* __restrict__ out, int B, int HW, int CP) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)B * 3 * HW) return;
  const int p = (int)(i % HW), c = (int)((i / HW) % 3);
  const long long n = i / (3LL * HW);
  out[i] = rec[((size_t)n * HW + p) * CP + c];
}
// d rec = 2 (rec - img) / (N 3 S^2) (jnp.mean((img - pred_img) ** 2)) on the real channels of the real frames, 0 elsewhere
__global__ void vae_rec_grad_kernel(const float* __restrict__ rec, const float* __restrict__ img, float* __restrict__ drec, int B, int Bp, int HW, int CP,
                                    float scale) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)Bp * HW * CP) return;
  const int c = (int)(i % CP);
  const long long np = i / CP;
  const int n = (int)(np / HW);
  drec[i] = (n < B && c < 3) ? scale * (rec[i] - img[np * 3 + c]) : 0.0f;
}
// backward of the posterior draw and the KL term: z = mean + exp(lv_c / 2) eps, lv_c = clip(lv, -30, 20), loss += beta mean_n KL_n with
// KL_n = 0.5 sum (mean^2 + exp(lv_c) - 1 - lv_c):   d mean = dz + beta mean / N;   d lv = dz eps std / 2 + beta (exp(lv) - 1) / (2 N) inside the
// clip, 0 outside.  mom / dz / dmom (Bp, E, CP) with channels [0, LC) mean and [LC, 2 LC) log-variance; eps as vae_posterior_kernel draws it.
// NT: the frames the loss is the mean over (B, or the whole batch that these B frames are a part of: ldp_train_vae_grad_part).
__global__ void vae_post_bwd_kernel(const float* __restrict__ mom, const float* __restrict__ dz, const float* __restrict__ eps, uint64_t seed,
                                    uint64_t row0, float* __restrict__ dmom, int B, int NT, int Bp, int E, int LC, int CP, int use_kl, float beta) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)Bp * E * CP) return;
  const int c = (int)(i % CP);
  const long long np = i / CP;
  const int n = (int)(np / E), pix = (int)(np % E);
  float out = 0.0f;
  if (n < B && c < 2 * LC) {
    const int cc = c < LC ? c : c - LC;
    const float g = dz[np * CP + cc];
    if (c < LC) {
      out = use_kl ? g + beta * mom[np * CP + cc] / (float)NT : g;
    } else {
      const float lv = mom[np * CP + c];
      if (lv > -30.0f && lv < 20.0f) {
        const uint64_t per = (uint64_t)E * (uint64_t)LC, e = (uint64_t)pix * LC + cc;
        const float ep = eps ? eps[(size_t)n * per + e] : philox_normal(seed, (row0 + (uint64_t)n) * per + e, 0u, LDP_PHILOX_STREAM_VAE_EPS);
        out = g * ep * expf(0.5f * lv) * 0.5f;
        if (use_kl) out += beta * (expf(lv) - 1.0f) / (2.0f * (float)NT);
      }
    }
  }
  dmom[i] = out;
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------
const int VAE_CH[6] = {128, 256, 256, 256, 256, 256};      // model/stable_vae_model.yaml:6 (vae.hip builds the same)
constexpr int VAE_NB = 6, VAE_LAYERS = 2;

// the Flax tree of weights.py vae_shapes, in its order; conv kernels (kh, kw, Cin, Cout) are [kh kw][Cin_p][Cout_p] with Cin / Cout padded to 32
void describe_vae(Module& m, int LC) {
  auto conv = [&](const std::string& p, int k, int cin, int cout) {
    m.add(p + "/kernel", {k, k, cin, cout}, rup(cin, RP), rup(cout, RP));
    m.add(p + "/bias", {cout}, 1, rup(cout, RP));
  };
  auto norm = [&](const std::string& p, int c) {
    m.add(p + "/scale", {c});
    m.add(p + "/bias", {c});
  };
  auto resnet = [&](const std::string& p, int cin, int cout) {
    norm(p + "/norm1", cin);
    conv(p + "/conv1", 3, cin, cout);
    norm(p + "/norm2", cout);
    conv(p + "/conv2", 3, cout, cout);
    if (cin != cout) conv(p + "/conv_shortcut", 1, cin, cout);
  };
  auto mid = [&](const std::string& p, int c) {
    resnet(p + "/resnets_0", c, c);
    const std::string a = p + "/attentions_0";
    norm(a + "/group_norm", c);
    for (const char* nm : {"query", "key", "value", "proj_attn"}) {
      m.add(a + "/" + nm + "/kernel", {c, c});
      m.add(a + "/" + nm + "/bias", {c});
    }
    resnet(p + "/resnets_1", c, c);
  };
  conv("encoder/conv_in", 3, 3, VAE_CH[0]);
  int cin = VAE_CH[0];
  for (int i = 0; i < VAE_NB; ++i) {
    for (int j = 0; j < VAE_LAYERS; ++j) {
      resnet("encoder/down_blocks_" + std::to_string(i) + "/resnets_" + std::to_string(j), cin, VAE_CH[i]);
      cin = VAE_CH[i];
    }
    if (i != VAE_NB - 1) conv("encoder/down_blocks_" + std::to_string(i) + "/downsamplers_0/conv", 3, VAE_CH[i], VAE_CH[i]);
  }
  mid("encoder/mid_block", VAE_CH[VAE_NB - 1]);
  norm("encoder/conv_norm_out", VAE_CH[VAE_NB - 1]);
  conv("encoder/conv_out", 3, VAE_CH[VAE_NB - 1], 2 * LC);
  conv("quant_conv", 1, 2 * LC, 2 * LC);
  conv("post_quant_conv", 1, LC, LC);
  conv("decoder/conv_in", 3, LC, VAE_CH[VAE_NB - 1]);
  mid("decoder/mid_block", VAE_CH[VAE_NB - 1]);
  cin = VAE_CH[VAE_NB - 1];
  for (int i = 0; i < VAE_NB; ++i) {
    const int c = VAE_CH[VAE_NB - 1 - i];
    for (int j = 0; j < VAE_LAYERS + 1; ++j) {
      resnet("decoder/up_blocks_" + std::to_string(i) + "/resnets_" + std::to_string(j), cin, c);
      cin = c;
    }
    if (i != VAE_NB - 1) conv("decoder/up_blocks_" + std::to_string(i) + "/upsamplers_0/conv", 3, c, c);
  }
  norm("decoder/conv_norm_out", VAE_CH[0]);
  conv("decoder/conv_out", 3, VAE_CH[0], 3);
}

// the plan of a convolution: built (and the tables marked for upload) the first time the dry walk of a tape asks for it
const ConvPlan& vae_plan(Trainer& t, int mode, int Sin, int Sout, int cin, int cout) {
  const std::string key = std::to_string(mode) + ":" + std::to_string(Sin) + ":" + std::to_string(Sout) + ":" + std::to_string(cin) + ":" + std::to_string(cout);
  auto it = t.vconvs.find(key);
  if (it != t.vconvs.end()) return it->second;
  t.tables_dirty = true;
  return t.vconvs.emplace(key, plan_2d(t.tab, mode, Sin, Sout, cin, cout)).first->second;
}

int vae_gn_fwd(const Ctx& c, const float* x, const float* gamma, const float* beta, float* y, float* stats, int Bp, int T, int C, int silu) {
  TK(vae_gn_fwd_kernel, dim3(Bp * VAE_NG), dim3(256), x, gamma, beta, y, stats, T, C, silu);
  return LDP_OK;
}
int vae_gn_bwd(const Ctx& c, const float* dy, const float* x, const float* stats, const float* gamma, const float* beta, const float* dres, float* dx,
               float* part, int Bp, int T, int C, int silu) {
  TK(vae_gn_bwd_kernel, dim3(Bp * VAE_NG), dim3(256), dy, x, stats, gamma, beta, dres, dx, part, T, C, silu);
  return LDP_OK;
}

// one step of the tape: what its backward needs
struct VaeOp {
  int kind = 0;                    // 0 conv, 1 ResnetBlock2D, 2 AttentionBlock, 3 GroupNorm + SiLU
  std::string p;
  const ConvPlan* cv[3] = {nullptr, nullptr, nullptr};      // conv: [0];  resnet: conv1, conv2, conv_shortcut
  int S = 0, cin = 0, cout = 0;    // resnet / norm / attention: side and (padded) widths
  const float* x = nullptr;
  float *y = nullptr, *a1 = nullptr, *h1 = nullptr, *a2 = nullptr, *r = nullptr, *st1 = nullptr, *st2 = nullptr;
  float *q = nullptr, *k = nullptr, *v = nullptr, *o = nullptr, *w = nullptr;
};

// ---- the StableVAE: loss + gradients (model/stable_vae_model.py:25-73; diffusers FlaxAutoencoderKL) -------------------------------------
// n_total >= B: the frames of the batch whose mean loss is differentiated (these B are a part of it; the metrics are these B frames' alone);
// gdst: the arena the gradients are written to (the module's own, or the part buffer that ldp_train_vae_grad_part adds to it afterwards)
int vae_tape(Ctx& c, const float* img, int B, int n_total, float* gdst, int use_kl, float beta, const float* eps, uint64_t seed, uint64_t row0, float* metrics) {
  Trainer& t = *c.t;
  Module& m = *c.M;
  const int S = c.h->cfg.image_size, LC = c.h->cfg.vae_latent_channels, Bp = rup(B, RP), HW = S * S;
  const int hl = S >> (VAE_NB - 1), E = hl * hl, CL = RP;      // CL: padded width of the image / latent-side tensors
  c.L->ws_used = 0;
  auto P = [&](const std::string& path) { return m.P.f() + m.leaf(path).off; };
  auto Gd = [&](const std::string& path) { return gdst + m.leaf(path).off; };
  auto take = [&](size_t n) { return ws_take(*c.L, n); };
  std::vector<VaeOp> ops;
  int err = LDP_OK;                                           // the first failed launch of the forward lambdas below
#define VAE_TRY(expr) do { if ((err = (expr)) != LDP_OK) return (float*)nullptr; } while (0)

  auto conv = [&](const std::string& p, int mode, int Sin, int Sout, int cin, int cout, const float* x, const float* add = nullptr) -> float* {
    VaeOp op;
    op.kind = 0; op.p = p; op.x = x;
    op.cv[0] = &vae_plan(t, mode, Sin, Sout, rup(cin, RP), rup(cout, RP));
    op.y = take((size_t)Bp * Sout * Sout * rup(cout, RP));
    VAE_TRY(conv_fwd(c, *op.cv[0], x, P(p + "/kernel"), P(p + "/bias"), add, op.y, Bp));
    ops.push_back(op);
    return op.y;
  };
  auto norm = [&](const std::string& p, int Sd, int C, const float* x) -> float* {
    VaeOp op;
    op.kind = 3; op.p = p; op.S = Sd; op.cout = C; op.x = x;
    op.y = take((size_t)Bp * Sd * Sd * C);
    op.st1 = take((size_t)Bp * VAE_NG * 2);
    VAE_TRY(vae_gn_fwd(c, x, P(p + "/scale"), P(p + "/bias"), op.y, op.st1, Bp, Sd * Sd, C, 1));
    ops.push_back(op);
    return op.y;
  };
  auto resnet = [&](const std::string& p, int Sd, int cin, int cout, const float* x) -> float* {
    VaeOp op;
    op.kind = 1; op.p = p; op.S = Sd; op.cin = cin; op.cout = cout; op.x = x;
    const size_t ni = (size_t)Bp * Sd * Sd * cin, no = (size_t)Bp * Sd * Sd * cout;
    op.a1 = take(ni); op.h1 = take(no); op.a2 = take(no); op.y = take(no);
    op.st1 = take((size_t)Bp * VAE_NG * 2); op.st2 = take((size_t)Bp * VAE_NG * 2);
    op.cv[0] = &vae_plan(t, VC_S1, Sd, Sd, cin, cout);
    op.cv[1] = &vae_plan(t, VC_S1, Sd, Sd, cout, cout);
    const float* res = x;
    if (cin != cout) {
      op.cv[2] = &vae_plan(t, VC_P1, Sd, Sd, cin, cout);
      op.r = take(no);
      VAE_TRY(conv_fwd(c, *op.cv[2], x, P(p + "/conv_shortcut/kernel"), P(p + "/conv_shortcut/bias"), nullptr, op.r, Bp));
      res = op.r;
    }
    VAE_TRY(vae_gn_fwd(c, x, P(p + "/norm1/scale"), P(p + "/norm1/bias"), op.a1, op.st1, Bp, Sd * Sd, cin, 1));
    VAE_TRY(conv_fwd(c, *op.cv[0], op.a1, P(p + "/conv1/kernel"), P(p + "/conv1/bias"), nullptr, op.h1, Bp));
    VAE_TRY(vae_gn_fwd(c, op.h1, P(p + "/norm2/scale"), P(p + "/norm2/bias"), op.a2, op.st2, Bp, Sd * Sd, cout, 1));
    VAE_TRY(conv_fwd(c, *op.cv[1], op.a2, P(p + "/conv2/kernel"), P(p + "/conv2/bias"), res, op.y, Bp));
    ops.push_back(op);
    return op.y;
  };
  const float scale = (float)(1.0 / std::sqrt((double)VAE_CH[VAE_NB - 1]));    // (C^-1/4)^2, applied once to q . k
  auto attn = [&](const std::string& p, int Sd, int C, const float* x) -> float* {
    VaeOp op;
    op.kind = 2; op.p = p; op.S = Sd; op.cout = C; op.x = x;
    const int T = Sd * Sd, R = Bp * T;
    op.a1 = take((size_t)R * C); op.st1 = take((size_t)Bp * VAE_NG * 2);
    op.q = take((size_t)R * C); op.k = take((size_t)R * C); op.v = take((size_t)R * C); op.o = take((size_t)R * C);
    op.w = take((size_t)Bp * T * T); op.y = take((size_t)R * C);
    VAE_TRY(vae_gn_fwd(c, x, P(p + "/group_norm/scale"), P(p + "/group_norm/bias"), op.a1, op.st1, Bp, T, C, 0));
    VAE_TRY(dense_fwd(c, op.a1, C, P(p + "/query/kernel"), C, P(p + "/query/bias"), nullptr, op.q, C, R, C, C));
    VAE_TRY(dense_fwd(c, op.a1, C, P(p + "/key/kernel"), C, P(p + "/key/bias"), nullptr, op.k, C, R, C, C));
    VAE_TRY(dense_fwd(c, op.a1, C, P(p + "/value/kernel"), C, P(p + "/value/bias"), nullptr, op.v, C, R, C, C));
    TK(vae_attn_fwd_kernel, dim3(Bp), dim3(256), op.q, op.k, op.v, op.o, op.w, T, C, scale);
    VAE_TRY(dense_fwd(c, op.o, C, P(p + "/proj_attn/kernel"), C, P(p + "/proj_attn/bias"), x, op.y, C, R, C, C));
    ops.push_back(op);
    return op.y;
  };
  auto mid = [&](const std::string& p, const float* x) -> float* {
    const int C = VAE_CH[VAE_NB - 1];
    float* y = resnet(p + "/resnets_0", hl, C, C, x);
    if (y) y = attn(p + "/attentions_0", hl, C, y);
    if (y) y = resnet(p + "/resnets_1", hl, C, C, y);
    return y;
  };
#define VAE_STEP(expr) do { if (!(x = (expr))) return err; } while (0)

  // ---- encoder ----------------------------------------------------------------------------------------------------------------------
  float* x0 = take((size_t)Bp * HW * CL);
  TK(vae_pad_img_kernel, g1((long long)Bp * HW * CL), dim3(256), img, x0, B, Bp, HW, CL);
  float* x = nullptr;
  VAE_STEP(conv("encoder/conv_in", VC_S1, S, S, 3, VAE_CH[0], x0));
  int Sd = S, cin = VAE_CH[0];
  for (int i = 0; i < VAE_NB; ++i) {
    for (int j = 0; j < VAE_LAYERS; ++j) {
      VAE_STEP(resnet("encoder/down_blocks_" + std::to_string(i) + "/resnets_" + std::to_string(j), Sd, cin, VAE_CH[i], x));
      cin = VAE_CH[i];
    }
    if (i != VAE_NB - 1) {
      VAE_STEP(conv("encoder/down_blocks_" + std::to_string(i) + "/downsamplers_0/conv", VC_S2, Sd, Sd / 2, cin, cin, x));
      Sd /= 2;
    }
  }
  VAE_STEP(mid("encoder/mid_block", x));
  VAE_STEP(norm("encoder/conv_norm_out", hl, cin, x));
  VAE_STEP(conv("encoder/conv_out", VC_S1, hl, hl, cin, 2 * LC, x));
  VAE_STEP(conv("quant_conv", VC_P1, hl, hl, 2 * LC, 2 * LC, x));
  float* mom = x;                                             // (Bp, E, CL): [0, LC) mean, [LC, 2 LC) log-variance
  const size_t n_enc = ops.size();

  // ---- posterior (FlaxDiagonalGaussianDistribution.sample / .kl) -------------------------------------------------------------------------
  float* momc = take((size_t)B * E * 2 * LC);
  float* zc = take((size_t)B * E * LC);
  float* kl = take((size_t)B);
  const int nzb = vae_posterior_blocks(B, E, LC), nib = vae_loss_blocks((long long)B * HW);
  double* zpart = reinterpret_cast<double*>(take((size_t)nzb * 12));
  double* ipart = reinterpret_cast<double*>(take((size_t)nib * 12));
  LDP_TRY(copy_cols(c, mom, CL, momc, 2 * LC, B * E, 2 * LC));
  if (!c.dry) LDP_TRY(vae_posterior_launch(momc, eps, seed, row0, zc, nullptr, kl, zpart, B, E, LC, c.s));
  float* zp = take((size_t)Bp * E * CL);
  LDP_TRY(copy_cols(c, nullptr, 0, zp, CL, Bp * E, CL));
  LDP_TRY(copy_cols(c, zc, LC, zp, CL, B * E, LC));

  // ---- decoder ----------------------------------------------------------------------------------------------------------------------
  VAE_STEP(conv("post_quant_conv", VC_P1, hl, hl, LC, LC, zp));
  VAE_STEP(conv("decoder/conv_in", VC_S1, hl, hl, LC, VAE_CH[VAE_NB - 1], x));
  VAE_STEP(mid("decoder/mid_block", x));
  cin = VAE_CH[VAE_NB - 1];
  for (int i = 0; i < VAE_NB; ++i) {
    const int co = VAE_CH[VAE_NB - 1 - i];
    for (int j = 0; j < VAE_LAYERS + 1; ++j) {
      VAE_STEP(resnet("decoder/up_blocks_" + std::to_string(i) + "/resnets_" + std::to_string(j), Sd, cin, co, x));
      cin = co;
    }
    if (i != VAE_NB - 1) {
      VAE_STEP(conv("decoder/up_blocks_" + std::to_string(i) + "/upsamplers_0/conv", VC_UP, Sd, 2 * Sd, co, co, x));
      Sd *= 2;
    }
  }
  VAE_STEP(norm("decoder/conv_norm_out", S, cin, x));
  VAE_STEP(conv("decoder/conv_out", VC_S1, S, S, cin, 3, x));
#undef VAE_STEP
#undef VAE_TRY
  const float* rec = x;                                       // (Bp, HW, CL), channels [0, 3) real

  // ---- loss and metrics (model/stable_vae_model.py:34-53), then d rec ---------------------------------------------------------------------
  float* recn = take((size_t)B * 3 * HW);
  TK(vae_rec_nchw_kernel, g1((long long)B * 3 * HW), dim3(256), rec, recn, B, HW, CL);
  if (!c.dry) {
    LDP_TRY(vae_loss_stats_launch(img, recn, (long long)B * HW, HW, ipart, c.s));
    LDP_TRY(vae_metrics_final_launch(ipart, nib, zpart, nzb, kl, B, use_kl, beta, metrics, c.s));
  }
  float* d = take((size_t)Bp * HW * CL);
  TK(vae_rec_grad_kernel, g1((long long)Bp * HW * CL), dim3(256), rec, img, d, B, Bp, HW, CL, (float)(2.0 / (3.0 * (double)n_total * HW)));

  // ---- backward: one op at a time, last first; weight-gradient work on the side streams -------------------------------------------------
  auto bwd = [&](const VaeOp& op, const float* dy, bool need_dx, float** dx_out) -> int {
    Ctx w;
    *dx_out = nullptr;
    if (op.kind == 0) {
      const ConvPlan& pl = *op.cv[0];
      LDP_TRY(fork(c, &w));
      LDP_TRY(conv_wgrad(w, pl, op.x, dy, Gd(op.p + "/kernel"), Bp));
      LDP_TRY(colsum(w, dy, pl.cout, Bp * pl.Tout, pl.cout, Gd(op.p + "/bias")));
      if (need_dx) {
        float* dx = take((size_t)Bp * pl.Tin * pl.cin);
        LDP_TRY(conv_dgrad(c, pl, dy, P(op.p + "/kernel"), nullptr, dx, Bp));
        *dx_out = dx;
      }
    } else if (op.kind == 3) {
      const int T = op.S * op.S, C = op.cout;
      float* dx = take((size_t)Bp * T * C);
      float* part = take((size_t)Bp * 3 * C);
      LDP_TRY(vae_gn_bwd(c, dy, op.x, op.st1, P(op.p + "/scale"), P(op.p + "/bias"), nullptr, dx, part, Bp, T, C, 1));
      LDP_TRY(fork(c, &w));
      LDP_TRY(colsum_to(w, part, 3 * C, Bp, 2 * C, ColOut{{Gd(op.p + "/scale"), Gd(op.p + "/bias"), nullptr}, C}));
      *dx_out = dx;
    } else if (op.kind == 1) {
      const int T = op.S * op.S;
      const std::string& p = op.p;
      const size_t ni = (size_t)Bp * T * op.cin, no = (size_t)Bp * T * op.cout;
      LDP_TRY(fork(c, &w));                                   // dy exists
      LDP_TRY(conv_wgrad(w, *op.cv[1], op.a2, dy, Gd(p + "/conv2/kernel"), Bp));
      LDP_TRY(colsum(w, dy, op.cout, Bp * T, op.cout, Gd(p + "/conv2/bias")));
      if (op.cv[2]) {
        LDP_TRY(conv_wgrad(w, *op.cv[2], op.x, dy, Gd(p + "/conv_shortcut/kernel"), Bp));
        LDP_TRY(colsum(w, dy, op.cout, Bp * T, op.cout, Gd(p + "/conv_shortcut/bias")));
      }
      float* da2 = take(no);
      LDP_TRY(conv_dgrad(c, *op.cv[1], dy, P(p + "/conv2/kernel"), nullptr, da2, Bp));
      float* dh1 = take(no);
      float* part2 = take((size_t)Bp * 3 * op.cout);
      LDP_TRY(vae_gn_bwd(c, da2, op.h1, op.st2, P(p + "/norm2/scale"), P(p + "/norm2/bias"), nullptr, dh1, part2, Bp, T, op.cout, 1));
      LDP_TRY(fork(c, &w));                                   // dh1, part2 exist
      LDP_TRY(colsum_to(w, part2, 3 * op.cout, Bp, 3 * op.cout, ColOut{{Gd(p + "/norm2/scale"), Gd(p + "/norm2/bias"), Gd(p + "/conv1/bias")}, op.cout}));
      LDP_TRY(conv_wgrad(w, *op.cv[0], op.a1, dh1, Gd(p + "/conv1/kernel"), Bp));
      float* da1 = take(ni);
      LDP_TRY(conv_dgrad(c, *op.cv[0], dh1, P(p + "/conv1/kernel"), nullptr, da1, Bp));
      float* dx = take(ni);
      float* part1 = take((size_t)Bp * 3 * op.cin);
      LDP_TRY(vae_gn_bwd(c, da1, op.x, op.st1, P(p + "/norm1/scale"), P(p + "/norm1/bias"), op.cv[2] ? nullptr : dy, dx, part1, Bp, T, op.cin, 1));
      LDP_TRY(fork(c, &w));
      LDP_TRY(colsum_to(w, part1, 3 * op.cin, Bp, 2 * op.cin, ColOut{{Gd(p + "/norm1/scale"), Gd(p + "/norm1/bias"), nullptr}, op.cin}));
      if (op.cv[2]) LDP_TRY(conv_dgrad(c, *op.cv[2], dy, P(p + "/conv_shortcut/kernel"), dx, dx, Bp));
      *dx_out = dx;
    } else {
      const int T = op.S * op.S, C = op.cout, R = Bp * T;
      const std::string& p = op.p;
      LDP_TRY(fork(c, &w));
      LDP_TRY(dense_wgrad(w, op.o, C, dy, C, Gd(p + "/proj_attn/kernel"), C, R, C, C));
      LDP_TRY(colsum(w, dy, C, R, C, Gd(p + "/proj_attn/bias")));
      float* dO = take((size_t)R * C);
      LDP_TRY(dense_dgrad(c, dy, C, P(p + "/proj_attn/kernel"), C, nullptr, dO, C, R, C, C));
      float* dq = take((size_t)R * C);
      float* dk = take((size_t)R * C);
      float* dv = take((size_t)R * C);
      TK(vae_attn_bwd_kernel, dim3(Bp), dim3(256), dO, op.q, op.k, op.v, op.w, dq, dk, dv, T, C, scale);
      LDP_TRY(fork(c, &w));
      const char* names[3] = {"query", "key", "value"};
      const float* grads[3] = {dq, dk, dv};
      for (int i = 0; i < 3; ++i) {
        LDP_TRY(dense_wgrad(w, op.a1, C, grads[i], C, Gd(p + "/" + names[i] + "/kernel"), C, R, C, C));
        // key/bias shifts every score of query i by the same q_i . b, which the softmax ignores: its gradient sum_j ds_ij q_i is zero for every
        // input.  It is written as the exact zero, not as the column sum of dk (round-off of sum_j ds_ij, which Adam's first steps would
        // blow up to a full +-lr step on a parameter that the loss does not depend on).
        if (i == 1) LDP_TRY(copy_cols(w, nullptr, 0, Gd(p + "/key/bias"), C, 1, C));
        else LDP_TRY(colsum(w, grads[i], C, R, C, Gd(p + "/" + names[i] + "/bias")));
      }
      float* dr = take((size_t)R * C);
      for (int i = 0; i < 3; ++i)
        LDP_TRY(dense_dgrad(c, grads[i], C, P(p + "/" + names[i] + "/kernel"), C, i ? dr : nullptr, dr, C, R, C, C));
      float* dx = take((size_t)R * C);
      float* part = take((size_t)Bp * 3 * C);
      LDP_TRY(vae_gn_bwd(c, dr, op.x, op.st1, P(p + "/group_norm/scale"), P(p + "/group_norm/bias"), dy, dx, part, Bp, T, C, 0));
      LDP_TRY(fork(c, &w));
      LDP_TRY(colsum_to(w, part, 3 * C, Bp, 2 * C, ColOut{{Gd(p + "/group_norm/scale"), Gd(p + "/group_norm/bias"), nullptr}, C}));
      *dx_out = dx;
    }
    return LDP_OK;
  };
  for (size_t i = ops.size(); i-- > n_enc;) {
    float* dx = nullptr;
    LDP_TRY(bwd(ops[i], d, true, &dx));
    d = dx;
  }
  float* dmom = take((size_t)Bp * E * CL);                   // d is now d z (Bp, E, CL)
  TK(vae_post_bwd_kernel, g1((long long)Bp * E * CL), dim3(256), mom, d, eps, seed, row0, dmom, B, n_total, Bp, E, LC, CL, use_kl, beta);
  d = dmom;
  for (size_t i = n_enc; i-- > 0;) {
    float* dx = nullptr;
    LDP_TRY(bwd(ops[i], d, i > 0, &dx));
    d = dx;
  }
  Ctx w;
  LDP_TRY(fork(c, &w, 1, 1));
  LDP_TRY(flush_colsums(w));
  if (!c.dry) LDP_HIP(hipGetLastError());
  return LDP_OK;
}
