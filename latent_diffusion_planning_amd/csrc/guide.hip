// guide.hip -- guided planning (include/ldp_hip.h "guided planning"): one projected gradient step on a trajectory cost
// inside every denoising step.  The cost per sample, on the clipped data prediction y (T, D):
//   J(y) = 1/2 sum_{t,c} wg[t,c] (y[t,c] - target[t,c])^2                                            soft goals / waypoints
//        + 1/2 sum_c lam[c] ( sum_{t < T-1} (y[t+1,c] - y[t,c])^2 + [anchor] (y[0,c] - anchor[c])^2 )   smoothness, continuity
//        + 1/2 sum_{t,c} beta[c] ( max(y - hi[c], 0)^2 + max(lo[c] - y, 0)^2 )                         box bounds
// Here: the guided step (one launch behind every U-Net evaluation of a guided loop), the cost itself (one launch), the staging of a
// call's guide into the handle-owned buffers the captured loop reads, and the two stand-alone entry points.
// Exact fp32 on the VALU; a work-group owns whole samples (the stencil along T goes through LDS); no atomics, vector stores only.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "engine.hpp"
#include "tconv.hpp"      // philox_normal

namespace ldp {
namespace {

constexpr unsigned GUIDE_MAX_BLOCKS = 2048;       // 8 work-groups of 256 threads per CU on 256 CUs: the rest is strided
constexpr int GUIDE_MAX_T = 16, GUIDE_MAX_D = 128;
constexpr int GUIDE_LDS_FLOATS = GUIDE_MAX_T * GUIDE_MAX_D;      // 8 KB: one sample's clipped data prediction
constexpr int GUIDE_MAX_STEPS = 4096;             // (check_sampler: a loop has at most 4094 steps)

// What a guide is made of, as the kernels read it.  target / wg: (B, T, ldg); anchor: (B, ldg) or nullptr (no continuity term); lam, beta,
// lo, hi: (D); rho: the step-size table, entry `step` is read.  All device memory.
struct GuideDev {
  const float* target; const float* wg; const float* anchor;
  const float* lam; const float* beta; const float* lo; const float* hi;
  const float* rho;
  int ldg;
};

__device__ __forceinline__ void load4(const float* p, size_t base, int c0, int D, bool vec, float (&v)[4]) {
  if (vec) {
    const float4 q = *reinterpret_cast<const float4*>(p + base);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = c0 + q < D ? p[base + q] : 0.0f;
  }
}

// The guided step of `B` samples of T rows and D real channels, in place on x when x_out == x.  Per element, every operation rounded to
// fp32 once, in this order (k: the step's coefficient row; r = rho[step]; y_prev / y_next: y at t-1 / t+1 of the same channel):
//   y    = clamp(rn(rn(fma(-k.sqrt_1mab, eps, x)) * k.inv_sqrt_ab), -1, 1)                                  (phase 1, into LDS)
//   g    = rn(wg * rn(y - target))
//   dn   = t < T-1 ? rn(y - y_next) : 0;   dp = t > 0 ? rn(y - y_prev) : anchor ? rn(y - anchor) : 0
//   g    = rn(fma(lam, rn(dn + dp), g))
//   g    = rn(fma(beta, rn(max(rn(y - hi), 0) - max(rn(lo - y), 0)), g))
//   y'   = clamp(rn(fma(-r, g, y)), -1, 1)
//   x'   = rn(fma(k.c_eps, eps, rn(fma(k.c_x, x, rn(k.c_x0 * y')))));   sigma != 0:  x' = rn(fma(k.sigma, z, x'))
// z = noise[r, c] when `noise` is given, else philox_normal(seed, (row0 + r) * DP + c, step, LDP_PHILOX_STREAM_STEP) -- the fused step's
// draw -- with r = b * T + t the local row and (seed, row0) read from `ctl` when there is one (inside a captured loop).
// A work-group owns whole samples: it fills LDS with one sample's y (phase 1), synchronises, and computes the update of that sample from
// LDS (phase 2); x and eps are read again in phase 2 by the thread that read them in phase 1, which is also the only thread that stores
// these elements of x.  No work-group reads what another writes.  A sample with more channel groups than threads is looped over.
// x / x_out have row stride ldx, eps / noise D, target / wg / anchor G.ldg; only the columns c < D are read or written.
// VX / VG / VE: that family's row stride is a multiple of four and its bases are 16-byte aligned, so a thread whose four columns all lie
// below D moves them as one 16-byte access; the group that straddles D and every family that cannot be vectorised go element by element.
template <bool VX, bool VG, bool VE>
__global__ __launch_bounds__(256) void plan_guide_step_kernel(const float* x, const float* __restrict__ eps, const float* __restrict__ noise,
                                                              float* x_out, GuideDev G, int ldx, int B, int T, int D, int DP, StepCoef k,
                                                              int step, const uint64_t* __restrict__ ctl, uint64_t seed, uint64_t row0) {
  __shared__ float y_s[GUIDE_LDS_FLOATS];
  const int gpr = (D + 3) / 4;                               // channel groups per row
  const int ls = gpr * 4;                                    // LDS row stride
  const int n = T * gpr;                                     // channel groups per sample
  if (ctl) { seed = ctl[0]; row0 = ctl[1]; }
  const float r = G.rho[step];
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    // phase 1: the clipped data prediction of this sample
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const int t = i / gpr, c0 = (i - t * gpr) * 4;
      const bool full = c0 + 4 <= D;
      const size_t row = (size_t)b * T + t;
      float xv[4], ev[4];
      load4(x, row * ldx + c0, c0, D, VX && full, xv);
      load4(eps, row * D + c0, c0, D, VE && full, ev);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float y = __fmul_rn(__fmaf_rn(-k.sqrt_1mab, ev[q], xv[q]), k.inv_sqrt_ab);
        y_s[t * ls + c0 + q] = c0 + q < D ? fminf(fmaxf(y, -1.0f), 1.0f) : 0.0f;
      }
    }
    __syncthreads();
    // phase 2: gradient, projected step, scheduler update
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const int t = i / gpr, c0 = (i - t * gpr) * 4;
      const bool full = c0 + 4 <= D;
      const size_t row = (size_t)b * T + t;
      float xv[4], ev[4], tv[4], wv[4], av[4] = {0.f, 0.f, 0.f, 0.f}, zv[4] = {0.f, 0.f, 0.f, 0.f};
      load4(x, row * ldx + c0, c0, D, VX && full, xv);
      load4(eps, row * D + c0, c0, D, VE && full, ev);
      load4(G.target, row * G.ldg + c0, c0, D, VG && full, tv);
      load4(G.wg, row * G.ldg + c0, c0, D, VG && full, wv);
      const bool anchored = t == 0 && G.anchor != nullptr;
      if (anchored) load4(G.anchor, (size_t)b * G.ldg + c0, c0, D, VG && full, av);
      if (k.sigma != 0.f && noise) load4(noise, row * D + c0, c0, D, VE && full, zv);
      float xo[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = c0 + q;
        xo[q] = 0.0f;
        if (c >= D) continue;
        const float y = y_s[t * ls + c];
        float g = __fmul_rn(wv[q], __fsub_rn(y, tv[q]));
        const float dn = t < T - 1 ? __fsub_rn(y, y_s[(t + 1) * ls + c]) : 0.0f;
        const float dp = t > 0 ? __fsub_rn(y, y_s[(t - 1) * ls + c]) : anchored ? __fsub_rn(y, av[q]) : 0.0f;
        g = __fmaf_rn(G.lam[c], __fadd_rn(dn, dp), g);
        const float hu = fmaxf(__fsub_rn(y, G.hi[c]), 0.0f), hl = fmaxf(__fsub_rn(G.lo[c], y), 0.0f);
        g = __fmaf_rn(G.beta[c], __fsub_rn(hu, hl), g);
        const float yg = fminf(fmaxf(__fmaf_rn(-r, g, y), -1.0f), 1.0f);
        float v = __fmaf_rn(k.c_eps, ev[q], __fmaf_rn(k.c_x, xv[q], __fmul_rn(k.c_x0, yg)));
        if (k.sigma != 0.f) {
          const float z = noise ? zv[q] : philox_normal(seed, (row0 + (uint64_t)row) * (uint64_t)DP + (uint64_t)c, (uint32_t)step, LDP_PHILOX_STREAM_STEP);
          v = __fmaf_rn(k.sigma, z, v);
        }
        xo[q] = v;
      }
      if (VX && full) {
        *reinterpret_cast<float4*>(x_out + row * ldx + c0) = make_float4(xo[0], xo[1], xo[2], xo[3]);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (c0 + q < D) x_out[row * ldx + c0 + q] = xo[q];
      }
    }
    __syncthreads();                                         // (the next sample of this work-group overwrites y_s)
  }
}

// J of `rows` samples (T, D) with row stride D: sample r is costed with row r / n_per of the guide (n_per candidates per observation).
// One wave per sample.  Lane l adds the terms of the elements e = l, l + 64, ... (e = t * D + c) in that order, then the 64 partial sums
// meet in a fixed butterfly (xor 32, 16, 8, 4, 2, 1); out[r] = 0.5 * the total.  The term of one element, every operation rounded once:
//   a = rn(wg * rn(d * d)),                          d = rn(y - target)
//   s = t < T-1 ? rn(f * f) : 0,                     f = rn(y_next - y);      t == 0 && anchor:  s = rn(fma(da, da, s)),  da = rn(y - anchor)
//   a = rn(fma(lam, s, a))
//   a = rn(fma(beta, rn(fma(hu, hu, rn(hl * hl))), a)),     hu = max(rn(y - hi), 0),  hl = max(rn(lo - y), 0)
// The result depends on the sample and its guide row alone: bitwise the same whatever the batch around it.
__global__ __launch_bounds__(64) void plan_guide_cost_kernel(const float* __restrict__ x, GuideDev G, float* __restrict__ out, int64_t rows,
                                                             int n_per, int T, int D) {
  const int lane = threadIdx.x;
  for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
    const int64_t gb = r / n_per;
    const float* xs = x + (size_t)r * T * D;
    float acc = 0.0f;
    for (int e = lane; e < T * D; e += 64) {
      const int t = e / D, c = e - t * D;
      const float y = xs[e];
      const size_t ge = ((size_t)gb * T + t) * G.ldg + c;
      const float d = __fsub_rn(y, G.target[ge]);
      float a = __fmul_rn(G.wg[ge], __fmul_rn(d, d));
      float s = 0.0f;
      if (t < T - 1) { const float f = __fsub_rn(xs[e + D], y); s = __fmul_rn(f, f); }
      if (t == 0 && G.anchor) { const float da = __fsub_rn(y, G.anchor[(size_t)gb * G.ldg + c]); s = __fmaf_rn(da, da, s); }
      a = __fmaf_rn(G.lam[c], s, a);
      const float hu = fmaxf(__fsub_rn(y, G.hi[c]), 0.0f), hl = fmaxf(__fsub_rn(G.lo[c], y), 0.0f);
      a = __fmaf_rn(G.beta[c], __fmaf_rn(hu, hu, __fmul_rn(hl, hl)), a);
      acc = __fadd_rn(acc, a);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc = __fadd_rn(acc, __shfl_xor(acc, m, 64));
    if (lane == 0) out[r] = __fmul_rn(0.5f, acc);
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int check_guide_shape(int T, int D) {
  if (T < 1 || T > GUIDE_MAX_T || D < 1 || D > GUIDE_MAX_D)
    return fail(LDP_EINVAL, "the guide kernels serve pred_horizon <= %d and obs_dim <= %d, got %d and %d", GUIDE_MAX_T, GUIDE_MAX_D, T, D);
  return LDP_OK;
}

int plan_guide_step_launch(const float* x, const float* eps, const float* noise, float* x_out, const GuideDev& G, int ldx, int B, int T, int D,
                           int DP, const StepCoef& k, int step, const uint64_t* ctl, uint64_t seed, uint64_t row0, hipStream_t st) {
  LDP_TRY(check_guide_shape(T, D));
  const dim3 grid((unsigned)std::min<int64_t>(B, GUIDE_MAX_BLOCKS)), block(256);
  const bool vx = ldx % 4 == 0 && aligned16(x) && aligned16(x_out);
  const bool vg = G.ldg % 4 == 0 && aligned16(G.target) && aligned16(G.wg) && (!G.anchor || aligned16(G.anchor));
  const bool ve = D % 4 == 0 && aligned16(eps) && (!noise || aligned16(noise));
#define LDP_GUIDE(VX, VG, VE) \
  hipLaunchKernelGGL((plan_guide_step_kernel<VX, VG, VE>), grid, block, 0, st, x, eps, noise, x_out, G, ldx, B, T, D, DP, k, step, ctl, seed, row0)
  if (vx && vg && ve) LDP_GUIDE(true, true, true);
  else if (vx && vg) LDP_GUIDE(true, true, false);
  else LDP_GUIDE(false, false, false);
#undef LDP_GUIDE
  LDP_HIP(hipGetLastError());
  return LDP_OK;
}

GuideDev staged_guide(const PlannerState& P, bool anchor) {
  const float* col = P.gcol.f();
  return GuideDev{P.gtarget.f(), P.gwg.f(), anchor ? P.ganchor.f() : nullptr, col, col + GUIDE_MAX_D, col + 2 * GUIDE_MAX_D, col + 3 * GUIDE_MAX_D,
                  col + 4 * GUIDE_MAX_D, P.DP};
}

}  // namespace

int check_guide(const GuideSpec* g, int D, int n_steps, int sampler) {
  if (!g) return LDP_OK;
  if (sampler == LDP_SAMPLER_DPMPP) return fail(LDP_EINVAL, "sampler %d (DPM-Solver++) with a guide is not built: guidance runs under DDPM and DDIM", sampler);
  if (!g->target) return fail(LDP_EINVAL, "target is required");
  if (!g->wg) return fail(LDP_EINVAL, "wg is required");
  if (!g->lam || !g->beta || !g->lo || !g->hi) return fail(LDP_EINVAL, "lam, beta, lo and hi are required (host arrays of obs_dim = %d floats)", D);
  if (!g->rho) return fail(LDP_EINVAL, "rho is required");
  if (g->n_rho != n_steps) return fail(LDP_EINVAL, "rho has %d entries: a guided loop of n_steps = %d needs one per step", g->n_rho, n_steps);
  for (int i = 0; i < g->n_rho; ++i)
    if (!(g->rho[i] >= 0.0f) || !std::isfinite(g->rho[i])) return fail(LDP_EINVAL, "rho[%d] = %g must be finite and >= 0", i, (double)g->rho[i]);
  for (int c = 0; c < D; ++c) {
    if (!(g->lam[c] >= 0.0f) || !std::isfinite(g->lam[c])) return fail(LDP_EINVAL, "lam[%d] = %g must be finite and >= 0", c, (double)g->lam[c]);
    if (!(g->beta[c] >= 0.0f) || !std::isfinite(g->beta[c])) return fail(LDP_EINVAL, "beta[%d] = %g must be finite and >= 0", c, (double)g->beta[c]);
    if (!(g->lo[c] <= g->hi[c])) return fail(LDP_EINVAL, "lo[%d] = %g > hi[%d] = %g", c, (double)g->lo[c], c, (double)g->hi[c]);
  }
  return LDP_OK;
}

int guide_stage(ldp_handle* h, const GuideSpec& g, int B, int Bg, hipStream_t st) {
  PlannerState& P = h->pl;
  LDP_TRY(check_guide_shape(P.T, P.D));
  const size_t rows = (size_t)std::max(Bg, (P.ws_B + 15) / 16 * 16);      // (grows with the workspace, not call by call)
  const size_t elems = rows * P.T * P.DP;
  if (elems * 4 > P.gtarget.bytes || rows * P.DP * 4 > P.ganchor.bytes || !P.gcol.p) {
    if (P.gtarget.p) drop_graphs(h);                         // captured guide nodes point into these buffers
    LDP_TRY(P.gtarget.alloc(elems * 4));
    LDP_TRY(P.gwg.alloc(elems * 4));
    LDP_TRY(P.ganchor.alloc(rows * P.DP * 4));
    LDP_TRY(P.gcol.alloc((4 * GUIDE_MAX_D + GUIDE_MAX_STEPS) * 4));
    // padding columns and the rows beyond the real ones are never written below: keep them defined
    LDP_HIP(hipMemsetAsync(P.gtarget.p, 0, P.gtarget.bytes, st));
    LDP_HIP(hipMemsetAsync(P.gwg.p, 0, P.gwg.bytes, st));
    LDP_HIP(hipMemsetAsync(P.ganchor.p, 0, P.ganchor.bytes, st));
    LDP_HIP(hipMemsetAsync(P.gcol.p, 0, P.gcol.bytes, st));
  }
  LDP_TRY(pad_rows_launch(g.target, P.gtarget.f(), (int64_t)B * P.T, P.D, P.DP, st));
  LDP_TRY(pad_rows_launch(g.wg, P.gwg.f(), (int64_t)B * P.T, P.D, P.DP, st));
  if (g.anchor) LDP_TRY(pad_rows_launch(g.anchor, P.ganchor.f(), B, P.D, P.DP, st));
  // the host vectors as one copy: [lam | beta | lo | hi] at GUIDE_MAX_D floats each, then the step sizes
  // (pageable host memory: the runtime has read it when the call returns)
  std::vector<float> col((size_t)4 * GUIDE_MAX_D + g.n_rho, 0.0f);
  const float* cols[4] = {g.lam, g.beta, g.lo, g.hi};
  for (int j = 0; j < 4; ++j) std::copy(cols[j], cols[j] + P.D, col.begin() + j * GUIDE_MAX_D);
  std::copy(g.rho, g.rho + g.n_rho, col.begin() + 4 * GUIDE_MAX_D);
  LDP_HIP(hipMemcpyAsync(P.gcol.p, col.data(), col.size() * 4, hipMemcpyHostToDevice, st));
  return LDP_OK;
}

int planner_guide_step(ldp_handle* h, int Bg, const LoopSpec& L, const StepCoef& k, const float* noise, int i, hipStream_t q) {
  PlannerState& P = h->pl;
  LDP_TRY(plan_guide_step_launch(P.state.f(), P.solver_eps.f(), noise, P.state.f(), staged_guide(P, L.guide == LDP_GUIDE_ANCHOR), P.DP, Bg, P.T,
                                 P.D, P.DP, k, i, h->ctl_planner(), 0, 0, q));
  h->last_total_launches++;
  return LDP_OK;
}

}  // namespace ldp

using namespace ldp;

extern "C" {

int ldp_plan_guide_step(ldp_handle* h, const float* x, const float* eps, const float* noise, const float* target, const float* wg,
                        const float* anchor, const float* lam, const float* beta, const float* lo, const float* hi, const float* rho,
                        int32_t sampler, int32_t n_steps, int32_t step, uint64_t seed, int64_t row_offset, float* x_out, int32_t ldx,
                        int32_t ldg, int32_t B, void* stream) {
  if (!h || !x || !x_out) return fail(LDP_EINVAL, "bad argument");
  if (B < 1) return fail(LDP_EINVAL, "B must be >= 1, got %d", B);
  if (!eps) return fail(LDP_EINVAL, "eps is required");
  if (!target) return fail(LDP_EINVAL, "target is required");
  if (!wg) return fail(LDP_EINVAL, "wg is required");
  if (!lam || !beta || !lo || !hi) return fail(LDP_EINVAL, "lam, beta, lo and hi are required");
  if (!rho) return fail(LDP_EINVAL, "rho is required");
  const int D = h->cfg.obs_dim, T = h->cfg.pred_horizon, n_train = h->cfg.planner_train_steps;
  if (sampler == LDP_SAMPLER_DPMPP) return fail(LDP_EINVAL, "sampler %d (DPM-Solver++) with a guide is not built: guidance runs under DDPM and DDIM", sampler);
  LDP_TRY(check_sampler(sampler, n_steps, n_train, "planner"));
  if (step < 0 || step >= n_steps) return fail(LDP_EINVAL, "step %d outside 0..n_steps-1 = %d", step, n_steps - 1);
  if (ldx < D) return fail(LDP_EINVAL, "ldx = %d must be >= obs_dim = %d", ldx, D);
  if (ldg < D) return fail(LDP_EINVAL, "ldg = %d must be >= obs_dim = %d", ldg, D);
  std::vector<StepCoef> coefs;
  make_step_coefs(n_train, n_steps, sampler, coefs);
  const GuideDev G{target, wg, anchor, lam, beta, lo, hi, rho, ldg};
  return plan_guide_step_launch(x, eps, noise, x_out, G, ldx, B, T, D, (D + 31) / 32 * 32, coefs[step], step, nullptr, seed,
                                (uint64_t)(row_offset * T), (hipStream_t)stream);
}

int ldp_plan_guide_cost(ldp_handle* h, const float* x, const float* target, const float* wg, const float* anchor, const float* lam,
                        const float* beta, const float* lo, const float* hi, int64_t rows, int32_t n_per, float* out, void* stream) {
  if (!h || !x || !out) return fail(LDP_EINVAL, "bad argument");
  if (n_per < 1) return fail(LDP_EINVAL, "n_per must be >= 1, got %d", n_per);
  if (rows < 1 || rows % n_per != 0) return fail(LDP_EINVAL, "rows = %lld must be a positive multiple of n_per = %d", (long long)rows, n_per);
  if (!target) return fail(LDP_EINVAL, "target is required");
  if (!wg) return fail(LDP_EINVAL, "wg is required");
  if (!lam || !beta || !lo || !hi) return fail(LDP_EINVAL, "lam, beta, lo and hi are required");
  const int D = h->cfg.obs_dim, T = h->cfg.pred_horizon;
  const GuideDev G{target, wg, anchor, lam, beta, lo, hi, nullptr, D};
  hipLaunchKernelGGL(plan_guide_cost_kernel, dim3((unsigned)std::min<int64_t>(rows, 65536)), dim3(64), 0, (hipStream_t)stream, x, G, out, rows,
                     n_per, T, D);
  LDP_HIP(hipGetLastError());
  return LDP_OK;
}

}  // extern "C"
