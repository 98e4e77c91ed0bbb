// guide.hip -- guided planning (include/ldp_hip.h "guided planning"): one projected gradient step on a trajectory cost
// inside every denoising step.  The cost per sample, on the clipped data prediction y (T, D):
//   J(y) = 1/2 sum_{t,c} wg[t,c] (y[t,c] - target[t,c])^2                                            soft goals / waypoints
//        + 1/2 sum_c lam[c] ( sum_{t < T-1} (y[t+1,c] - y[t,c])^2 + [anchor] (y[0,c] - anchor[c])^2 )   smoothness, continuity
//        + 1/2 sum_{t,c} beta[c] ( max(y - hi[c], 0)^2 + max(lo[c] - y, 0)^2 )                         box bounds
// The guided step itself is compose.hip's plan_compose_step_kernel<0, true, false> (one launch behind every U-Net evaluation).  Here: the
// cost (one launch), the staging of a call's guide into the handle-owned buffers the captured loop reads, and the two stand-alone entry
// points.  Exact fp32 on the VALU; no atomics, vector stores only.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "engine.hpp"

namespace ldp {
namespace {

// What a guide is made of, as the cost kernel reads it.  target / wg: (B, T, ldg); anchor: (B, ldg) or nullptr (no continuity term); lam,
// beta, lo, hi: (D).  All device memory.
struct GuideDev {
  const float* target; const float* wg; const float* anchor;
  const float* lam; const float* beta; const float* lo; const float* hi;
  int ldg;
};

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

}  // namespace

int check_guide_shape(int T, int D) {
  if (T < 1 || T > PLAN_MAX_T || D < 1 || D > PLAN_MAX_D)
    return fail(LDP_EINVAL, "the guide kernels serve pred_horizon <= %d and obs_dim <= %d, got %d and %d", PLAN_MAX_T, PLAN_MAX_D, T, D);
  return LDP_OK;
}

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
    LDP_TRY(P.gcol.alloc((4 * PLAN_MAX_D + PLAN_MAX_STEPS) * 4));
    // padding columns and the rows beyond the real ones are never written below: keep them defined
    LDP_HIP(hipMemsetAsync(P.gtarget.p, 0, P.gtarget.bytes, st));
    LDP_HIP(hipMemsetAsync(P.gwg.p, 0, P.gwg.bytes, st));
    LDP_HIP(hipMemsetAsync(P.ganchor.p, 0, P.ganchor.bytes, st));
    LDP_HIP(hipMemsetAsync(P.gcol.p, 0, P.gcol.bytes, st));
  }
  LDP_TRY(pad_rows_launch(g.target, P.gtarget.f(), (int64_t)B * P.T, P.D, P.DP, st));
  LDP_TRY(pad_rows_launch(g.wg, P.gwg.f(), (int64_t)B * P.T, P.D, P.DP, st));
  if (g.anchor) LDP_TRY(pad_rows_launch(g.anchor, P.ganchor.f(), B, P.D, P.DP, st));
  // the host vectors as one copy: [lam | beta | lo | hi] at PLAN_MAX_D floats each, then the step sizes
  // (pageable host memory: the runtime has read it when the call returns)
  std::vector<float> col((size_t)4 * PLAN_MAX_D + g.n_rho, 0.0f);
  const float* cols[4] = {g.lam, g.beta, g.lo, g.hi};
  for (int j = 0; j < 4; ++j) std::copy(cols[j], cols[j] + P.D, col.begin() + j * PLAN_MAX_D);
  std::copy(g.rho, g.rho + g.n_rho, col.begin() + 4 * PLAN_MAX_D);
  LDP_HIP(hipMemcpyAsync(P.gcol.p, col.data(), col.size() * 4, hipMemcpyHostToDevice, st));
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
  ComposeArgs A{};
  A.x = x; A.x_out = x_out; A.eps = eps; A.noise = noise;
  A.g_target = target; A.g_wg = wg; A.g_anchor = anchor; A.lam = lam; A.beta = beta; A.lo = lo; A.hi = hi; A.rho = rho;
  A.seed = seed; A.row0 = (uint64_t)(row_offset * T);
  A.ldx = ldx; A.ldg = ldg; A.B = B; A.T = T; A.D = D; A.DP = (D + 31) / 32 * 32; A.step = step;
  set_scheduler_coefs(A, coefs[step]);
  return plan_compose_launch(A, false, true, false, (hipStream_t)stream);
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
  const GuideDev G{target, wg, anchor, lam, beta, lo, hi, D};
  hipLaunchKernelGGL(plan_guide_cost_kernel, dim3((unsigned)std::min<int64_t>(rows, 65536)), dim3(64), 0, (hipStream_t)stream, x, G, out, rows,
                     n_per, T, D);
  LDP_HIP(hipGetLastError());
  return LDP_OK;
}

}  // extern "C"
