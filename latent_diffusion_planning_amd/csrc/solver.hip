// solver.hip -- DPM-Solver++(2M) on the clipped data prediction over a registered timestep table (include/ldp_hip.h "solver sampler",
// DESIGN.md 4.18): the table and its coefficient rows (host, float64 -> float32), the solver update as one elementwise launch behind
// every U-Net evaluation of a sampler-2 loop, and the buffers that loop keeps (the evaluation's eps and the previous step's x0).
// Exact fp32 on the VALU, one thread per group of four channels, no atomics, no LDS, vector stores only.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "engine.hpp"

namespace ldp {
namespace {

constexpr unsigned SOLVER_MAX_BLOCKS = 2048;      // 8 work-groups of 256 threads per CU on 256 CUs: the rest is strided

// One solver update over `rows` rows of D real channels, every rounding spelled out:
//   x0  = clamp(rn(rn(fma(-sg, eps, x)) * inv_a), -1, 1)             (the scheduler's clip_sample)
//   Dv  = second ? rn(fma(w, rn(x0 - x0_prev), x0)) : x0
//   x'  = rn(fma(c_x, x, rn(c_D * Dv)));     x0_out = x0
// x / x_out have row stride ldx, x0_prev / x0_out ldh, eps lde (the loop: DP, DP and D; a stand-alone call: D everywhere).  Only the
// columns c < D are read or written: the padding columns of a padded row keep what they hold.
// VX / VH / VE: that operand's row stride is a multiple of four and its bases are 16-byte aligned, so a thread whose four columns all
// lie below D moves them as one 16-byte access; the group that straddles D and every operand that cannot be vectorised go element by
// element (32-bit accesses).  x_out may be x and x0_out may be x0_prev (no __restrict__ on them): a thread reads its four elements of
// every operand before it stores any.
template <bool VX, bool VH, bool VE>
__global__ __launch_bounds__(256) void plan_solver_kernel(const float* x, const float* __restrict__ eps, const float* x0_prev, float* x_out,
                                                          float* x0_out, int ldx, int ldh, int lde, int64_t rows, int D, SolverCoef k,
                                                          int second) {
  const int gpr = (D + 3) / 4;                               // channel groups per row
  const int64_t n = rows * gpr;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / gpr;
    const int c0 = (int)(i - r * gpr) * 4;
    const bool full = c0 + 4 <= D;
    const size_t bx = (size_t)r * ldx + c0, bh = (size_t)r * ldh + c0, be = (size_t)r * lde + c0;
    float xv[4] = {0.f, 0.f, 0.f, 0.f}, ev[4] = {0.f, 0.f, 0.f, 0.f}, pv[4] = {0.f, 0.f, 0.f, 0.f};
    if (VX && full) {
      const float4 q = *reinterpret_cast<const float4*>(x + bx);
      xv[0] = q.x; xv[1] = q.y; xv[2] = q.z; xv[3] = q.w;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (c0 + q < D) xv[q] = x[bx + q];
    }
    if (VE && full) {
      const float4 q = *reinterpret_cast<const float4*>(eps + be);
      ev[0] = q.x; ev[1] = q.y; ev[2] = q.z; ev[3] = q.w;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (c0 + q < D) ev[q] = eps[be + q];
    }
    if (second) {
      if (VH && full) {
        const float4 q = *reinterpret_cast<const float4*>(x0_prev + bh);
        pv[0] = q.x; pv[1] = q.y; pv[2] = q.z; pv[3] = q.w;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (c0 + q < D) pv[q] = x0_prev[bh + q];
      }
    }
    float xo[4], x0o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float x0 = __fmul_rn(__fmaf_rn(-k.sg, ev[q], xv[q]), k.inv_a);
      x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
      const float dv = second ? __fmaf_rn(k.w, __fsub_rn(x0, pv[q]), x0) : x0;
      xo[q] = __fmaf_rn(k.c_x, xv[q], __fmul_rn(k.c_D, dv));
      x0o[q] = x0;
    }
    if (VX && full) {
      *reinterpret_cast<float4*>(x_out + bx) = make_float4(xo[0], xo[1], xo[2], xo[3]);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (c0 + q < D) x_out[bx + q] = xo[q];
    }
    if (VH && full) {
      *reinterpret_cast<float4*>(x0_out + bh) = make_float4(x0o[0], x0o[1], x0o[2], x0o[3]);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (c0 + q < D) x0_out[bh + q] = x0o[q];
    }
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

const SolverTable* solver_table(const ldp_handle* h, int n_steps) {
  const auto it = h->solver_tabs.find(n_steps);
  return it == h->solver_tabs.end() ? nullptr : &it->second;
}

// the rows of schedule.solver_coefficients: float64 from the float32 abar table until the final cast
void make_solver_coefs(int n_train, const std::vector<int32_t>& ts, std::vector<SolverCoef>& out) {
  std::vector<float> betas, alphas, acp;
  betas_squaredcos(n_train, betas, alphas, acp);
  const int n = (int)ts.size();
  out.assign(n, SolverCoef{});
  auto lam = [&](int t) { const double a = acp[t]; return 0.5 * std::log(a / (1.0 - a)); };
  double h_prev = 0.0;
  for (int i = 0; i < n; ++i) {
    const int t = ts[i];
    const double ab_t = acp[t];
    const double a_t = std::sqrt(ab_t), s_t = std::sqrt(1.0 - ab_t);
    SolverCoef c{};
    c.t = (float)t;
    c.inv_a = (float)(1.0 / a_t);
    c.sg = (float)s_t;
    if (i == n - 1) {                              // to the clean level: alpha_s = 1, sigma_s = 0
      c.c_x = 0.0f; c.c_D = 1.0f; c.w = 0.0f;
    } else {
      const int s = ts[i + 1];
      const double ab_s = acp[s];
      const double a_s = std::sqrt(ab_s), s_s = std::sqrt(1.0 - ab_s);
      const double hh = lam(s) - lam(t);
      c.c_x = (float)(s_s / s_t);
      c.c_D = (float)(a_s - s_s * a_t / s_t);
      c.w = i > 0 ? (float)(hh / (2.0 * h_prev)) : 0.0f;
      h_prev = hh;
    }
    out[i] = c;
  }
}

int plan_solver_launch(const float* x, const float* eps, const float* x0_prev, float* x_out, float* x0_out, int ldx, int ldh, int lde,
                       int64_t rows, int D, const SolverCoef& k, bool second, hipStream_t st) {
  const int64_t n = rows * ((D + 3) / 4);
  const dim3 grid((unsigned)std::min<int64_t>((n + 255) / 256, SOLVER_MAX_BLOCKS)), block(256);
  const bool vx = ldx % 4 == 0 && aligned16(x) && aligned16(x_out);
  const bool vh = ldh % 4 == 0 && aligned16(x0_out) && (!second || aligned16(x0_prev));
  const bool ve = lde % 4 == 0 && aligned16(eps);
#define LDP_SOLVER(VX, VH, VE) \
  hipLaunchKernelGGL((plan_solver_kernel<VX, VH, VE>), grid, block, 0, st, x, eps, x0_prev, x_out, x0_out, ldx, ldh, lde, rows, D, k, second ? 1 : 0)
  if (vx && vh && ve) LDP_SOLVER(true, true, true);
  else if (vx && vh) LDP_SOLVER(true, true, false);
  else LDP_SOLVER(false, false, false);
#undef LDP_SOLVER
  LDP_HIP(hipGetLastError());
  return LDP_OK;
}

int solver_workspace(ldp_handle* h, int Bg) {
  PlannerState& P = h->pl;
  const size_t rows = (size_t)std::max(Bg, (P.ws_B + 15) / 16 * 16) * P.T;      // (grows with the workspace, not call by call)
  if (rows * P.D * 4 > P.solver_eps.bytes || rows * P.DP * 4 > P.solver_x0.bytes) {
    if (P.solver_eps.p || P.solver_x0.p) drop_graphs(h);     // captured solver nodes point into these buffers
    LDP_TRY(P.solver_eps.alloc(rows * P.D * 4));
    LDP_TRY(P.solver_x0.alloc(rows * P.DP * 4));
    LDP_HIP(hipMemset(P.solver_x0.p, 0, P.solver_x0.bytes));      // (its padding columns are never written: keep them defined)
  }
  return LDP_OK;
}

int planner_solver_step(ldp_handle* h, int Bg, const SolverTable& tab, int i, bool second, hipStream_t q) {
  PlannerState& P = h->pl;
  LDP_TRY(plan_solver_launch(P.state.f(), P.solver_eps.f(), P.solver_x0.f(), P.state.f(), P.solver_x0.f(), P.DP, P.DP, P.D,
                             (int64_t)Bg * P.T, P.D, tab.rows[i], second, q));
  h->last_total_launches++;
  return LDP_OK;
}

}  // namespace ldp

using namespace ldp;

extern "C" {

int ldp_solver_timesteps(ldp_handle* h, const int32_t* ts_host, int32_t n_steps) {
  if (!h) return fail(LDP_EINVAL, "bad argument");
  const int n_train = h->cfg.planner_train_steps;
  if (n_steps < 1 || n_steps > n_train) return fail(LDP_EINVAL, "n_steps must be in 1..planner_train_steps = %d, got %d", n_train, n_steps);
  if (!ts_host) return fail(LDP_EINVAL, "ts is required");
  for (int i = 0; i < n_steps; ++i) {
    if (ts_host[i] < 0 || ts_host[i] >= n_train)
      return fail(LDP_EINVAL, "ts[%d] = %d outside 0..planner_train_steps-1 = %d", i, ts_host[i], n_train - 1);
    if (i > 0 && ts_host[i] >= ts_host[i - 1])
      return fail(LDP_EINVAL, "ts[%d] = %d does not lie below ts[%d] = %d: the table must be strictly decreasing", i, ts_host[i], i - 1,
                  ts_host[i - 1]);
  }
  if (ts_host[n_steps - 1] != 0) return fail(LDP_EINVAL, "ts[%d] = %d: the last entry must be 0", n_steps - 1, ts_host[n_steps - 1]);
  std::vector<int32_t> ts(ts_host, ts_host + n_steps);
  auto it = h->solver_tabs.find(n_steps);
  if (it != h->solver_tabs.end()) {
    if (it->second.ts == ts) return LDP_OK;                // the same table again: nothing to do
    drop_graphs(h);                                        // captured solver launches carry the old rows by value
  }
  SolverTable tab;
  tab.ts = ts;
  make_solver_coefs(n_train, tab.ts, tab.rows);
  h->solver_tabs[n_steps] = std::move(tab);
  return LDP_OK;
}

int ldp_plan_solver_step(ldp_handle* h, const float* x, const float* eps, const float* x0_prev, int32_t n_steps, int32_t step, float* x_out,
                         float* x0_out, int32_t B, void* stream) {
  if (!h || !x || !eps || !x_out || !x0_out) return fail(LDP_EINVAL, "bad argument");
  if (B < 1) return fail(LDP_EINVAL, "B must be >= 1, got %d", B);
  const SolverTable* tab = solver_table(h, n_steps);
  if (!tab) return fail(LDP_ESTATE, "no timestep table registered for n_steps = %d: call ldp_solver_timesteps first", n_steps);
  if (step < 0 || step >= n_steps) return fail(LDP_EINVAL, "step %d outside 0..n_steps-1 = %d", step, n_steps - 1);
  const int D = h->cfg.obs_dim, T = h->cfg.pred_horizon;      // (elementwise on caller memory: no weights needed)
  return plan_solver_launch(x, eps, x0_prev, x_out, x0_out, D, D, D, (int64_t)B * T, D, tab->rows[step],
                            x0_prev != nullptr && step < n_steps - 1, (hipStream_t)stream);
}

}  // extern "C"
