// compose.hip -- the planner's step kernel (include/ldp_hip.h "composed planning"): ONE launch behind every U-Net
// evaluation of a stepped loop (a guide, or sampler 2) -- the clipped data prediction, the guide's projected gradient step on it, the
// scheduler (DDPM / DDIM) or solver (DPM-Solver++(2M)) update, and the constraint overwrite at the next level; each part a template
// switch.  The guided step of guide.hip's entry point is <0, true, false>, the solver update of solver.hip's is <1, false, false>.
// Here: the kernel, its launch on the loop state from the buffers guide_stage / constrain_stage filled, the table-level
// constraint in front of a solver loop, and the stand-alone entry point.  The sampling entry points are engine.hip's.
// Exact fp32 on the VALU; with a guide a work-group owns whole samples (the stencil along T goes through LDS), without one the launch is
// plain elementwise; no atomics, vector stores only.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "engine.hpp"
#include "tconv.hpp"      // philox_normal

namespace ldp {
namespace {

constexpr unsigned COMPOSE_MAX_BLOCKS = 2048;     // 8 work-groups of 256 threads per CU on 256 CUs: the rest is strided
constexpr int COMPOSE_LDS_FLOATS = PLAN_MAX_T * PLAN_MAX_D;      // 8 KB: one sample's clipped data prediction

__device__ __forceinline__ void load4(const float* p, size_t base, int c0, int D, bool vec, float (&v)[4]) {
  if (vec) {
    const float4 q = *reinterpret_cast<const float4*>(p + base);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = c0 + q < D ? p[base + q] : 0.0f;
  }
}

// the four mask bytes of a channel group as one word (byte q: column c0 + q).  VG: ldc % 4 == 0 and the base is 4-byte aligned, so the
// word at c0 lies inside the row even for the group that straddles D (c0 + 4 <= ldc); columns >= D are masked out by the caller.
template <bool VG>
__device__ __forceinline__ uint32_t load_mask4(const uint8_t* m, size_t base, int c0, int D) {
  if (VG) return *reinterpret_cast<const uint32_t*>(m + base);
  uint32_t w = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (c0 + q < D) w |= (m[base + q] != 0 ? 1u : 0u) << (8 * q);
  return w;
}

__device__ __forceinline__ void store4(float* p, size_t base, int c0, int D, bool vec, const float (&v)[4]) {
  if (vec) {
    *reinterpret_cast<float4*>(p + base) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (c0 + q < D) p[base + q] = v[q];
  }
}

// update + constraint of one element whose guided data prediction is yg (steps 3 and 4 of the kernel's header comment)
template <int SAMPLER, bool CONSTRAIN>
__device__ __forceinline__ float compose_update(const ComposeArgs& A, float yg, float xv, float ev, float zv, float pv, float tv, uint32_t mbyte,
                                                uint64_t elem, uint64_t seed) {
  float v;
  if (SAMPLER == 0) {
    v = __fmaf_rn(A.c_eps, ev, __fmaf_rn(A.c_x, xv, __fmul_rn(A.c_y, yg)));
    if (A.sigma != 0.f) {
      const float z = A.noise ? zv : philox_normal(seed, elem, (uint32_t)A.step, LDP_PHILOX_STREAM_STEP);
      v = __fmaf_rn(A.sigma, z, v);
    }
  } else {
    const float dv = A.second ? __fmaf_rn(A.w, __fsub_rn(yg, pv), yg) : yg;
    v = __fmaf_rn(A.c_x, xv, __fmul_rn(A.c_y, dv));
  }
  if (CONSTRAIN && mbyte != 0u) {                             // a select, never a blend
    v = tv;
    if (A.c_noise) {
      const float z = philox_normal(seed, elem, (uint32_t)(A.step + 1), LDP_PHILOX_STREAM_CONSTRAIN);
      v = __fmaf_rn(A.ca, tv, __fmul_rn(A.cs, z));
    }
  }
  return v;
}

// The composed step of B samples of T rows and D real channels, in place on x when x_out == x (and on the history when h_out == h_prev).
// Per element, every operation rounded to fp32 once, in this order (r = rho[step]; y_prev / y_next: y at t-1 / t+1 of the same channel):
//   1  y    = clamp(rn(rn(fma(-s, eps, x)) * inv_a), -1, 1)
//   2  GUIDE:  g  = rn(wg * rn(y - target))
//              dn = t < T-1 ? rn(y - y_next) : 0;   dp = t > 0 ? rn(y - y_prev) : anchor ? rn(y - anchor) : 0
//              g  = rn(fma(lam, rn(dn + dp), g))
//              g  = rn(fma(beta, rn(max(rn(y - hi), 0) - max(rn(lo - y), 0)), g))
//              y' = clamp(rn(fma(-r, g, y)), -1, 1);    else y' = y
//   3  SAMPLER 0 (DDPM / DDIM):      x' = rn(fma(c_eps, eps, rn(fma(c_x, x, rn(c_y * y')))));   sigma != 0:  x' = rn(fma(sigma, z, x'))
//      SAMPLER 1 (DPM-Solver++ 2M):  Dv = second ? rn(fma(w, rn(y' - h_prev), y')) : y';   x' = rn(fma(c_x, x, rn(c_y * Dv)));   h_out = y'
//   4  CONSTRAIN, where mask != 0:   x' = c_noise ? fma(ca, target, rn(cs * z_c)) : target
// z = noise[r, c] when `noise` is given, else philox_normal(seed, (row0 + r) * DP + c, step, LDP_PHILOX_STREAM_STEP); z_c = philox_normal(seed,
// the same element, step + 1, LDP_PHILOX_STREAM_CONSTRAIN) -- plan_constrain_kernel's draw at level step + 1; r = b * T + t the local row and
// (seed, row0) read from `ctl` when there is one (inside a captured loop).  The history holds the GUIDED data prediction and is never
// overwritten by the constraint.
// GUIDE: a work-group owns whole samples: it fills LDS with one sample's y (phase 1), synchronises, and computes steps 2 - 4 of that sample
// from LDS (phase 2); x and eps are read again in phase 2 by the thread that read them in phase 1, which is also the only thread that
// stores these elements.  A sample with more channel groups than threads is looped over.  Without GUIDE there is no stencil: a plain
// grid-stride loop over the channel groups, no LDS.  Either way a thread reads all of its operands before it stores any, and no
// work-group reads what another writes; only the columns c < D are read or written.
// VX (x, x_out, h_prev, h_out) / VG (the guide's target, weights, anchor and the constraint's target and mask) / VE (eps, noise): that
// family's row stride is a multiple of four and its bases are 16-byte aligned (the mask's: 4-byte), so a thread whose four columns all lie
// below D moves them as one 16-byte access (four mask bytes: one 32-bit load); the group that straddles D and every family that cannot be
// vectorised go element by element.
template <int SAMPLER, bool GUIDE, bool CONSTRAIN, bool VX, bool VG, bool VE>
__global__ __launch_bounds__(256) void plan_compose_step_kernel(ComposeArgs A) {
  const int D = A.D, T = A.T;
  const int gpr = (D + 3) / 4;                               // channel groups per row
  uint64_t seed = A.seed, row0 = A.row0;
  if (A.ctl) { seed = A.ctl[0]; row0 = A.ctl[1]; }
  if constexpr (GUIDE) {
    __shared__ float y_s[COMPOSE_LDS_FLOATS];
    const int ls = gpr * 4;                                  // LDS row stride
    const int n = T * gpr;                                   // channel groups per sample
    const float r = A.rho[A.step];
    for (int b = blockIdx.x; b < A.B; b += gridDim.x) {
      // phase 1: the clipped data prediction of this sample
      for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int t = i / gpr, c0 = (i - t * gpr) * 4;
        const bool full = c0 + 4 <= D;
        const size_t row = (size_t)b * T + t;
        float xv[4], ev[4];
        load4(A.x, row * A.ldx + c0, c0, D, VX && full, xv);
        load4(A.eps, row * D + c0, c0, D, VE && full, ev);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float y = __fmul_rn(__fmaf_rn(-A.s, ev[q], xv[q]), A.inv_a);
          y_s[t * ls + c0 + q] = c0 + q < D ? fminf(fmaxf(y, -1.0f), 1.0f) : 0.0f;
        }
      }
      __syncthreads();
      // phase 2: gradient, projected step, update, constraint
      for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int t = i / gpr, c0 = (i - t * gpr) * 4;
        const bool full = c0 + 4 <= D;
        const size_t row = (size_t)b * T + t;
        float xv[4], ev[4], tv[4], wv[4], av[4] = {0.f, 0.f, 0.f, 0.f}, zv[4] = {0.f, 0.f, 0.f, 0.f}, pv[4] = {0.f, 0.f, 0.f, 0.f};
        float cv[4] = {0.f, 0.f, 0.f, 0.f};
        uint32_t m = 0;
        load4(A.x, row * A.ldx + c0, c0, D, VX && full, xv);
        load4(A.eps, row * D + c0, c0, D, VE && full, ev);
        load4(A.g_target, row * A.ldg + c0, c0, D, VG && full, tv);
        load4(A.g_wg, row * A.ldg + c0, c0, D, VG && full, wv);
        const bool anchored = t == 0 && A.g_anchor != nullptr;
        if (anchored) load4(A.g_anchor, (size_t)b * A.ldg + c0, c0, D, VG && full, av);
        if (SAMPLER == 0 && A.sigma != 0.f && A.noise) load4(A.noise, row * D + c0, c0, D, VE && full, zv);
        if (SAMPLER == 1 && A.second) load4(A.h_prev, row * A.ldx + c0, c0, D, VX && full, pv);
        if (CONSTRAIN) {
          m = load_mask4<VG>(A.c_mask, row * A.ldc + c0, c0, D);
          if (m != 0u) load4(A.c_target, row * A.ldc + c0, c0, D, VG && full, cv);
        }
        float xo[4], ho[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int c = c0 + q;
          xo[q] = 0.0f; ho[q] = 0.0f;
          if (c >= D) continue;
          const float y = y_s[t * ls + c];
          float g = __fmul_rn(wv[q], __fsub_rn(y, tv[q]));
          const float dn = t < T - 1 ? __fsub_rn(y, y_s[(t + 1) * ls + c]) : 0.0f;
          const float dp = t > 0 ? __fsub_rn(y, y_s[(t - 1) * ls + c]) : anchored ? __fsub_rn(y, av[q]) : 0.0f;
          g = __fmaf_rn(A.lam[c], __fadd_rn(dn, dp), g);
          const float hu = fmaxf(__fsub_rn(y, A.hi[c]), 0.0f), hl = fmaxf(__fsub_rn(A.lo[c], y), 0.0f);
          g = __fmaf_rn(A.beta[c], __fsub_rn(hu, hl), g);
          const float yg = fminf(fmaxf(__fmaf_rn(-r, g, y), -1.0f), 1.0f);
          ho[q] = yg;
          xo[q] = compose_update<SAMPLER, CONSTRAIN>(A, yg, xv[q], ev[q], zv[q], pv[q], cv[q], (m >> (8 * q)) & 0xffu,
                                                     (row0 + (uint64_t)row) * (uint64_t)A.DP + (uint64_t)c, seed);
        }
        store4(A.x_out, row * A.ldx + c0, c0, D, VX && full, xo);
        if (SAMPLER == 1) store4(A.h_out, row * A.ldx + c0, c0, D, VX && full, ho);
      }
      __syncthreads();                                       // (the next sample of this work-group overwrites y_s)
    }
  } else {
    const int64_t n = (int64_t)A.B * T * gpr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
      const int64_t row = i / gpr;
      const int c0 = (int)(i - row * gpr) * 4;
      const bool full = c0 + 4 <= D;
      float xv[4], ev[4], zv[4] = {0.f, 0.f, 0.f, 0.f}, pv[4] = {0.f, 0.f, 0.f, 0.f}, cv[4] = {0.f, 0.f, 0.f, 0.f};
      uint32_t m = 0;
      load4(A.x, (size_t)row * A.ldx + c0, c0, D, VX && full, xv);
      load4(A.eps, (size_t)row * D + c0, c0, D, VE && full, ev);
      if (SAMPLER == 0 && A.sigma != 0.f && A.noise) load4(A.noise, (size_t)row * D + c0, c0, D, VE && full, zv);
      if (SAMPLER == 1 && A.second) load4(A.h_prev, (size_t)row * A.ldx + c0, c0, D, VX && full, pv);
      if (CONSTRAIN) {
        m = load_mask4<VG>(A.c_mask, (size_t)row * A.ldc + c0, c0, D);
        if (m != 0u) load4(A.c_target, (size_t)row * A.ldc + c0, c0, D, VG && full, cv);
      }
      float xo[4], ho[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = c0 + q;
        xo[q] = 0.0f; ho[q] = 0.0f;
        if (c >= D) continue;
        const float y = fminf(fmaxf(__fmul_rn(__fmaf_rn(-A.s, ev[q], xv[q]), A.inv_a), -1.0f), 1.0f);
        ho[q] = y;
        xo[q] = compose_update<SAMPLER, CONSTRAIN>(A, y, xv[q], ev[q], zv[q], pv[q], cv[q], (m >> (8 * q)) & 0xffu,
                                                   (row0 + (uint64_t)row) * (uint64_t)A.DP + (uint64_t)c, seed);
      }
      store4(A.x_out, (size_t)row * A.ldx + c0, c0, D, VX && full, xo);
      if (SAMPLER == 1) store4(A.h_out, (size_t)row * A.ldx + c0, c0, D, VX && full, ho);
    }
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

template <int SAMPLER, bool GUIDE, bool CONSTRAIN>
void compose_launch_v(const ComposeArgs& A, bool vx, bool vg, bool ve, dim3 grid, hipStream_t st) {
  const dim3 block(256);
  if (vx && vg && ve) hipLaunchKernelGGL((plan_compose_step_kernel<SAMPLER, GUIDE, CONSTRAIN, true, true, true>), grid, block, 0, st, A);
  else if (vx && vg) hipLaunchKernelGGL((plan_compose_step_kernel<SAMPLER, GUIDE, CONSTRAIN, true, true, false>), grid, block, 0, st, A);
  else hipLaunchKernelGGL((plan_compose_step_kernel<SAMPLER, GUIDE, CONSTRAIN, false, false, false>), grid, block, 0, st, A);
}

}  // namespace

int plan_compose_launch(const ComposeArgs& A, bool solver, bool guide, bool constrain, hipStream_t st) {
  if (guide) LDP_TRY(check_guide_shape(A.T, A.D));
  const int64_t groups = (int64_t)A.B * A.T * ((A.D + 3) / 4);
  const dim3 grid(guide ? (unsigned)std::min<int64_t>(A.B, COMPOSE_MAX_BLOCKS)
                        : (unsigned)std::min<int64_t>((groups + 255) / 256, COMPOSE_MAX_BLOCKS));
  const bool vx = A.ldx % 4 == 0 && aligned16(A.x) && aligned16(A.x_out) &&
                  (!solver || (aligned16(A.h_out) && (!A.second || aligned16(A.h_prev))));
  const bool vg = (!guide || (A.ldg % 4 == 0 && aligned16(A.g_target) && aligned16(A.g_wg) && (!A.g_anchor || aligned16(A.g_anchor)))) &&
                  (!constrain || (A.ldc % 4 == 0 && aligned16(A.c_target) && aligned4(A.c_mask)));
  const bool ve = A.D % 4 == 0 && aligned16(A.eps) && (!A.noise || aligned16(A.noise));
  const int sel = (solver ? 4 : 0) | (guide ? 2 : 0) | (constrain ? 1 : 0);
  switch (sel) {
    case 0: compose_launch_v<0, false, false>(A, vx, vg, ve, grid, st); break;
    case 1: compose_launch_v<0, false, true>(A, vx, vg, ve, grid, st); break;
    case 2: compose_launch_v<0, true, false>(A, vx, vg, ve, grid, st); break;
    case 3: compose_launch_v<0, true, true>(A, vx, vg, ve, grid, st); break;
    case 4: compose_launch_v<1, false, false>(A, vx, vg, ve, grid, st); break;
    case 5: compose_launch_v<1, false, true>(A, vx, vg, ve, grid, st); break;
    case 6: compose_launch_v<1, true, false>(A, vx, vg, ve, grid, st); break;
    default: compose_launch_v<1, true, true>(A, vx, vg, ve, grid, st); break;
  }
  LDP_HIP(hipGetLastError());
  return LDP_OK;
}

void set_scheduler_coefs(ComposeArgs& A, const StepCoef& k) {
  A.s = k.sqrt_1mab; A.inv_a = k.inv_sqrt_ab; A.c_y = k.c_x0; A.c_x = k.c_x; A.c_eps = k.c_eps; A.sigma = k.sigma; A.w = 0.0f;
}
void set_solver_coefs(ComposeArgs& A, const SolverCoef& k) {
  A.s = k.sg; A.inv_a = k.inv_a; A.c_y = k.c_D; A.c_x = k.c_x; A.c_eps = 0.0f; A.sigma = 0.0f; A.w = k.w;
}

int compose_level_coefs(const ldp_handle* h, int sampler, int n_steps, int level, float* a, float* s) {
  if (sampler != LDP_SAMPLER_DPMPP) return level_coefs(h->cfg.planner_train_steps, n_steps, level, a, s);
  const SolverTable* tab = solver_table(h, n_steps);
  if (!tab) return fail(LDP_ESTATE, "no timestep table registered for n_steps = %d: call ldp_solver_timesteps first", n_steps);
  return table_level_coefs(h->cfg.planner_train_steps, tab->ts, level, a, s);
}

int planner_constrain_begin(ldp_handle* h, int Bg, const LoopSpec& L, int level, hipStream_t q) {
  if (L.sampler != LDP_SAMPLER_DPMPP) return planner_constrain_level(h, Bg, L, level, q);
  PlannerState& P = h->pl;
  float a = 1.0f, s = 0.0f;
  LDP_TRY(compose_level_coefs(h, L.sampler, L.n_steps, level, &a, &s));
  const bool noise = L.constrain == LDP_CONSTRAIN_REPAINT && level < L.n_steps;
  LDP_TRY(plan_constrain_launch(P.state.f(), P.ctarget.f(), P.cmask.as<uint8_t>(), P.state.f(), P.DP, (int64_t)Bg * P.T, P.D, P.DP, a, s, level,
                                noise, h->ctl_planner(), 0, 0, q));
  h->last_total_launches++;
  return LDP_OK;
}

int planner_compose_step(ldp_handle* h, int Bg, const LoopSpec& L, const StepCoef* k, const SolverCoef* ks, const float* noise, int i,
                         bool second, hipStream_t q) {
  PlannerState& P = h->pl;
  ComposeArgs A{};
  A.x = P.state.f(); A.x_out = P.state.f(); A.eps = P.solver_eps.f(); A.noise = noise;
  A.h_prev = P.solver_x0.f(); A.h_out = P.solver_x0.f();
  if (L.guide) {
    const float* col = P.gcol.f();
    A.g_target = P.gtarget.f(); A.g_wg = P.gwg.f(); A.g_anchor = L.guide == LDP_GUIDE_ANCHOR ? P.ganchor.f() : nullptr;
    A.lam = col; A.beta = col + PLAN_MAX_D; A.lo = col + 2 * PLAN_MAX_D; A.hi = col + 3 * PLAN_MAX_D; A.rho = col + 4 * PLAN_MAX_D;
  }
  if (L.constrain) {
    A.c_target = P.ctarget.f(); A.c_mask = P.cmask.as<uint8_t>();
    LDP_TRY(compose_level_coefs(h, L.sampler, L.n_steps, i + 1, &A.ca, &A.cs));
    A.c_noise = L.constrain == LDP_CONSTRAIN_REPAINT && i + 1 < L.n_steps ? 1 : 0;
  }
  A.ctl = h->ctl_planner();
  A.ldx = A.ldg = A.ldc = P.DP; A.B = Bg; A.T = P.T; A.D = P.D; A.DP = P.DP; A.step = i; A.second = second ? 1 : 0;
  if (ks) set_solver_coefs(A, *ks); else set_scheduler_coefs(A, *k);
  LDP_TRY(plan_compose_launch(A, ks != nullptr, L.guide != 0, L.constrain != 0, q));
  h->last_total_launches++;
  return LDP_OK;
}

}  // namespace ldp

using namespace ldp;

extern "C" {

int ldp_plan_compose_step(ldp_handle* h, const float* x, const float* eps, const float* noise, const float* x0_prev,
                          const ldp_plan_compose* parts, int32_t sampler, int32_t n_steps, int32_t step, int32_t second, uint64_t seed,
                          int64_t row_offset, float* x_out, float* x0_out, int32_t ldx, int32_t ldg, int32_t ldc, int32_t B, void* stream) {
  if (!h || !x || !x_out) return fail(LDP_EINVAL, "bad argument");
  if (B < 1) return fail(LDP_EINVAL, "B must be >= 1, got %d", B);
  if (!eps) return fail(LDP_EINVAL, "eps is required");
  const ldp_plan_compose none{};
  const ldp_plan_compose& C = parts ? *parts : none;
  const bool guide = C.g_target || C.g_wg || C.rho, constrain = C.target || C.mask;
  const int D = h->cfg.obs_dim, T = h->cfg.pred_horizon, n_train = h->cfg.planner_train_steps;
  if (guide) {
    if (!C.g_target) return fail(LDP_EINVAL, "g_target is required");
    if (!C.g_wg) return fail(LDP_EINVAL, "g_wg is required");
    if (!C.lam || !C.beta || !C.lo || !C.hi) return fail(LDP_EINVAL, "lam, beta, lo and hi are required");
    if (!C.rho) return fail(LDP_EINVAL, "rho is required");
    if (C.n_rho != n_steps) return fail(LDP_EINVAL, "rho has %d entries: n_steps = %d needs one per step", C.n_rho, n_steps);
    if (ldg < D) return fail(LDP_EINVAL, "ldg = %d must be >= obs_dim = %d", ldg, D);
  }
  if (constrain) {
    if (!C.target) return fail(LDP_EINVAL, "target is required");
    if (!C.mask) return fail(LDP_EINVAL, "mask is required");
    LDP_TRY(check_constrain_mode(C.mode));
    if (ldc < D) return fail(LDP_EINVAL, "ldc = %d must be >= obs_dim = %d", ldc, D);
  }
  LDP_TRY(check_sampler(sampler, n_steps, n_train, "planner", h));
  if (step < 0 || step >= n_steps) return fail(LDP_EINVAL, "step %d outside 0..n_steps-1 = %d", step, n_steps - 1);
  if (ldx < D) return fail(LDP_EINVAL, "ldx = %d must be >= obs_dim = %d", ldx, D);
  const bool solver = sampler == LDP_SAMPLER_DPMPP;
  if (solver && !x0_out) return fail(LDP_EINVAL, "x0_out is required under sampler %d", sampler);
  if (solver && second && !x0_prev) return fail(LDP_EINVAL, "second order needs x0_prev");
  ComposeArgs A{};
  A.x = x; A.x_out = x_out; A.eps = eps; A.noise = noise; A.h_prev = x0_prev; A.h_out = x0_out;
  A.g_target = C.g_target; A.g_wg = C.g_wg; A.g_anchor = C.g_anchor; A.lam = C.lam; A.beta = C.beta; A.lo = C.lo; A.hi = C.hi; A.rho = C.rho;
  A.c_target = C.target; A.c_mask = C.mask;
  A.ctl = nullptr; A.seed = seed; A.row0 = (uint64_t)(row_offset * T);
  A.ldx = ldx; A.ldg = ldg; A.ldc = ldc; A.B = B; A.T = T; A.D = D; A.DP = (D + 31) / 32 * 32; A.step = step;
  A.second = solver && second && step < n_steps - 1 ? 1 : 0;
  if (constrain) {
    LDP_TRY(compose_level_coefs(h, sampler, n_steps, step + 1, &A.ca, &A.cs));
    A.c_noise = C.mode == LDP_CONSTRAIN_REPAINT && step + 1 < n_steps ? 1 : 0;
  }
  if (solver) {
    set_solver_coefs(A, solver_table(h, n_steps)->rows[step]);
  } else {
    std::vector<StepCoef> coefs;
    make_step_coefs(n_train, n_steps, sampler, coefs);
    set_scheduler_coefs(A, coefs[step]);
  }
  return plan_compose_launch(A, solver, guide, constrain, (hipStream_t)stream);
}

}  // extern "C"
