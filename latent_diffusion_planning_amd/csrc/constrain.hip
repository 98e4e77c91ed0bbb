// constrain.hip -- constrained planning (include/ldp_hip.h "constrained planning"): the constraint operation C_j that
// overwrites the masked entries of the planner state with the known values at the noise level of level j (inpainting), and the staging of
// a caller's target / mask into the handle-owned padded buffers the captured loop reads.
// Exact fp32 on the VALU, one thread per group of four channels, no atomics, vector stores only.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "engine.hpp"

namespace ldp {
namespace {

constexpr unsigned CONSTRAIN_MAX_BLOCKS = 2048;      // 8 work-groups of 256 threads per CU on 256 CUs: the rest is strided

// out[r, c] = mask[r, c] != 0 && c < D ? v(r, c) : x[r, c]        -- a select, never a blend: target is not touched by arithmetic
//   v = target[r, c]                                                (noise == 0: clamp, and every mode at the last level)
//   v = fma(a, target[r, c], rn(s * z)),  z = philox_normal(seed, (row0 + r) * DP + c, step = level, LDP_PHILOX_STREAM_CONSTRAIN)   (repaint)
// r = b * T + j is the local row; x, target, mask and out all have row stride ld (DP: the padded loop state, in place; D: caller memory).
// (seed, row0) come from the control block `ctl` when there is one (inside a captured loop: a graph never bakes a seed), else from the
// arguments.  The products are spelled with explicit roundings, as in plan_warm_init_kernel.
// VEC (ld % 4 == 0, every base 16-byte aligned): 16-byte loads of state and target, one 32-bit load of four mask bytes, a 16-byte store.
// x and out may be the same memory (no __restrict__ on them): a thread reads its four elements before it stores them.
template <bool VEC>
__global__ __launch_bounds__(256) void plan_constrain_kernel(const float* x, const float* __restrict__ target,
                                                             const uint8_t* __restrict__ mask, float* out, int ld, int64_t rows, int D,
                                                             int DP, float a, float s, int level, int noise,
                                                             const uint64_t* __restrict__ ctl, uint64_t seed, uint64_t row0) {
  const int gpr = (ld + 3) / 4;                              // channel groups per row
  const int64_t n = rows * gpr;
  if (ctl) { seed = ctl[0]; row0 = ctl[1]; }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / gpr;
    const int c0 = (int)(i - r * gpr) * 4;
    const size_t base = (size_t)r * ld + c0;
    float xv[4] = {0.f, 0.f, 0.f, 0.f}, tv[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t m = 0;
    if (VEC) {
      m = *reinterpret_cast<const uint32_t*>(mask + base);
      if (m == 0 && out == x) continue;                      // in place and nothing masked: the four elements stay as they are
      const float4 xq = *reinterpret_cast<const float4*>(x + base);
      const float4 tq = *reinterpret_cast<const float4*>(target + base);
      xv[0] = xq.x; xv[1] = xq.y; xv[2] = xq.z; xv[3] = xq.w;
      tv[0] = tq.x; tv[1] = tq.y; tv[2] = tq.z; tv[3] = tq.w;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (c0 + q < ld) {
          xv[q] = x[base + q];
          tv[q] = target[base + q];
          m |= (mask[base + q] != 0 ? 1u : 0u) << (8 * q);
        }
    }
    float o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = c0 + q;
      float v = xv[q];
      if (((m >> (8 * q)) & 0xffu) != 0u && c < D) {
        v = tv[q];
        if (noise) {
          const float z = philox_normal(seed, (row0 + (uint64_t)r) * (uint64_t)DP + (uint64_t)c, (uint32_t)level, LDP_PHILOX_STREAM_CONSTRAIN);
          v = __fmaf_rn(a, tv[q], __fmul_rn(s, z));
        }
      }
      o[q] = v;
    }
    if (VEC) {
      *reinterpret_cast<float4*>(out + base) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (c0 + q < ld) out[base + q] = o[q];
    }
  }
}

// (B, T, D) target / mask in caller memory -> (Bg, T, DP) handle buffers: zero beyond D and beyond the B real rows; the mask as 0 / 1
__global__ __launch_bounds__(256) void constrain_stage_kernel(const float* __restrict__ target, const uint8_t* __restrict__ mask,
                                                              float* __restrict__ tdst, uint8_t* __restrict__ mdst, int64_t rows,
                                                              int64_t rows_pad, int D, int DP) {
  const int gpr = DP / 4;
  const int64_t n = rows_pad * gpr;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / gpr;
    const int c0 = (int)(i - r * gpr) * 4;
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t m = 0;
    if (r < rows) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (c0 + q < D) {
          t[q] = target[(size_t)r * D + c0 + q];
          m |= (mask[(size_t)r * D + c0 + q] != 0 ? 1u : 0u) << (8 * q);
        }
    }
    *reinterpret_cast<float4*>(tdst + (size_t)r * DP + c0) = make_float4(t[0], t[1], t[2], t[3]);
    *reinterpret_cast<uint32_t*>(mdst + (size_t)r * DP + c0) = m;
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

unsigned capped_grid(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, CONSTRAIN_MAX_BLOCKS); }

}  // namespace

int check_constrain_mode(int mode) {
  if (mode != LDP_CONSTRAIN_CLAMP && mode != LDP_CONSTRAIN_REPAINT)
    return fail(LDP_EINVAL, "mode must be LDP_CONSTRAIN_CLAMP (%d) or LDP_CONSTRAIN_REPAINT (%d), got %d", LDP_CONSTRAIN_CLAMP,
                LDP_CONSTRAIN_REPAINT, mode);
  return LDP_OK;
}

int level_coefs(int n_train, int n_steps, int level, float* a, float* s) {
  if (level < 0 || level > n_steps) return fail(LDP_EINVAL, "level %d outside 0..n_steps = %d", level, n_steps);
  if (level == n_steps) { *a = 1.0f; *s = 0.0f; return LDP_OK; }
  return warm_coefs(n_train, n_steps, level, a, s);      // t_level = (n_steps - 1 - level) * (n_train / n_steps): warm_coefs' convention
}

// the same over a registered timestep table (sampler 2, compose.hip): level j < n has the timestep ts[j]
int table_level_coefs(int n_train, const std::vector<int32_t>& ts, int level, float* a, float* s) {
  const int n_steps = (int)ts.size();
  if (level < 0 || level > n_steps) return fail(LDP_EINVAL, "level %d outside 0..n_steps = %d", level, n_steps);
  if (level == n_steps) { *a = 1.0f; *s = 0.0f; return LDP_OK; }
  std::vector<float> betas, alphas, acp;
  betas_squaredcos(n_train, betas, alphas, acp);
  const double a_t = acp[ts[level]];              // float32 table, float64 from here (warm_coefs' convention)
  *a = (float)std::sqrt(a_t);
  *s = (float)std::sqrt(1.0 - a_t);
  return LDP_OK;
}

int plan_constrain_launch(const float* x, const float* target, const uint8_t* mask, float* out, int ld, int64_t rows, int D, int DP, float a,
                          float s, int level, bool noise, const uint64_t* ctl, uint64_t seed, uint64_t row0, hipStream_t st) {
  const int64_t n = rows * ((ld + 3) / 4);
  const dim3 grid(capped_grid(n)), block(256);
  const bool vec = ld % 4 == 0 && aligned16(x) && aligned16(target) && aligned16(out) && aligned4(mask);
  if (vec)
    hipLaunchKernelGGL((plan_constrain_kernel<true>), grid, block, 0, st, x, target, mask, out, ld, rows, D, DP, a, s, level, noise ? 1 : 0, ctl,
                       seed, row0);
  else
    hipLaunchKernelGGL((plan_constrain_kernel<false>), grid, block, 0, st, x, target, mask, out, ld, rows, D, DP, a, s, level, noise ? 1 : 0, ctl,
                       seed, row0);
  LDP_HIP(hipGetLastError());
  return LDP_OK;
}

int constrain_stage(ldp_handle* h, const float* target, const uint8_t* mask, int B, int Bg, hipStream_t st) {
  PlannerState& P = h->pl;
  const size_t elems = (size_t)std::max(Bg, (P.ws_B + 15) / 16 * 16) * P.T * P.DP;      // (grows with the workspace, not call by call)
  if (elems * 4 > P.ctarget.bytes || elems > P.cmask.bytes) {
    drop_graphs(h);                                          // captured constraint nodes point into these buffers
    LDP_TRY(P.ctarget.alloc(elems * 4));
    LDP_TRY(P.cmask.alloc(elems));
  }
  const int64_t rows_pad = (int64_t)Bg * P.T;
  hipLaunchKernelGGL(constrain_stage_kernel, dim3(capped_grid(rows_pad * (P.DP / 4))), dim3(256), 0, st, target, mask, P.ctarget.f(),
                     P.cmask.as<uint8_t>(), (int64_t)B * P.T, rows_pad, P.D, P.DP);
  LDP_HIP(hipGetLastError());
  return LDP_OK;
}

int planner_constrain_level(ldp_handle* h, int Bg, const LoopSpec& L, int level, hipStream_t q) {
  PlannerState& P = h->pl;
  float a = 1.0f, s = 0.0f;
  LDP_TRY(level_coefs(P.n_train, L.n_steps, level, &a, &s));
  const bool noise = L.constrain == LDP_CONSTRAIN_REPAINT && level < L.n_steps;
  LDP_TRY(plan_constrain_launch(P.state.f(), P.ctarget.f(), P.cmask.as<uint8_t>(), P.state.f(), P.DP, (int64_t)Bg * P.T, P.D, P.DP, a, s, level,
                                noise, h->ctl_planner(), 0, 0, q));
  h->last_total_launches++;
  return LDP_OK;
}

}  // namespace ldp

using namespace ldp;

extern "C" {

int ldp_plan_constrain(ldp_handle* h, const float* x, const float* target, const uint8_t* mask, int32_t mode, int32_t sampler,
                       int32_t n_steps, int32_t level, uint64_t seed, int64_t row_offset, float* x_out, int32_t B, void* stream) {
  if (!h || !x || !x_out) return fail(LDP_EINVAL, "bad argument");
  if (B < 1) return fail(LDP_EINVAL, "B must be >= 1, got %d", B);
  if (!h->pl.ready) return fail(LDP_ESTATE, "planner weights not finalized");
  if (!target) return fail(LDP_EINVAL, "target is required");
  if (!mask) return fail(LDP_EINVAL, "mask is required");
  LDP_TRY(check_constrain_mode(mode));
  PlannerState& P = h->pl;
  LDP_TRY(check_sampler(sampler, n_steps, P.n_train, "planner"));
  float a = 1.0f, s = 0.0f;
  LDP_TRY(level_coefs(P.n_train, n_steps, level, &a, &s));
  return plan_constrain_launch(x, target, mask, x_out, P.D, (int64_t)B * P.T, P.D, P.DP, a, s, level,
                               mode == LDP_CONSTRAIN_REPAINT && level < n_steps, nullptr, seed, (uint64_t)(row_offset * P.T),
                               (hipStream_t)stream);
}

}  // extern "C"
