// replan.hip -- warm-started replanning (include/ldp_hip.h "warm-started replanning"): the initial state of a planner loop
// that resumes at executed step `step_begin` from the previous call's plan, and the write-back of the new state into the slot table.
// Exact fp32 on the VALU, one thread per group of four output channels, no atomics, vector stores only.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "engine.hpp"

namespace ldp {
namespace {

// x[b, j, c] = a * x_prev[src(b), min(j + shift, T-1), c] + s * eps[b, j, c]  for c < D,  0 for D <= c < ld_out
//   src(b) = slot[b] (or b);  eps = philox_init_kernel's draw: stream LDP_PHILOX_STREAM_INIT, step 0, element (row0 + b * T + j) * DP + c.
// x_prev rows are (T, D) unpadded; dst rows have stride ld_out (DP: the padded loop state; D: caller memory).  A thread owns the four
// channels c0 .. c0 + 3 of one (b, j): with VIN the 16-byte load of x_prev (D % 4 == 0), with VOUT the 16-byte store (ld_out % 4 == 0).
// The sum is spelled with explicit roundings -- fma(a, xs, rn(s * eps)) -- so it does not depend on the contraction setting.
template <bool VIN, bool VOUT>
__global__ __launch_bounds__(256) void plan_warm_init_kernel(const float* __restrict__ x_prev, const int32_t* __restrict__ slot,
                                                             float* __restrict__ dst, int ld_out, int B, int T, int D, int DP, int shift,
                                                             float a, float s, uint64_t seed, uint64_t row0) {
  const int gpr = (ld_out + 3) / 4;                          // channel groups per row
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * T * gpr) return;
  const int64_t r = i / gpr;                                 // local row b * T + j
  const int c0 = (int)(i - r * gpr) * 4;
  const int b = (int)(r / T), j = (int)(r - (int64_t)b * T);
  const int jj = min(j + min(shift, T), T - 1);              // edge hold (shift >= T: the last state everywhere)
  const int64_t sb = slot ? (int64_t)slot[b] : (int64_t)b;
  const float* src = x_prev + ((size_t)sb * T + jj) * D;
  float xs[4] = {0.f, 0.f, 0.f, 0.f};
  if (VIN && c0 + 3 < D) {
    const float4 v = *reinterpret_cast<const float4*>(src + c0);
    xs[0] = v.x; xs[1] = v.y; xs[2] = v.z; xs[3] = v.w;
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (c0 + q < D) xs[q] = src[c0 + q];
  }
  float o[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = c0 + q;
    float v = 0.0f;
    if (c < D) {
      const float eps = philox_normal(seed, (row0 + (uint64_t)r) * (uint64_t)DP + (uint64_t)c, 0u, LDP_PHILOX_STREAM_INIT);
      v = __fmaf_rn(a, xs[q], __fmul_rn(s, eps));
    }
    o[q] = v;
  }
  float* out = dst + (size_t)r * ld_out + c0;
  if (VOUT) {
    *reinterpret_cast<float4*>(out) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (c0 + q < ld_out) out[q] = o[q];
  }
}

// dst[(slot[b] or b), j, c] = src[b, j, c] for c < D: rows of the padded loop state (stride DP) into rows of the unpadded slot table
__global__ void unpad_rows_index_kernel(const float* __restrict__ src, float* __restrict__ dst, const int32_t* __restrict__ slot, int B, int T,
                                        int D, int DP) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * T * D) return;
  const int64_t r = i / D;
  const int c = (int)(i - r * D);
  const int b = (int)(r / T), j = (int)(r - (int64_t)b * T);
  const int64_t sb = slot ? (int64_t)slot[b] : (int64_t)b;
  dst[((size_t)sb * T + j) * D + c] = src[(size_t)r * DP + c];
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

int warm_coefs(int n_train, int n_steps, int step_begin, float* a, float* s) {
  if (n_steps <= 0 || n_train % n_steps != 0) return fail(LDP_EINVAL, "n_steps %d must divide the %d training steps", n_steps, n_train);
  if (step_begin < 0 || step_begin >= n_steps) return fail(LDP_EINVAL, "step_begin %d outside 0..n_steps-1 = %d", step_begin, n_steps - 1);
  std::vector<float> betas, alphas, acp;
  betas_squaredcos(n_train, betas, alphas, acp);
  const int t = (n_steps - 1 - step_begin) * (n_train / n_steps);
  const double a_t = acp[t];                      // float32 table, float64 from here (make_step_coefs' convention)
  *a = (float)std::sqrt(a_t);
  *s = (float)std::sqrt(1.0 - a_t);
  return LDP_OK;
}

static bool slots_on_device(const int32_t* slot) {
  hipPointerAttribute_t at{};
  const hipError_t e = hipPointerGetAttributes(&at, slot);
  if (e != hipSuccess) (void)hipGetLastError();    // (older runtimes report plain host memory as an error: it is host memory)
  return e == hipSuccess && (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged);
}

int check_host_slots(const int32_t* slot, int n_slots, int B) {
  if (!slot || slots_on_device(slot)) return LDP_OK;      // device-side slot values are not checked
  for (int b = 0; b < B; ++b)
    if (slot[b] < 0 || slot[b] >= n_slots) return fail(LDP_EINVAL, "slot[%d] = %d outside 0..n_slots-1 = %d", b, slot[b], n_slots - 1);
  return LDP_OK;
}

int stage_slots(ldp_handle* h, const int32_t* slot, int n_slots, int B, hipStream_t s, const int32_t** dev_out) {
  *dev_out = nullptr;
  if (!slot) return LDP_OK;
  if (slots_on_device(slot)) {
    *dev_out = slot;
    return LDP_OK;
  }
  LDP_TRY(check_host_slots(slot, n_slots, B));
  LDP_TRY(h->slot_buf.alloc((size_t)std::max(B, 4096) * 4));
  // (pageable host memory: the runtime has read the table when the call returns)
  LDP_HIP(hipMemcpyAsync(h->slot_buf.p, slot, (size_t)B * 4, hipMemcpyHostToDevice, s));
  *dev_out = h->slot_buf.as<int32_t>();
  return LDP_OK;
}

int plan_warm_init_launch(const float* x_prev, const int32_t* slot_dev, float* dst, int ld_out, int B, int T, int D, int DP, int shift,
                          float a, float s, uint64_t seed, uint64_t row0, hipStream_t st) {
  const int64_t n = (int64_t)B * T * ((ld_out + 3) / 4);
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  const bool vin = D % 4 == 0 && aligned16(x_prev), vout = ld_out % 4 == 0 && aligned16(dst);
#define LDP_WARM(VI, VO) \
  hipLaunchKernelGGL((plan_warm_init_kernel<VI, VO>), grid, block, 0, st, x_prev, slot_dev, dst, ld_out, B, T, D, DP, shift, a, s, seed, row0)
  if (vin && vout) LDP_WARM(true, true);
  else if (vin) LDP_WARM(true, false);
  else if (vout) LDP_WARM(false, true);
  else LDP_WARM(false, false);
#undef LDP_WARM
  LDP_HIP(hipGetLastError());
  return LDP_OK;
}

int unpad_rows_index_launch(const float* src, float* dst, const int32_t* slot_dev, int B, int T, int D, int DP, hipStream_t st) {
  const int64_t n = (int64_t)B * T * D;
  hipLaunchKernelGGL(unpad_rows_index_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, dst, slot_dev, B, T, D, DP);
  LDP_HIP(hipGetLastError());
  return LDP_OK;
}

}  // namespace ldp

using namespace ldp;

extern "C" {

int ldp_plan_warm_init(ldp_handle* h, const float* x_prev, const int32_t* slot, int32_t n_slots, int32_t shift, uint64_t seed,
                       int64_t row_offset, int32_t sampler, int32_t n_steps, int32_t step_begin, float* x_out, int32_t B, void* stream) {
  if (!h || !x_prev || !x_out) return fail(LDP_EINVAL, "bad argument");
  if (B < 1) return fail(LDP_EINVAL, "B must be >= 1, got %d", B);
  if (!h->pl.ready) return fail(LDP_ESTATE, "planner weights not finalized");
  PlannerState& P = h->pl;
  if (n_slots < 1) return fail(LDP_EINVAL, "n_slots must be >= 1, got %d", n_slots);
  if (shift < 0) return fail(LDP_EINVAL, "shift must be >= 0, got %d", shift);
  if (!slot && B > n_slots) return fail(LDP_EINVAL, "slot is NULL and B = %d exceeds n_slots = %d", B, n_slots);
  LDP_TRY(check_sampler(sampler, n_steps, P.n_train, "planner"));
  float a = 0.f, s = 0.f;
  LDP_TRY(warm_coefs(P.n_train, n_steps, step_begin, &a, &s));
  hipStream_t st = (hipStream_t)stream;
  const int32_t* slot_dev = nullptr;
  LDP_TRY(stage_slots(h, slot, n_slots, B, st, &slot_dev));
  return plan_warm_init_launch(x_prev, slot_dev, x_out, P.D, B, P.T, P.D, P.DP, shift, a, s, seed, (uint64_t)(row_offset * P.T), st);
}

}  // extern "C"
