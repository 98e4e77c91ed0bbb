// push.hip -- the device-resident pushing task (include/ldp_push.h), built into a library of its own (libldp_push.so): the state, the
// contact dynamics, the observation and the scripted policies of `push2d` for N environments in lockstep, one thread per environment.  Stateless like
// env.hip: no handle, no atomics, plain stores only -- the outputs are a function of the arguments alone.  Exact fp32 on the VALU, every operation
// rounded once and spelled (__fmaf_rn, __fmul_rn, ...) so that nothing is contracted or reassociated; no transcendental function.  The square root
// is the float result of a double-precision sqrt of the float argument (correctly rounded: 53 >= 2 * 24 + 2 bits), because __fsqrt_rn is the
// hardware's approximate v_sqrt_f32 in this toolchain; the divides are __fdiv_rn, correctly rounded as in env.hip.
// tests/pushenv_oracle.py restates every line in NumPy float32 and the kernels reproduce it bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>

#include "../../include/ldp_push.h"
#include "tconv.hpp"      // philox4x32_10

namespace ldp {
namespace {

// the library's own error plumbing (libldp_hip.so's lives in kernels_misc.hip and is not linked here)
std::string& push_last_error() {
  static thread_local std::string e;
  return e;
}

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  push_last_error() = buf;
  return code;
}

#define PUSH_HIP(expr)                                                                                                       \
  do {                                                                                                                       \
    hipError_t _e = (expr);                                                                                                  \
    if (_e != hipSuccess) return fail(LDP_PUSH_EHIP, "%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
  } while (0)
#define PUSH_TRY(expr)                  \
  do {                                  \
    int _r = (expr);                    \
    if (_r != LDP_PUSH_OK) return _r;   \
  } while (0)

constexpr int PT = 256;                            // threads per work-group
constexpr unsigned PUSH_MAX_BLOCKS = 2048;         // the rest is strided
constexpr float PUSH_C = 0.2f, PUSH_DT = 0.08f, PUSH_TOL = 0.1f, PUSH_LIM = 0.85f, PUSH_INV_DT = 12.5f;

struct PushState { float px, py, ox, oy, gx, gy, side, t, first, blocked, pushed; };

// the observation buffers of one call: frame j of environment i at row i * frames + j
struct PushObs { float* pos; float* goal; float* latent; };

__device__ __forceinline__ float uniform24(uint32_t w) { return __fmul_rn((float)(w >> 8), 1.0f / 16777216.0f); }      // exact
__device__ __forceinline__ float clamp1(float v) { return fminf(fmaxf(v, -1.0f), 1.0f); }
__device__ __forceinline__ float sqrt_rn(float v) { return (float)sqrt((double)v); }                                   // correctly rounded
__device__ __forceinline__ float dot2(float ax, float ay, float bx, float by) { return __fmaf_rn(ax, bx, __fmul_rn(ay, by)); }

__device__ __forceinline__ PushState load_state(const float* __restrict__ state, size_t i) {
  const float4* p = reinterpret_cast<const float4*>(state + i * LDP_PUSH_STATE);
  const float4 a = p[0], b = p[1], c = p[2];
  return PushState{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z};
}

__device__ __forceinline__ void store_state(float* __restrict__ state, size_t i, const PushState& s) {
  float4* p = reinterpret_cast<float4*>(state + i * LDP_PUSH_STATE);
  p[0] = make_float4(s.px, s.py, s.ox, s.oy);
  p[1] = make_float4(s.gx, s.gy, s.side, s.t);
  p[2] = make_float4(s.first, s.blocked, s.pushed, 0.0f);
}

// (T1, T2) of x: T2 = fma(2x, x, -1)
__device__ __forceinline__ void chebyshev2(float x, float* __restrict__ out) {
  out[0] = x; out[1] = __fmaf_rn(__fadd_rn(x, x), x, -1.0f);
}

__device__ __forceinline__ float half_diff(float a, float b) { return __fmul_rn(__fsub_rn(a, b), 0.5f); }

__device__ __forceinline__ void write_obs(const PushState& s, const PushObs& O, size_t row) {
  if (O.pos) { O.pos[row * 2] = s.px; O.pos[row * 2 + 1] = s.py; }
  if (O.goal) { O.goal[row * 2] = s.gx; O.goal[row * 2 + 1] = s.gy; }
  if (O.latent) {
    float* l = O.latent + row * LDP_PUSH_LATENT;
    chebyshev2(s.px, l);
    chebyshev2(s.py, l + 2);
    chebyshev2(s.ox, l + 4);
    chebyshev2(s.oy, l + 6);
    chebyshev2(half_diff(s.gx, s.ox), l + 8);
    chebyshev2(half_diff(s.gy, s.oy), l + 10);
    chebyshev2(half_diff(s.ox, s.px), l + 12);
    chebyshev2(half_diff(s.oy, s.py), l + 14);
  }
}

// the expert's target: behind the disc (as seen from the goal) it pushes; beside or ahead of the disc it goes round on the side it is on
__device__ __forceinline__ void expert_target(const PushState& s, float& tx, float& ty) {
  const float vx = __fsub_rn(s.gx, s.ox), vy = __fsub_rn(s.gy, s.oy);
  const float L = fmaxf(sqrt_rn(dot2(vx, vy, vx, vy)), 1e-6f);
  const float ux = __fdiv_rn(vx, L), uy = __fdiv_rn(vy, L);
  const float nx = -uy, ny = ux;
  const float rx = __fsub_rn(s.px, s.ox), ry = __fsub_rn(s.py, s.oy);
  const float along = dot2(rx, ry, ux, uy), lat = dot2(rx, ry, nx, ny);
  const float sg = fabsf(lat) > 0.05f ? (lat > 0.0f ? 1.0f : -1.0f) : s.side;
  const float ax = __fmaf_rn(-0.3f, ux, s.ox), ay = __fmaf_rn(-0.3f, uy, s.oy);
  const float w = __fmul_rn(0.39f, sg);
  if (along < -0.1f && fabsf(lat) < __fmul_rn(0.6f, fabsf(along))) {
    tx = __fmaf_rn(-0.1f, ux, s.ox); ty = __fmaf_rn(-0.1f, uy, s.oy);
  } else if (along > -0.25f) {
    if (fabsf(lat) < 0.3f) {
      const float c = clamp1(along);
      tx = __fmaf_rn(w, nx, __fmaf_rn(c, ux, s.ox)); ty = __fmaf_rn(w, ny, __fmaf_rn(c, uy, s.oy));
    } else {
      tx = __fmaf_rn(w, nx, ax); ty = __fmaf_rn(w, ny, ay);
    }
  } else {
    tx = ax; ty = ay;
  }
}

// the action of a scripted policy at the state's own time t: the draws of step 1 + t
__device__ __forceinline__ void scripted(const PushState& s, int policy, float noise, uint64_t seed, uint64_t episode, float& ax, float& ay) {
  uint32_t w[4];
  philox4x32_10(seed, episode, 1u + (uint32_t)s.t, LDP_PHILOX_STREAM_PUSH, w);
  const float rx = __fmaf_rn(2.0f, uniform24(w[0]), -1.0f), ry = __fmaf_rn(2.0f, uniform24(w[1]), -1.0f);
  if (policy == LDP_PUSH_POLICY_RANDOM) { ax = rx; ay = ry; return; }
  float tx = s.ox, ty = s.oy;
  if (policy == LDP_PUSH_POLICY_EXPERT) expert_target(s, tx, ty);
  const float dx = __fmul_rn(__fsub_rn(tx, s.px), PUSH_INV_DT), dy = __fmul_rn(__fsub_rn(ty, s.py), PUSH_INV_DT);
  const float m = fmaxf(fmaxf(fabsf(dx), fabsf(dy)), 1.0f);
  ax = clamp1(__fmaf_rn(noise, rx, __fdiv_rn(dx, m)));
  ay = clamp1(__fmaf_rn(noise, ry, __fdiv_rn(dy, m)));
}

__device__ __forceinline__ void advance(PushState& s, float ax, float ay) {
  const float qx = clamp1(__fmaf_rn(PUSH_DT, ax, s.px)), qy = clamp1(__fmaf_rn(PUSH_DT, ay, s.py));
  const float dx = __fsub_rn(s.ox, qx), dy = __fsub_rn(s.oy, qy);
  const float d2 = dot2(dx, dy, dx, dy);
  if (d2 < __fmul_rn(PUSH_C, PUSH_C)) {
    const float dist = sqrt_rn(d2);
    const bool apart = dist > 0.0f;
    const float nx = apart ? __fdiv_rn(dx, dist) : 1.0f, ny = apart ? __fdiv_rn(dy, dist) : 0.0f;
    const float ox = __fmaf_rn(PUSH_C, nx, qx), oy = __fmaf_rn(PUSH_C, ny, qy);
    if (fabsf(ox) > PUSH_LIM || fabsf(oy) > PUSH_LIM) {
      s.blocked = __fadd_rn(s.blocked, 1.0f);
    } else {
      s.px = qx; s.py = qy; s.ox = ox; s.oy = oy;
      s.pushed = __fadd_rn(s.pushed, 1.0f);
    }
  } else {
    s.px = qx; s.py = qy;
  }
  s.t = __fadd_rn(s.t, 1.0f);
  const float ex = __fsub_rn(s.ox, s.gx), ey = __fsub_rn(s.oy, s.gy);
  if (s.first == 0.0f && dot2(ex, ey, ex, ey) <= __fmul_rn(PUSH_TOL, PUSH_TOL)) s.first = s.t;
}

__global__ __launch_bounds__(PT) void push_reset_kernel(float* __restrict__ state, int N, uint64_t seed, uint64_t episode0) {
  for (size_t i = (size_t)blockIdx.x * PT + threadIdx.x; i < (size_t)N; i += (size_t)gridDim.x * PT) {
    uint32_t w[4];
    philox4x32_10(seed, episode0 + i, 0u, LDP_PHILOX_STREAM_PUSH, w);
    store_state(state, i, PushState{-0.8f, __fadd_rn(-0.5f, uniform24(w[0])),
                                    __fmaf_rn(0.6f, uniform24(w[1]), -0.3f), __fmaf_rn(0.8f, uniform24(w[2]), -0.4f),
                                    (w[0] & 1u) ? -0.6f : 0.6f, __fadd_rn(-0.5f, uniform24(w[3])),
                                    (w[1] & 1u) ? 1.0f : -1.0f, 0.0f, 0.0f, 0.0f, 0.0f});
  }
}

__global__ __launch_bounds__(PT) void push_observe_kernel(const float* __restrict__ state, int N, const PushObs O) {
  for (size_t i = (size_t)blockIdx.x * PT + threadIdx.x; i < (size_t)N; i += (size_t)gridDim.x * PT) write_obs(load_state(state, i), O, i);
}

// n_sub sub-steps of every environment: the state stays in registers between them
__global__ __launch_bounds__(PT) void push_step_kernel(float* __restrict__ state, int N, int n_sub, const float* __restrict__ actions, int A,
                                                       int policy, float noise, uint64_t seed, uint64_t episode0, float* __restrict__ actions_out,
                                                       const PushObs O) {
  for (size_t i = (size_t)blockIdx.x * PT + threadIdx.x; i < (size_t)N; i += (size_t)gridDim.x * PT) {
    PushState s = load_state(state, i);
    for (int j = 0; j < n_sub; ++j) {
      const size_t row = i * (size_t)n_sub + j;
      write_obs(s, O, row);
      float ax, ay;
      if (policy == LDP_PUSH_POLICY_GIVEN) {
        ax = actions[row * A]; ay = actions[row * A + 1];
        ax = clamp1(ax == ax ? ax : 0.0f); ay = clamp1(ay == ay ? ay : 0.0f);
      } else {
        scripted(s, policy, noise, seed, episode0 + i, ax, ay);
      }
      if (actions_out) {
        actions_out[row * A] = ax; actions_out[row * A + 1] = ay;
        for (int c = 2; c < A; ++c) actions_out[row * A + c] = 0.0f;
      }
      advance(s, ax, ay);
    }
    store_state(state, i, s);
  }
}

unsigned push_blocks(int N) { return std::min((unsigned)(((size_t)N + PT - 1) / PT), PUSH_MAX_BLOCKS); }

int check_state(const float* state, int32_t N) {
  if (!state) return fail(LDP_PUSH_EINVAL, "null state");
  if (N < 1) return fail(LDP_PUSH_EINVAL, "N must be >= 1, got %d", N);
  if ((uintptr_t)state % 16) return fail(LDP_PUSH_EINVAL, "state must be 16-byte aligned");
  return LDP_PUSH_OK;
}

}  // namespace
}  // namespace ldp

using namespace ldp;

extern "C" {

const char* ldp_push_last_error(void) { return push_last_error().c_str(); }

int ldp_push_reset(float* state, int32_t N, uint64_t seed, int64_t episode0, void* stream) {
  PUSH_TRY(check_state(state, N));
  if (episode0 < 0) return fail(LDP_PUSH_EINVAL, "episode0 must be >= 0, got %lld", (long long)episode0);
  hipLaunchKernelGGL(push_reset_kernel, dim3(push_blocks(N)), dim3(PT), 0, (hipStream_t)stream, state, N, seed, (uint64_t)episode0);
  PUSH_HIP(hipGetLastError());
  return LDP_PUSH_OK;
}

int ldp_push_observe(const float* state, int32_t N, float* pos, float* goal, float* latent, void* stream) {
  PUSH_TRY(check_state(state, N));
  if (!pos && !goal && !latent) return fail(LDP_PUSH_EINVAL, "no output: pos, goal and latent are all null");
  hipLaunchKernelGGL(push_observe_kernel, dim3(push_blocks(N)), dim3(PT), 0, (hipStream_t)stream, state, N, PushObs{pos, goal, latent});
  PUSH_HIP(hipGetLastError());
  return LDP_PUSH_OK;
}

int ldp_push_step(float* state, int32_t N, int32_t n_sub, const float* actions, int32_t A, int32_t policy, float noise, uint64_t seed,
                  int64_t episode0, float* actions_out, float* pos_out, float* goal_out, float* latent_out, void* stream) {
  PUSH_TRY(check_state(state, N));
  if (n_sub < 1) return fail(LDP_PUSH_EINVAL, "n_sub must be >= 1, got %d", n_sub);
  if (A < 2) return fail(LDP_PUSH_EINVAL, "A must be >= 2 (the task reads two action components), got %d", A);
  if (policy < LDP_PUSH_POLICY_GIVEN || policy > LDP_PUSH_POLICY_RANDOM)
    return fail(LDP_PUSH_EINVAL, "unknown policy %d (0 given actions, 1 expert, 2 straight, 3 random)", policy);
  if (!std::isfinite(noise)) return fail(LDP_PUSH_EINVAL, "noise must be finite");
  if (episode0 < 0) return fail(LDP_PUSH_EINVAL, "episode0 must be >= 0, got %lld", (long long)episode0);
  if ((policy == LDP_PUSH_POLICY_GIVEN) != (actions != nullptr))
    return fail(LDP_PUSH_EINVAL, "actions go with policy 0 (given actions) and with no other: policy %d, actions %s", policy, actions ? "given" : "null");
  hipLaunchKernelGGL(push_step_kernel, dim3(push_blocks(N)), dim3(PT), 0, (hipStream_t)stream, state, N, n_sub, actions, A, policy, noise, seed,
                     (uint64_t)episode0, actions_out, PushObs{pos_out, goal_out, latent_out});
  PUSH_HIP(hipGetLastError());
  return LDP_PUSH_OK;
}

}  // extern "C"
