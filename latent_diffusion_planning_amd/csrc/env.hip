// env.hip -- the device-resident reach task (include/ldp_env.h), built into a library of its own (libldp_env.so): the state, the
// dynamics, the observation and the scripted policies of `reach2d` for N environments in lockstep, one thread per environment.  Stateless like data.hip:
// no handle, no atomics, plain stores only -- the outputs are a function of the arguments alone.  Exact fp32 on the VALU, every operation
// rounded once and spelled (__fmaf_rn, __fmul_rn, ...) so that nothing is contracted or reassociated; no transcendental function.
// tests/toyenv_oracle.py restates every line in NumPy float32 and the kernels reproduce it bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>

#include "../../include/ldp_env.h"
#include "tconv.hpp"      // philox4x32_10

namespace ldp {
namespace {

// the library's own error plumbing (libldp_hip.so's lives in kernels_misc.hip and is not linked here)
std::string& env_last_error() {
  static thread_local std::string e;
  return e;
}

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  env_last_error() = buf;
  return code;
}

#define ENV_HIP(expr)                                                                                                       \
  do {                                                                                                                      \
    hipError_t _e = (expr);                                                                                                 \
    if (_e != hipSuccess) return fail(LDP_ENV_EHIP, "%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
  } while (0)
#define ENV_TRY(expr)                  \
  do {                                 \
    int _r = (expr);                   \
    if (_r != LDP_ENV_OK) return _r;   \
  } while (0)

constexpr int ET = 256;                           // threads per work-group
constexpr unsigned ENV_MAX_BLOCKS = 2048;         // the rest is strided
constexpr float ENV_R = 0.3f, ENV_DT = 0.08f, ENV_TOL = 0.08f, ENV_WY = 0.65f, ENV_INV_DT = 12.5f;

struct EnvState { float px, py, gx, gy, side, t, first, blocked; };

// the observation buffers of one call: frame j of environment i at row i * frames + j
struct EnvObs { float* pos; float* goal; float* latent; };

__device__ __forceinline__ float uniform24(uint32_t w) { return __fmul_rn((float)(w >> 8), 1.0f / 16777216.0f); }      // exact
__device__ __forceinline__ float clamp1(float v) { return fminf(fmaxf(v, -1.0f), 1.0f); }

__device__ __forceinline__ EnvState load_state(const float* __restrict__ state, size_t i) {
  const float4 a = *reinterpret_cast<const float4*>(state + i * LDP_ENV_STATE), b = *reinterpret_cast<const float4*>(state + i * LDP_ENV_STATE + 4);
  return EnvState{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
}

__device__ __forceinline__ void store_state(float* __restrict__ state, size_t i, const EnvState& s) {
  *reinterpret_cast<float4*>(state + i * LDP_ENV_STATE) = make_float4(s.px, s.py, s.gx, s.gy);
  *reinterpret_cast<float4*>(state + i * LDP_ENV_STATE + 4) = make_float4(s.side, s.t, s.first, s.blocked);
}

// T1..T4 of u: T2 = fma(2u, u, -1), T3 = fma(2u, T2, -u), T4 = fma(2u, T3, -T2)
__device__ __forceinline__ void chebyshev4(float u, float* __restrict__ out) {
  const float u2 = __fadd_rn(u, u);
  const float t2 = __fmaf_rn(u2, u, -1.0f);
  const float t3 = __fmaf_rn(u2, t2, -u);
  out[0] = u; out[1] = t2; out[2] = t3; out[3] = __fmaf_rn(u2, t3, -t2);
}

__device__ __forceinline__ void write_obs(const EnvState& s, const EnvObs& O, size_t row) {
  if (O.pos) { O.pos[row * 2] = s.px; O.pos[row * 2 + 1] = s.py; }
  if (O.goal) { O.goal[row * 2] = s.gx; O.goal[row * 2 + 1] = s.gy; }
  if (O.latent) {
    float* l = O.latent + row * LDP_ENV_LATENT;
    chebyshev4(s.px, l);
    chebyshev4(s.py, l + 4);
    chebyshev4(__fmul_rn(__fsub_rn(s.gx, s.px), 0.5f), l + 8);
    chebyshev4(__fmul_rn(__fsub_rn(s.gy, s.py), 0.5f), l + 12);
  }
}

// the action of a scripted policy at the state's own time t: the draws of step 1 + t
__device__ __forceinline__ void scripted(const EnvState& s, int policy, float noise, uint64_t seed, uint64_t episode, float& ax, float& ay) {
  uint32_t w[4];
  philox4x32_10(seed, episode, 1u + (uint32_t)s.t, LDP_PHILOX_STREAM_ENV, w);
  const float rx = __fmaf_rn(2.0f, uniform24(w[0]), -1.0f), ry = __fmaf_rn(2.0f, uniform24(w[1]), -1.0f);
  if (policy == LDP_ENV_POLICY_RANDOM) { ax = rx; ay = ry; return; }
  const bool detour = policy == LDP_ENV_POLICY_EXPERT && s.px < 0.0f;
  const float tx = detour ? 0.0f : s.gx, ty = detour ? __fmul_rn(s.side, ENV_WY) : s.gy;
  const float dx = __fmul_rn(__fsub_rn(tx, s.px), ENV_INV_DT), dy = __fmul_rn(__fsub_rn(ty, s.py), ENV_INV_DT);
  const float m = fmaxf(fmaxf(fabsf(dx), fabsf(dy)), 1.0f);
  ax = clamp1(__fmaf_rn(noise, rx, __fdiv_rn(dx, m)));
  ay = clamp1(__fmaf_rn(noise, ry, __fdiv_rn(dy, m)));
}

__device__ __forceinline__ void advance(EnvState& s, float ax, float ay) {
  const float qx = clamp1(__fmaf_rn(ENV_DT, ax, s.px)), qy = clamp1(__fmaf_rn(ENV_DT, ay, s.py));
  if (__fmaf_rn(qx, qx, __fmul_rn(qy, qy)) < __fmul_rn(ENV_R, ENV_R)) {
    s.blocked = __fadd_rn(s.blocked, 1.0f);
  } else {
    s.px = qx; s.py = qy;
  }
  s.t = __fadd_rn(s.t, 1.0f);
  const float dx = __fsub_rn(s.px, s.gx), dy = __fsub_rn(s.py, s.gy);
  if (s.first == 0.0f && __fmaf_rn(dx, dx, __fmul_rn(dy, dy)) <= __fmul_rn(ENV_TOL, ENV_TOL)) s.first = s.t;
}

__global__ __launch_bounds__(ET) void env_reset_kernel(float* __restrict__ state, int N, uint64_t seed, uint64_t episode0) {
  for (size_t i = (size_t)blockIdx.x * ET + threadIdx.x; i < (size_t)N; i += (size_t)gridDim.x * ET) {
    uint32_t w[4];
    philox4x32_10(seed, episode0 + i, 0u, LDP_PHILOX_STREAM_ENV, w);
    store_state(state, i, EnvState{-0.8f, __fadd_rn(-0.5f, uniform24(w[0])), 0.8f, __fadd_rn(-0.5f, uniform24(w[1])),
                                   (w[2] & 1u) ? 1.0f : -1.0f, 0.0f, 0.0f, 0.0f});
  }
}

__global__ __launch_bounds__(ET) void env_observe_kernel(const float* __restrict__ state, int N, const EnvObs O) {
  for (size_t i = (size_t)blockIdx.x * ET + threadIdx.x; i < (size_t)N; i += (size_t)gridDim.x * ET) write_obs(load_state(state, i), O, i);
}

// n_sub sub-steps of every environment: the state stays in registers between them
__global__ __launch_bounds__(ET) void env_step_kernel(float* __restrict__ state, int N, int n_sub, const float* __restrict__ actions, int A,
                                                      int policy, float noise, uint64_t seed, uint64_t episode0, float* __restrict__ actions_out,
                                                      const EnvObs O) {
  for (size_t i = (size_t)blockIdx.x * ET + threadIdx.x; i < (size_t)N; i += (size_t)gridDim.x * ET) {
    EnvState s = load_state(state, i);
    for (int j = 0; j < n_sub; ++j) {
      const size_t row = i * (size_t)n_sub + j;
      write_obs(s, O, row);
      float ax, ay;
      if (policy == LDP_ENV_POLICY_GIVEN) {
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

unsigned env_blocks(int N) { return std::min((unsigned)((N + ET - 1) / ET), ENV_MAX_BLOCKS); }

int check_state(const float* state, int32_t N) {
  if (!state) return fail(LDP_ENV_EINVAL, "null state");
  if (N < 1) return fail(LDP_ENV_EINVAL, "N must be >= 1, got %d", N);
  if ((uintptr_t)state % 16) return fail(LDP_ENV_EINVAL, "state must be 16-byte aligned");
  return LDP_ENV_OK;
}

}  // namespace
}  // namespace ldp

using namespace ldp;

extern "C" {

const char* ldp_env_last_error(void) { return env_last_error().c_str(); }

int ldp_env_reset(float* state, int32_t N, uint64_t seed, int64_t episode0, void* stream) {
  ENV_TRY(check_state(state, N));
  if (episode0 < 0) return fail(LDP_ENV_EINVAL, "episode0 must be >= 0, got %lld", (long long)episode0);
  hipLaunchKernelGGL(env_reset_kernel, dim3(env_blocks(N)), dim3(ET), 0, (hipStream_t)stream, state, N, seed, (uint64_t)episode0);
  ENV_HIP(hipGetLastError());
  return LDP_ENV_OK;
}

int ldp_env_observe(const float* state, int32_t N, float* pos, float* goal, float* latent, void* stream) {
  ENV_TRY(check_state(state, N));
  if (!pos && !goal && !latent) return fail(LDP_ENV_EINVAL, "no output: pos, goal and latent are all null");
  hipLaunchKernelGGL(env_observe_kernel, dim3(env_blocks(N)), dim3(ET), 0, (hipStream_t)stream, state, N, EnvObs{pos, goal, latent});
  ENV_HIP(hipGetLastError());
  return LDP_ENV_OK;
}

int ldp_env_step(float* state, int32_t N, int32_t n_sub, const float* actions, int32_t A, int32_t policy, float noise, uint64_t seed,
                 int64_t episode0, float* actions_out, float* pos_out, float* goal_out, float* latent_out, void* stream) {
  ENV_TRY(check_state(state, N));
  if (n_sub < 1) return fail(LDP_ENV_EINVAL, "n_sub must be >= 1, got %d", n_sub);
  if (A < 2) return fail(LDP_ENV_EINVAL, "A must be >= 2 (the task reads two action components), got %d", A);
  if (policy < LDP_ENV_POLICY_GIVEN || policy > LDP_ENV_POLICY_RANDOM)
    return fail(LDP_ENV_EINVAL, "unknown policy %d (0 given actions, 1 expert, 2 straight, 3 random)", policy);
  if (!std::isfinite(noise)) return fail(LDP_ENV_EINVAL, "noise must be finite");
  if (episode0 < 0) return fail(LDP_ENV_EINVAL, "episode0 must be >= 0, got %lld", (long long)episode0);
  if ((policy == LDP_ENV_POLICY_GIVEN) != (actions != nullptr))
    return fail(LDP_ENV_EINVAL, "actions go with policy 0 (given actions) and with no other: policy %d, actions %s", policy, actions ? "given" : "null");
  hipLaunchKernelGGL(env_step_kernel, dim3(env_blocks(N)), dim3(ET), 0, (hipStream_t)stream, state, N, n_sub, actions, A, policy, noise, seed,
                     (uint64_t)episode0, actions_out, EnvObs{pos_out, goal_out, latent_out});
  ENV_HIP(hipGetLastError());
  return LDP_ENV_OK;
}

}  // extern "C"
