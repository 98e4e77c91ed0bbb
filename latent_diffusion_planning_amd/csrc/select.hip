// select.hip -- best-of-N planning (include/ldp_hip.h "best-of-N planning"): the candidate loop's tiled condition, the two
// built-in costs and the per-observation argmin + gather.  Exact fp32 on the VALU (statistics in float64), no atomics, every sum in a
// fixed order.  Rows are candidate-major: candidate c of observation b is row c * B + b.
#include <cmath>

#include "engine.hpp"

namespace ldp {
namespace {

// cond[r][e] = obs_emb[r mod B][e], e < G = obs_horizon * D (the first obs_horizon frames of an observation are contiguous)
__global__ void tile_cond_kernel(const float* __restrict__ obs_emb, float* __restrict__ cond, int B, int H, int D, int G, int64_t rows) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * G) return;
  const int64_t r = i / G;
  const int e = (int)(i - r * G);
  cond[i] = obs_emb[(size_t)(r % B) * H * D + e];
}

// ---- density cost -------------------------------------------------------------------------------------------------------------------
// m_b = 2 sum_k Var_k over the N candidates of observation b, float64, two passes (centred); one work-group of 1024 per observation:
// 64 threads over k x 16 groups over the candidates (group g owns c = g, g + 16, ...), partial sums combined in the order g = 0 .. 15,
// then one tree over the work-group.  -> inv2h2[b] = 1 / (2 bandwidth^2 m_b) as float32 (0 when m_b = 0: every exp is exp(-0) = 1).
constexpr int ST_K = 64, ST_G = 16;
__global__ __launch_bounds__(ST_K* ST_G) void density_stats_kernel(const float* __restrict__ x, int B, int N, int K, double bw2,
                                                                  float* __restrict__ inv2h2) {
  __shared__ double part[ST_G][ST_K];
  __shared__ double red[ST_K * ST_G];
  const int b = blockIdx.x, kx = threadIdx.x % ST_K, g = threadIdx.x / ST_K;
  double acc = 0.0;
  for (int k0 = 0; k0 < K; k0 += ST_K) {
    const int k = k0 + kx;
    double s = 0.0;
    if (k < K)
      for (int c = g; c < N; c += ST_G) s += (double)x[((size_t)c * B + b) * K + k];
    part[g][kx] = s;
    __syncthreads();
    double mean = 0.0;
    for (int q = 0; q < ST_G; ++q) mean += part[q][kx];
    mean /= (double)N;
    __syncthreads();
    if (k < K)
      for (int c = g; c < N; c += ST_G) {
        const double d = (double)x[((size_t)c * B + b) * K + k] - mean;
        acc += d * d;
      }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int w = ST_K * ST_G / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double m = 2.0 * red[0] / (double)N;
    inv2h2[b] = m > 0.0 ? (float)(1.0 / (2.0 * bw2 * m)) : 0.0f;
  }
}

// One work-group = 16 rows i of one observation against all N candidates j, in tiles of 64 j (16 rows: 64 work-groups already at 1024
// candidates of one observation).  The row tiles are staged in LDS in chunks of 32 k (rows padded to 33 words: lane l reads bank
// (l + k) % 32); thread (ti, tj) owns the 4 pairs (ti, tj + 16 q) and carries each d2 as ONE fp32 FMA chain over k = 0 .. K-1.  The tile's
// exp values go through LDS to the row's owner (thread i), which adds them in the order j = 0 .. 63 to its running sum: the sum over j is
// strictly sequential in the global order 0 .. N-1, and the tiling depends on nothing but N.
constexpr int DTI = 16, DTJ = 64, DKC = 32;
__global__ __launch_bounds__(256) void density_cost_kernel(const float* __restrict__ x, int B, int N, int K, int c0, int n_loc,
                                                           const float* __restrict__ inv2h2, float* __restrict__ cost) {
  __shared__ float xi[DTI][DKC + 1], xj[DTJ][DKC + 1], ev[DTI][DTJ + 1];
  const int b = blockIdx.y, i0 = blockIdx.x * DTI;         // local row tile: candidates c0 + i0 ...
  const int tid = threadIdx.x, ti = tid / 16, tj = tid % 16;
  const float s = inv2h2[b];
  float total = 0.0f;                                      // threads 0 .. 15: the running sum of row i0 + tid
  for (int j0 = 0; j0 < N; j0 += DTJ) {
    float d2[4] = {};
    for (int k0 = 0; k0 < K; k0 += DKC) {
      __syncthreads();                                     // the previous chunk (and the previous tile's ev) has been read
      for (int e = tid; e < DTJ * DKC; e += 256) {
        const int r = e / DKC, kk = e % DKC, k = k0 + kk;
        const int ci = i0 + r, cj = j0 + r;
        if (r < DTI) xi[r][kk] = (ci < n_loc && k < K) ? x[((size_t)(c0 + ci) * B + b) * K + k] : 0.0f;
        xj[r][kk] = (cj < N && k < K) ? x[((size_t)cj * B + b) * K + k] : 0.0f;
      }
      __syncthreads();
      const int kn = min(DKC, K - k0);
      for (int k = 0; k < kn; ++k) {
        const float a = xi[ti][k];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float d = a - xj[tj + 16 * q][k];
          d2[q] = fmaf(d, d, d2[q]);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) ev[ti][tj + 16 * q] = expf(-(d2[q] * s));
    __syncthreads();
    if (tid < DTI) {
      const int jn = min(DTJ, N - j0);
      for (int j = 0; j < jn; ++j) total += ev[tid][j];
    }
  }
  if (tid < DTI && i0 + tid < n_loc) cost[(size_t)(i0 + tid) * B + b] = -total;
}

// ---- goal cost: one thread per candidate row, d = 0 .. D-1 in order -----------------------------------------------------------------------
__global__ void goal_cost_kernel(const float* __restrict__ x, int B, int64_t rows, int T, int D, int t_goal, const float* __restrict__ goal,
                                 const float* __restrict__ weight, float* __restrict__ cost) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const float* xr = x + ((size_t)r * T + t_goal) * D;
  const float* g = goal + (size_t)(r % B) * D;
  float acc = 0.0f;
  for (int d = 0; d < D; ++d) {
    const float e = xr[d] - g[d];
    acc = fmaf(weight[d] * e, e, acc);
  }
  cost[r] = acc;
}

// ---- argmin + gather: one work-group per observation ----------------------------------------------------------------------------------
// key = cost, a NaN as +inf; (key, c) pairs are compared lexicographically, so ties -- all-NaN columns among them -- go to the lowest c.
__device__ inline bool better(float ka, int ca, float kb, int cb) { return ka < kb || (ka == kb && ca < cb); }
__global__ __launch_bounds__(256) void select_kernel(const float* __restrict__ cost, const float* __restrict__ x, int B, int N, int K,
                                                     int* __restrict__ best_index, float* __restrict__ best_cost,
                                                     float* __restrict__ x_best) {
  __shared__ float rk[256];
  __shared__ int rc[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  float bk = INFINITY;
  int bc = 0x7fffffff;
  for (int c = tid; c < N; c += 256) {
    const float v = cost[(size_t)c * B + b];
    const float key = v != v ? INFINITY : v;
    if (better(key, c, bk, bc)) { bk = key; bc = c; }
  }
  rk[tid] = bk; rc[tid] = bc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w && better(rk[tid + w], rc[tid + w], rk[tid], rc[tid])) { rk[tid] = rk[tid + w]; rc[tid] = rc[tid + w]; }
    __syncthreads();
  }
  const int win = rc[0];                                   // < N: thread 0 always holds c = 0
  if (tid == 0) {
    best_index[b] = win;
    best_cost[b] = cost[(size_t)win * B + b];
  }
  const float* src = x + ((size_t)win * B + b) * K;
  for (int k = tid; k < K; k += 256) x_best[(size_t)b * K + k] = src[k];
}

}  // namespace
}  // namespace ldp

using namespace ldp;

extern "C" {

int ldp_plan_candidates(ldp_handle* h, const float* obs_emb, int32_t obs_frames, int32_t obs_horizon, int32_t B, int32_t c0,
                        int32_t n_loc, const float* x_init, const float* step_noise, uint64_t seed, int32_t sampler, int32_t n_steps,
                        float* x_out, int32_t use_graph, void* stream) {
  if (!h || !obs_emb || !x_out) return fail(LDP_EINVAL, "bad argument");
  if (B < 1) return fail(LDP_EINVAL, "B must be >= 1, got %d", B);
  if (c0 < 0) return fail(LDP_EINVAL, "c0 must be >= 0, got %d", c0);
  if (n_loc < 1) return fail(LDP_EINVAL, "n_loc must be >= 1, got %d", n_loc);
  if (!h->pl.ready) return fail(LDP_ESTATE, "planner weights not finalized");
  PlannerState& P = h->pl;
  if (obs_horizon <= 0 || obs_frames < obs_horizon || obs_horizon * P.D != P.G)
    return fail(LDP_EINVAL, "obs_horizon %d x obs_dim %d does not match global_cond_dim %d (frames given: %d)", obs_horizon, P.D, P.G,
                obs_frames);
  const int64_t rows = (int64_t)n_loc * B;
  if (rows > (1 << 24)) return fail(LDP_EINVAL, "n_loc * B = %lld candidate rows in one call (at most 2^24)", (long long)rows);
  LDP_TRY(entry_fault_check(h));
  hipStream_t s = (hipStream_t)stream;
  LDP_TRY(h->cand_cond.alloc((size_t)rows * P.G * 4));
  const int64_t n = rows * P.G;
  hipLaunchKernelGGL(tile_cond_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, obs_emb, h->cand_cond.f(), B, obs_frames,
                     P.D, P.G, rows);
  LDP_HIP(hipGetLastError());
  return ldp_plan_sample(h, h->cand_cond.f(), x_init, step_noise, seed, (int64_t)c0 * B, sampler, n_steps, x_out, (int32_t)rows,
                         use_graph, stream);
}

int ldp_plan_cost_density(const float* x_all, int32_t B, int32_t N, int32_t K, int32_t c0, int32_t n_loc, float bandwidth,
                          float* cost_out, void* stream) {
  if (!x_all || !cost_out) return fail(LDP_EINVAL, "bad argument");
  if (B < 1 || B > 65535) return fail(LDP_EINVAL, "B must be in 1..65535, got %d", B);
  if (N < 1) return fail(LDP_EINVAL, "N must be >= 1, got %d", N);
  if (K < 1) return fail(LDP_EINVAL, "K must be >= 1, got %d", K);
  if (c0 < 0) return fail(LDP_EINVAL, "c0 must be >= 0, got %d", c0);
  if (n_loc < 1) return fail(LDP_EINVAL, "n_loc must be >= 1, got %d", n_loc);
  if ((int64_t)c0 + n_loc > N) return fail(LDP_EINVAL, "c0 + n_loc = %lld exceeds N = %d", (long long)c0 + n_loc, N);
  if (!std::isfinite(bandwidth) || bandwidth <= 0.0f) return fail(LDP_EINVAL, "bandwidth must be finite and > 0, got %g", (double)bandwidth);
  hipStream_t s = (hipStream_t)stream;
  float* inv2h2 = nullptr;
  LDP_HIP(hipMallocAsync((void**)&inv2h2, (size_t)B * sizeof(float), s));
  hipLaunchKernelGGL(density_stats_kernel, dim3(B), dim3(ST_K * ST_G), 0, s, x_all, B, N, K, (double)bandwidth * (double)bandwidth, inv2h2);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) {
    hipLaunchKernelGGL(density_cost_kernel, dim3((unsigned)((n_loc + DTI - 1) / DTI), (unsigned)B), dim3(256), 0, s, x_all, B, N, K, c0,
                       n_loc, inv2h2, cost_out);
    e = hipGetLastError();
  }
  const hipError_t e2 = hipFreeAsync(inv2h2, s);
  if (e != hipSuccess) return fail(LDP_EHIP, "density cost launch: %s", hipGetErrorString(e));
  LDP_HIP(e2);
  return LDP_OK;
}

int ldp_plan_cost_goal(const float* x, int32_t B, int32_t n, int32_t T, int32_t D, int32_t t_goal, const float* goal,
                       const float* weight, float* cost_out, void* stream) {
  if (!x || !goal || !weight || !cost_out) return fail(LDP_EINVAL, "bad argument");
  if (B < 1) return fail(LDP_EINVAL, "B must be >= 1, got %d", B);
  if (n < 1) return fail(LDP_EINVAL, "n must be >= 1, got %d", n);
  if (T < 1 || D < 1) return fail(LDP_EINVAL, "T and D must be >= 1, got %d x %d", T, D);
  if (t_goal < 0 || t_goal >= T) return fail(LDP_EINVAL, "t_goal %d outside 0..%d", t_goal, T - 1);
  const int64_t rows = (int64_t)n * B;
  hipLaunchKernelGGL(goal_cost_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, B, rows, T, D, t_goal,
                     goal, weight, cost_out);
  LDP_HIP(hipGetLastError());
  return LDP_OK;
}

int ldp_plan_select(const float* cost_all, const float* x_all, int32_t B, int32_t N, int32_t K, int32_t* best_index_out,
                    float* best_cost_out, float* x_best_out, void* stream) {
  if (!cost_all || !x_all || !best_index_out || !best_cost_out || !x_best_out) return fail(LDP_EINVAL, "bad argument");
  if (B < 1) return fail(LDP_EINVAL, "B must be >= 1, got %d", B);
  if (N < 1) return fail(LDP_EINVAL, "N must be >= 1, got %d", N);
  if (K < 1) return fail(LDP_EINVAL, "K must be >= 1, got %d", K);
  hipLaunchKernelGGL(select_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, cost_all, x_all, B, N, K, best_index_out, best_cost_out,
                     x_best_out);
  LDP_HIP(hipGetLastError());
  return LDP_OK;
}

}  // extern "C"
