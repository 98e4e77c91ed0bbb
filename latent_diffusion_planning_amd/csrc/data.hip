// data.hip -- the device-resident training data layer (include/ldp_hip.h "device-resident training data"): the window
// indices of a batch from Philox and the gather of the episode-clamped windows of every key, in one launch.  A pure copy: bandwidth- and
// latency-bound, no matrix work, no atomics, no state -- the outputs are a function of the arguments alone.
#include "common.hpp"
#include "tconv.hpp"

namespace ldp {
namespace {

// Both tables travel by value as kernel arguments (no upload is enqueued, nothing outlives the call).
struct DataSets {
  int64_t base[LDP_DATA_MAX_SETS], total[LDP_DATA_MAX_SETS];
  uint64_t thr[LDP_DATA_MAX_SETS];
  int32_t n;
};
struct DataKeys {
  const char* table[LDP_DATA_MAX_KEYS];
  char* out[LDP_DATA_MAX_KEYS];
  uint32_t row_units[LDP_DATA_MAX_KEYS];   // row_bytes in units of the key's vector (16 or 4 bytes)
  uint32_t units[LDP_DATA_MAX_KEYS];       // n_rows * row_units: one sample's window
  uint32_t block0[LDP_DATA_MAX_KEYS];      // first work-group of the key among the work-groups of one sample
  int32_t first_row[LDP_DATA_MAX_KEYS];
  uint32_t vec16;                          // bit k: key k moves as 16-byte vectors
  int32_t n;
};

constexpr int DT = 256;                    // threads per work-group
constexpr int DQ = 4;                      // vectors per thread: all DQ loads are issued before the first store
constexpr uint32_t DUNITS = DT * DQ;       // vectors per work-group: 16 KiB of 16-byte vectors, 4 KiB of words

// global row r of a call -> welded row (header: the first d with w[1] < thr[d], then the multiply-shift map onto [0, total_d))
__device__ __forceinline__ int64_t draw_index(const DataSets& S, uint64_t seed, uint64_t r, uint32_t step) {
  uint32_t w[4];
  philox4x32_10(seed, r, step, LDP_PHILOX_STREAM_DATA, w);
  int d = 0;
  while (d < S.n - 1 && (uint64_t)w[1] >= S.thr[d]) ++d;
  return S.base[d] + (int64_t)(((uint64_t)w[0] * (uint64_t)S.total[d]) >> 32);
}

__global__ void data_draw_kernel(uint64_t seed, uint64_t row0, uint32_t step, int32_t B, int64_t* __restrict__ index_out, const DataSets S) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) index_out[b] = draw_index(S, seed, row0 + (uint64_t)b, step);
}

// Units [u0, uend) (step DT) of one sample's window of one key: unit u is vector u % ru of window row u / ru, which is welded row
// clamp(first + u / ru, lo, hi).  Consecutive lanes read consecutive vectors of a row and write consecutive vectors of the output.
template <class V>
__device__ __forceinline__ void copy_window(const char* __restrict__ table, char* __restrict__ out, uint32_t ru, int64_t first, int64_t lo,
                                            int64_t hi, uint32_t u0, uint32_t uend) {
  V v[DQ];
#pragma unroll
  for (int q = 0; q < DQ; ++q) {
    const uint32_t u = min(u0 + q * DT, uend - 1);     // past the end: the last unit again (loaded, never stored), so that v stays in registers
    const uint32_t j = u / ru, w = u - j * ru;
    int64_t row = first + (int64_t)j;
    row = row < lo ? lo : row > hi ? hi : row;
    v[q] = *reinterpret_cast<const V*>(table + ((size_t)row * ru + w) * sizeof(V));
  }
#pragma unroll
  for (int q = 0; q < DQ; ++q) {
    const uint32_t u = u0 + q * DT;
    if (u < uend) *reinterpret_cast<V*>(out + (size_t)u * sizeof(V)) = v[q];
  }
}

// Work-group x = b * bps + j: sample b, and j names (key, 16-KiB piece of its window) through block0.  Every work-group of a sample derives
// the sample's index itself (ten Philox rounds and one 8-byte load: cheaper than a second launch or an exchange).
__global__ __launch_bounds__(DT) void data_sample_kernel(const int32_t* __restrict__ bounds, const int64_t* __restrict__ index_in,
                                                         int64_t* __restrict__ index_out, uint64_t seed, uint64_t row0, uint32_t step,
                                                         int32_t fs, uint32_t bps, int64_t total_rows, const DataSets S, const DataKeys K) {
  const uint32_t b = blockIdx.x / bps, j = blockIdx.x - b * bps;
  int k = 0;
  for (int q = 1; q < K.n; ++q)
    if (K.block0[q] <= j) k = q;
  int64_t i;
  if (index_in) {
    i = index_in[b];
    i = i < 0 ? 0 : i >= total_rows ? total_rows - 1 : i;
  } else {
    i = draw_index(S, seed, row0 + (uint64_t)b, step);
  }
  if (index_out && j == 0 && threadIdx.x == 0) index_out[b] = i;
  const int2 se = reinterpret_cast<const int2*>(bounds)[i];      // the episode [s, e) of welded row i
  const int64_t first = i - (int64_t)(fs - 1) + K.first_row[k];
  const uint32_t units = K.units[k], ru = K.row_units[k];
  const uint32_t u0 = (j - K.block0[k]) * DUNITS + threadIdx.x;
  const uint32_t uend = min(u0 - threadIdx.x + DUNITS, units);
  if ((K.vec16 >> k) & 1)
    copy_window<uint4>(K.table[k], K.out[k] + (size_t)b * units * 16, ru, first, se.x, (int64_t)se.y - 1, u0, uend);
  else
    copy_window<uint32_t>(K.table[k], K.out[k] + (size_t)b * units * 4, ru, first, se.x, (int64_t)se.y - 1, u0, uend);
}

int fill_sets(DataSets& S, const int64_t* base, const int64_t* total, const uint64_t* thr, int32_t n_sets, int64_t total_rows) {
  if (!base || !total || !thr) return fail(LDP_EINVAL, "null dataset table");
  if (n_sets < 1 || n_sets > LDP_DATA_MAX_SETS) return fail(LDP_EINVAL, "n_sets must be in 1..%d, got %d", LDP_DATA_MAX_SETS, n_sets);
  S = DataSets{};
  S.n = n_sets;
  for (int d = 0; d < n_sets; ++d) {
    if (total[d] < 1 || total[d] >= ((int64_t)1 << 31))
      return fail(LDP_EINVAL, "dataset %d has %lld samples: the draw needs 1 <= total < 2^31", d, (long long)total[d]);
    if (base[d] < 0 || (total_rows >= 0 && base[d] + total[d] > total_rows))
      return fail(LDP_EINVAL, "dataset %d covers rows [%lld, %lld) outside the %lld welded rows", d, (long long)base[d],
                  (long long)(base[d] + total[d]), (long long)total_rows);
    if (d > 0 && thr[d] < thr[d - 1]) return fail(LDP_EINVAL, "thr must not decrease (dataset %d)", d);
    S.base[d] = base[d]; S.total[d] = total[d]; S.thr[d] = thr[d];
  }
  S.thr[n_sets - 1] = (uint64_t)1 << 32;
  return LDP_OK;
}

}  // namespace
}  // namespace ldp

using namespace ldp;

extern "C" {

int ldp_data_draw(const int64_t* dataset_base, const int64_t* dataset_total, const uint64_t* thr, int32_t n_sets, uint64_t seed,
                  int64_t row_offset, uint32_t step, int32_t B, int64_t* index_out, void* stream) {
  if (!index_out) return fail(LDP_EINVAL, "null index_out");
  if (B < 1) return fail(LDP_EINVAL, "B must be >= 1, got %d", B);
  if (row_offset < 0) return fail(LDP_EINVAL, "row_offset must be >= 0, got %lld", (long long)row_offset);
  DataSets S;
  LDP_TRY(fill_sets(S, dataset_base, dataset_total, thr, n_sets, -1));
  hipLaunchKernelGGL(data_draw_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, (hipStream_t)stream, seed, (uint64_t)row_offset, step, B,
                     index_out, S);
  LDP_HIP(hipGetLastError());
  return LDP_OK;
}

int ldp_data_sample(const ldp_data_key* keys, int32_t n_keys, const int32_t* bounds, int64_t total_rows, const int64_t* dataset_base,
                    const int64_t* dataset_total, const uint64_t* thr, int32_t n_sets, uint64_t seed, int64_t row_offset, uint32_t step,
                    int32_t B, int32_t frame_stack, int32_t seq_length, const int64_t* index_in, int64_t* index_out, void* stream) {
  if (!keys || !bounds) return fail(LDP_EINVAL, "null key table or bounds table");
  if (n_keys < 1 || n_keys > LDP_DATA_MAX_KEYS) return fail(LDP_EINVAL, "n_keys must be in 1..%d, got %d", LDP_DATA_MAX_KEYS, n_keys);
  if (B < 1) return fail(LDP_EINVAL, "B must be >= 1, got %d", B);
  if (frame_stack < 1) return fail(LDP_EINVAL, "frame_stack must be >= 1, got %d", frame_stack);
  if (seq_length < 1) return fail(LDP_EINVAL, "seq_length must be >= 1, got %d", seq_length);
  if (row_offset < 0) return fail(LDP_EINVAL, "row_offset must be >= 0, got %lld", (long long)row_offset);
  if (total_rows < 1 || total_rows >= ((int64_t)1 << 31)) return fail(LDP_EINVAL, "total_rows must be in 1..2^31-1, got %lld", (long long)total_rows);
  if ((uintptr_t)bounds % 8) return fail(LDP_EINVAL, "bounds must be 8-byte aligned");
  const int64_t W = (int64_t)frame_stack + seq_length - 1;
  DataSets S;
  LDP_TRY(fill_sets(S, dataset_base, dataset_total, thr, n_sets, total_rows));
  DataKeys K{};
  K.n = n_keys;
  uint64_t bps = 0;
  for (int k = 0; k < n_keys; ++k) {
    const ldp_data_key& d = keys[k];
    if (!d.table || !d.out) return fail(LDP_EINVAL, "key %d: null table or output", k);
    if (d.row_bytes < 4 || d.row_bytes % 4) return fail(LDP_EINVAL, "key %d: row_bytes must be a positive multiple of 4, got %lld", k, (long long)d.row_bytes);
    if (d.first_row < 0 || d.n_rows < 1 || (int64_t)d.first_row + d.n_rows > W)
      return fail(LDP_EINVAL, "key %d: window rows [%d, %d) outside the %lld rows of frame_stack %d + seq_length %d - 1", k, d.first_row,
                  d.first_row + d.n_rows, (long long)W, frame_stack, seq_length);
    if ((uintptr_t)d.table % 4 || (uintptr_t)d.out % 4) return fail(LDP_EINVAL, "key %d: table and output must be 4-byte aligned", k);
    if (d.row_bytes * d.n_rows >= ((int64_t)1 << 31))
      return fail(LDP_EINVAL, "key %d: one window has %lld bytes (at most 2^31 - 1)", k, (long long)(d.row_bytes * d.n_rows));
    const bool v16 = d.row_bytes % 16 == 0 && (uintptr_t)d.table % 16 == 0 && (uintptr_t)d.out % 16 == 0;
    const uint32_t vb = v16 ? 16 : 4;
    K.table[k] = static_cast<const char*>(d.table);
    K.out[k] = static_cast<char*>(d.out);
    K.row_units[k] = (uint32_t)(d.row_bytes / vb);
    K.units[k] = K.row_units[k] * (uint32_t)d.n_rows;
    K.first_row[k] = d.first_row;
    K.block0[k] = (uint32_t)bps;
    if (v16) K.vec16 |= 1u << k;
    bps += (K.units[k] + DUNITS - 1) / DUNITS;
  }
  if (bps * (uint64_t)B >= ((uint64_t)1 << 31))
    return fail(LDP_EINVAL, "%llu work-groups per sample x %d samples exceed one launch", (unsigned long long)bps, B);
  hipLaunchKernelGGL(data_sample_kernel, dim3((unsigned)(bps * (uint64_t)B)), dim3(DT), 0, (hipStream_t)stream, bounds, index_in, index_out, seed,
                     (uint64_t)row_offset, step, frame_stack, (uint32_t)bps, total_rows, S, K);
  LDP_HIP(hipGetLastError());
  return LDP_OK;
}

}  // extern "C"
