// pix.hip -- the camera of the reach task (include/ldp_pix.h), built into a library of its own (libldp_pix.so): the scene of
// `reach2d` rasterised to 64 x 64 x 3 bytes per row of (pos, goal).  A pure streaming-store kernel: 16 bytes in and 12 288 bytes out per frame, no
// LDS, no atomics, no workspace.  One thread produces 16 consecutive bytes of a frame and stores them with one 16-byte vector store.  Exact fp32
// on the VALU, every operation rounded once and spelled (__fmaf_rn, __fmul_rn, ...), contraction off; no transcendental function.
// tests/pix_oracle.py restates the scene in NumPy float32 and the kernel reproduces it byte for byte.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <string>

#include "../../include/ldp_pix.h"

#pragma clang fp contract(off)

namespace ldp {
namespace {

// the library's own error plumbing (as env.hip: libldp_hip.so's is not linked here)
std::string& pix_last_error() {
  static thread_local std::string e;
  return e;
}

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  pix_last_error() = buf;
  return code;
}

#define PIX_HIP(expr)                                                                                                       \
  do {                                                                                                                      \
    hipError_t _e = (expr);                                                                                                 \
    if (_e != hipSuccess) return fail(LDP_PIX_EHIP, "%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
  } while (0)

// A frame row is 64 pixels x 3 bytes = 192 B = 12 chunks of 16 B, so a chunk never straddles a row: one y, five or six x.  A frame is 768
// chunks = 3 work-groups of 256 threads = 12 waves: the UNIT of work is a third of a frame, the frame index is uniform over the work-group and
// the four centre floats arrive through the scalar cache.
constexpr int PT = 256;                           // threads per work-group = chunks per unit
constexpr int PIX_ROW_CHUNKS = LDP_PIX_SIZE * 3 / 16;                       // 12
constexpr int PIX_FRAME_UNITS = LDP_PIX_FRAME_BYTES / 16 / PT;             // 3
constexpr unsigned PIX_MAX_BLOCKS = 2048;         // 8 resident work-groups on each of 256 CUs; the rest is strided
static_assert(PIX_ROW_CHUNKS * 16 == LDP_PIX_SIZE * 3 && PIX_FRAME_UNITS * PT * 16 == LDP_PIX_FRAME_BYTES, "chunks tile rows and units tile frames");

// c_k = (2k - 63) * 2^-6: exact
__device__ __forceinline__ float pixel_centre(int k) { return __fmul_rn((float)(2 * k - (LDP_PIX_SIZE - 1)), 1.0f / LDP_PIX_SIZE); }

// blob(q, K) at a pixel whose rn(dy * dy) is dy2
__device__ __forceinline__ uint32_t blob_byte(float x, float qx, float dy2, float K) {
  const float dx = __fsub_rn(x, qx);
  const float d2 = __fmaf_rn(dx, dx, dy2);
  const float t = __fmaf_rn(-d2, K, 1.0f);
  const float s = t > 0.0f ? t : 0.0f;            // NaN -> 0
  const float v = __fmul_rn(s, s);
  return (uint32_t)__fmaf_rn(255.0f, v, 0.5f);    // in [0.5, 255.5]: the conversion truncates
}

__global__ __launch_bounds__(PT) void pix_render_kernel(const float* __restrict__ pos, int64_t pos_stride, const float* __restrict__ goal,
                                                        int64_t goal_stride, int64_t units, uint8_t* __restrict__ frames) {
  const int tid = threadIdx.x;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {                       // u < 3 M: 64-bit, M * 12 288 passes 2^31 at 174 763 frames
    const int64_t f = u / PIX_FRAME_UNITS;
    const int q = (int)(u - f * PIX_FRAME_UNITS) * PT + tid;                      // the chunk within the frame, 0 .. 767
    const int row = q / PIX_ROW_CHUNKS, k = q - row * PIX_ROW_CHUNKS;
    const float* p = pos + f * pos_stride;
    const float* g = goal + f * goal_stride;
    const float cx[3] = {p[0], g[0], 0.0f}, cy[3] = {p[1], g[1], 0.0f};        // uniform over the work-group: scalar loads
    const float y = pixel_centre(row);
    float cd[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float dy = __fsub_rn(y, cy[c]);
      cd[c] = __fmul_rn(dy, dy);
    }
    // byte e of the chunk is byte 16 k + e of the row: channel (ph + e) % 3 of pixel j0 + (ph + e) / 3.  With e = 3 a + r the channel depends on
    // r alone, so the three channels are rotated by ph ONCE and byte e reads slot r; its pixel is j0 + [ph + r >= 3] + a.
    const int j0 = (16 * k) / 3, ph = 16 * k - 3 * j0;
    float qx[3], d2y[3], K[3], xb[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int c1 = (r + 1) % 3, c2 = (r + 2) % 3;
      qx[r] = ph == 0 ? cx[r] : ph == 1 ? cx[c1] : cx[c2];
      d2y[r] = ph == 0 ? cd[r] : ph == 1 ? cd[c1] : cd[c2];
      K[r] = r == 2 - ph ? LDP_PIX_K_DISC : LDP_PIX_K_POINT;                    // the disc's channel 2 sits in slot 2 - ph
      xb[r] = pixel_centre(j0 + (ph + r >= 3 ? 1 : 0));
    }
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int a = e / 3, r = e - 3 * a;
      const float x = __fadd_rn(xb[r], (float)a * (2.0f / LDP_PIX_SIZE));       // c_{j + a} = c_j + a * 2^-5: exact
      w[e >> 2] |= blob_byte(x, qx[r], d2y[r], K[r]) << (8 * (e & 3));
    }
    *reinterpret_cast<uint4*>(frames + (u * PT + tid) * 16) = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

}  // namespace
}  // namespace ldp

using namespace ldp;

extern "C" {

const char* ldp_pix_last_error(void) { return pix_last_error().c_str(); }

int ldp_pix_render(const float* pos, int64_t pos_stride, const float* goal, int64_t goal_stride, int64_t M, uint8_t* frames, void* stream) {
  if (M < 1) return fail(LDP_PIX_EINVAL, "M must be >= 1, got %lld", (long long)M);
  if (!pos) return fail(LDP_PIX_EINVAL, "null pos");
  if (!goal) return fail(LDP_PIX_EINVAL, "null goal");
  if (!frames) return fail(LDP_PIX_EINVAL, "null frames");
  if (pos_stride < 2) return fail(LDP_PIX_EINVAL, "pos_stride must be >= 2 (two floats are read per row), got %lld", (long long)pos_stride);
  if (goal_stride < 2) return fail(LDP_PIX_EINVAL, "goal_stride must be >= 2 (two floats are read per row), got %lld", (long long)goal_stride);
  if ((uintptr_t)frames % 16) return fail(LDP_PIX_EINVAL, "frames must be 16-byte aligned");
  if (M > INT64_MAX / LDP_PIX_FRAME_BYTES) return fail(LDP_PIX_EINVAL, "M = %lld frames do not fit a 64-bit byte count", (long long)M);
  const int64_t units = M * PIX_FRAME_UNITS;
  const unsigned blocks = (unsigned)std::min<int64_t>(units, PIX_MAX_BLOCKS);
  hipLaunchKernelGGL(pix_render_kernel, dim3(blocks), dim3(PT), 0, (hipStream_t)stream, pos, pos_stride, goal, goal_stride, units, frames);
  PIX_HIP(hipGetLastError());
  return LDP_PIX_OK;
}

}  // extern "C"
