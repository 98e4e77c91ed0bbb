/* ldp_pix.h -- C ABI of libldp_pix.so: the camera of the reach task `reach2d` (csrc/pix.hip).
 * A library of its own beside libldp_env.so (include/ldp_env.h) and libldp_hip.so (include/ldp_hip.h): it renders the scene the task's
 * state describes and shares nothing with either but the stream the caller passes.  Same conventions: device pointers as plain
 * pointers, `stream` a hipStream_t (NULL: the default stream), every call returns LDP_PIX_OK or a negative code and leaves a message
 * for ldp_pix_last_error() (thread-local); nothing synchronises, nothing is read from the environment. */
#ifndef LDP_PIX_H
#define LDP_PIX_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define LDP_PIX_API __attribute__((visibility("default")))

#define LDP_PIX_OK 0
#define LDP_PIX_EINVAL (-1)   /* bad argument: the message names it */
#define LDP_PIX_EHIP (-3)     /* a HIP runtime call failed           */

#define LDP_PIX_SIZE 64                                        /* a frame is LDP_PIX_SIZE x LDP_PIX_SIZE x 3 bytes, row-major, RGB interleaved */
#define LDP_PIX_FRAME_BYTES (LDP_PIX_SIZE * LDP_PIX_SIZE * 3)  /* 12 288 */

LDP_PIX_API const char* ldp_pix_last_error(void);

/* The scene of `reach2d` as a camera frame: the square [-1, 1]^2 on 64 x 64 pixels, one soft blob per channel.  Stateless: no handle,
 * no workspace, no atomics -- the frame is a pure function of the two centres.  All arithmetic is fp32 with every operation rounded
 * once (rn), fma fused, no transcendental function: tests/pix_oracle.py restates it in NumPy and the kernel reproduces it byte for byte.
 *   pixel centres  c_k = (2k - 63) * 2^-6 for k = 0 .. 63 (exact in fp32).  Row i has y = c_i (row 0 is the BOTTOM), column j has x = c_j.
 *   blob(q, K)     at the pixel (x, y):  dx = rn(x - qx);  dy = rn(y - qy);  d2 = fma(dx, dx, rn(dy * dy));  t = fma(-d2, K, 1);
 *                  s = t > 0 ? t : 0 (a NaN centre gives 0);  v = rn(s * s);  byte = (uint8) trunc(fma(255, v, 0.5))
 *   channel 0 (R)  blob(p, 16): the point; radius 1 / sqrt(16) = 0.25, which is 8 pixels
 *   channel 1 (G)  blob(g, 16): the goal
 *   channel 2 (B)  blob((0, 0), 11.111111f): the blocking disc (radius 0.3); the same in every frame
 * The blobs live in separate channels, so nothing occludes anything; the quadratic edge is what carries sub-pixel position. */
#define LDP_PIX_K_POINT 16.0f
#define LDP_PIX_K_DISC 11.111111f

/* frames (M, 64, 64, 3) uint8, 16-byte aligned <- the scenes of M rows.  pos / goal: row r at pos + r * pos_stride floats (two floats
 * read), likewise goal; so the live state (N, 8) of ldp_env.h serves with pos = state, goal = state + 2, both strides 8, and recorded
 * (M, 2) tables with stride 2.  ONE launch, whatever M.
 * LDP_PIX_EINVAL names the argument, before any HIP call: M < 1, a null pos, goal or frames, a stride < 2, frames not 16-byte aligned. */
LDP_PIX_API int ldp_pix_render(const float* pos, int64_t pos_stride, const float* goal, int64_t goal_stride, int64_t M, uint8_t* frames,
                               void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LDP_PIX_H */
