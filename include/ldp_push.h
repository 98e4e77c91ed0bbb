/* ldp_push.h -- C ABI of libldp_push.so: the device-resident pushing task `push2d` (csrc/push.hip).
 * A library of its own beside libldp_hip.so (include/ldp_hip.h), libldp_env.so (include/ldp_env.h) and libldp_pix.so (include/ldp_pix.h):
 * it shares nothing with them but the Philox generator (csrc/tconv.hpp) and the stream the caller passes.  Same conventions: device
 * pointers as plain pointers, `stream` a hipStream_t (NULL: the default stream), every call returns LDP_PUSH_OK or a negative
 * code and leaves a message for ldp_push_last_error() (thread-local); nothing synchronises, nothing is read from the environment. */
#ifndef LDP_PUSH_H
#define LDP_PUSH_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define LDP_PUSH_API __attribute__((visibility("default")))

#define LDP_PUSH_OK 0
#define LDP_PUSH_EINVAL (-1)   /* bad argument: the message names it */
#define LDP_PUSH_EHIP (-3)     /* a HIP runtime call failed           */

/* Philox stream of the task, beside the LDP_PHILOX_STREAM_* of include/ldp_hip.h (0, 1, 7 .. 12) and LDP_PHILOX_STREAM_ENV (13):
 * element = the global episode, step 0 the reset, step 1 + t a scripted policy's noise at time t */
#define LDP_PHILOX_STREAM_PUSH 14u

LDP_PUSH_API const char* ldp_push_last_error(void);

/* `push2d`: a point (radius 0.05) in [-1, 1]^2 pushes a disc (radius 0.15) to a goal.  The point starts on the left; the goal is on the
 * left or on the right, so in half of the episodes the point starts on the wrong side of the disc and has to go round it.  Contact is a
 * projection: a move that would bring the point's centre within C of the disc's puts the disc at distance C along the contact normal.
 * N environments run in lockstep, one thread each; a control cycle (n_sub sub-steps) is ONE launch.  Stateless: no handle, no
 * workspace, no atomics -- the outputs are a pure function of the arguments.  Defined by this repository.
 * All arithmetic is fp32 with every operation rounded once (rn), fma fused where written, sqrt and / correctly rounded, no
 * transcendental function: tests/pushenv_oracle.py restates it in NumPy and the kernels reproduce it bit for bit.
 *   constants   C = 0.2, DT = 0.08, TOL = 0.1, LIM = 0.85; C2 = rn(C * C), TOL2 = rn(TOL * TOL); an episode has LDP_PUSH_EPISODE_LEN steps
 *   state       (N, LDP_PUSH_STATE) floats, 16-byte aligned, three float4: px, py, ox, oy | gx, gy, side (+-1), t | first, blocked, pushed, 0
 *               (t and the last three before the pad: counts held as floats)
 *   draws       w = Philox words of (seed, element = episode0 + env, step, LDP_PHILOX_STREAM_PUSH); u(w) = (w >> 8) * 2^-24
 *   reset       step 0: p = (-0.8, -0.5 + u(w0));  o = (fma(0.6, u(w1), -0.3), fma(0.8, u(w2), -0.4));
 *               g = ((w0 & 1) ? -0.6 : 0.6, -0.5 + u(w3));  side = (w1 & 1) ? +1 : -1;  the rest 0.  (u drops the low bits: they are independent of it.)
 *   sub-step    with action a (only a[0], a[1] are read; NaN reads as 0; clamped to [-1, 1]):
 *               q = clamp(fma(DT, a, p), -1, 1);  d = rn(o - q);  d2 = fma(dx, dx, rn(dy * dy));
 *               d2 < C2:  dist = sqrt(d2);  n = dist > 0 ? (dx / dist, dy / dist) : (1, 0);  o' = fma(C, n, q);
 *                         |o'x| > LIM or |o'y| > LIM: the move is refused, blocked += 1, p and o stay;
 *                         otherwise p = q, o = o', pushed += 1;
 *               else      p = q;
 *               t += 1;  e = rn(o - g);  first == 0 and fma(ex, ex, rn(ey * ey)) <= TOL2: first = t.
 *               Success: first != 0 (latched).  It says where the disc is, not where the point is.
 *   policies    r = (fma(2, u(w0), -1), fma(2, u(w1), -1)) from the draws of step 1 + t (t: the state's own time);   random: a = r;
 *               the others head for a target:  dd = rn(rn(tgt - p) * 12.5);  m = max(|ddx|, |ddy|, 1);  a = clamp(fma(noise, r, dd / m), -1, 1)
 *               straight: tgt = o
 *               expert:   v = rn(g - o);  L = sqrt(fma(vx, vx, rn(vy * vy)));  uh = v / max(L, 1e-6);  nh = (-uhy, uhx);  rr = rn(p - o);
 *                         along = fma(rrx, uhx, rn(rry * uhy));  lat = fma(rrx, nhx, rn(rry * nhy));
 *                         s = |lat| > 0.05 ? sign(lat) : side;
 *                         appr = fma(-0.3, uh, o);  push = fma(-0.1, uh, o);
 *                         wp = fma(0.39 * s, nh, fma(clamp(along, -1, 1), uh, o));  corner = fma(0.39 * s, nh, appr);
 *                         behind = along < -0.1 and |lat| < rn(0.6 * |along|);  ahead = along > -0.25;
 *                         tgt = behind ? push : ahead ? (|lat| < 0.3 ? wp : corner) : appr
 *   observation pos (2) = p, goal (2) = g, latent (LDP_PUSH_LATENT = 16) = the pairs (T1, T2) = (x, fma(2x, x, -1)) of the eight numbers
 *               px, py, ox, oy, rn(rn(gx - ox) * 0.5), rn(rn(gy - oy) * 0.5), rn(rn(ox - px) * 0.5), rn(rn(oy - py) * 0.5), in that order.
 *               Every value lies in [-1, 1].  The disc's position is in the latent only.
 * episode0 makes environment i the global episode episode0 + i whatever the split of a batch over calls. */
#define LDP_PUSH_STATE 12
#define LDP_PUSH_LATENT 16
#define LDP_PUSH_EPISODE_LEN 48
#define LDP_PUSH_POLICY_GIVEN 0     /* the actions argument */
#define LDP_PUSH_POLICY_EXPERT 1
#define LDP_PUSH_POLICY_STRAIGHT 2
#define LDP_PUSH_POLICY_RANDOM 3

/* state (N, 12) <- the reset of episodes episode0 .. episode0 + N - 1.  LDP_PUSH_EINVAL: N < 1, episode0 < 0, a null or misaligned state. */
LDP_PUSH_API int ldp_push_reset(float* state, int32_t N, uint64_t seed, int64_t episode0, void* stream);

/* The observation of every environment as (N, 1, 2) / (N, 1, 2) / (N, 1, 16) floats; any of the three may be NULL (not all). */
LDP_PUSH_API int ldp_push_observe(const float* state, int32_t N, float* pos, float* goal, float* latent, void* stream);

/* n_sub sub-steps of every environment in ONE launch, in place on state.  policy LDP_PUSH_POLICY_GIVEN: sub-step j of environment i
 * takes actions[i, j, :2] of the device tensor actions (N, n_sub, A); a scripted policy (actions NULL) computes its own with `noise`
 * and the draws of (seed, episode0 + i).  Optional outputs (NULL: not written): actions_out (N, n_sub, A) the actions taken
 * (after NaN -> 0 and the clamp; components from 2 up are written as 0; must not alias actions), pos_out / goal_out / latent_out
 * (N, n_sub, 2 / 2 / 16) the observation IN FRONT OF every sub-step -- how demonstrations are recorded.
 * LDP_PUSH_EINVAL names the argument: N < 1, n_sub < 1, A < 2, an unknown policy, a noise that is not finite, episode0 < 0, actions
 * without policy 0 or policy 0 without actions. */
LDP_PUSH_API int ldp_push_step(float* state, int32_t N, int32_t n_sub, const float* actions, int32_t A, int32_t policy, float noise,
                               uint64_t seed, int64_t episode0, float* actions_out, float* pos_out, float* goal_out, float* latent_out,
                               void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LDP_PUSH_H */
