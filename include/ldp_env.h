/* ldp_env.h -- C ABI of libldp_env.so: the device-resident reach task `reach2d` (csrc/env.hip).
 * A library of its own beside libldp_hip.so (include/ldp_hip.h): the task is not part of the agent's engine, needs no handle and
 * shares nothing with it but the Philox generator (csrc/tconv.hpp) and the stream the caller passes.  Same conventions: device
 * pointers as plain pointers, `stream` a hipStream_t (NULL: the default stream), every call returns LDP_ENV_OK or a negative
 * code and leaves a message for ldp_env_last_error() (thread-local); nothing synchronises, nothing is read from the environment. */
#ifndef LDP_ENV_H
#define LDP_ENV_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define LDP_ENV_API __attribute__((visibility("default")))

#define LDP_ENV_OK 0
#define LDP_ENV_EINVAL (-1)   /* bad argument: the message names it */
#define LDP_ENV_EHIP (-3)     /* a HIP runtime call failed           */

/* Philox stream of the task, beside the LDP_PHILOX_STREAM_* of include/ldp_hip.h (0, 1, 7 .. 12): element = the global episode,
 * step 0 the reset, step 1 + t a scripted policy's noise at time t */
#define LDP_PHILOX_STREAM_ENV 13u

LDP_ENV_API const char* ldp_env_last_error(void);

/* `reach2d`, a fully specified control task that lives where the plans live: a point in [-1, 1]^2 starts on the left, the goal
 * is on the right, a blocking disc of radius R sits at the origin.  N environments run in lockstep, one thread each; a control
 * cycle (n_sub sub-steps) is ONE launch.  Stateless: no handle, no workspace, no atomics -- the outputs are a pure function of
 * the arguments.  Defined by this repository (the reference evaluates in robosuite / dm_control).
 * All arithmetic is fp32 with every operation rounded once (rn), fma fused, no transcendental function: tests/toyenv_oracle.py
 * restates it in NumPy and the kernels reproduce it bit for bit.
 *   constants   R = 0.3, DT = 0.08, TOL = 0.08, WY = 0.65; R^2 = rn(R * R), TOL^2 = rn(TOL * TOL); an episode has LDP_ENV_EPISODE_LEN steps
 *   state       (N, LDP_ENV_STATE) floats, 16-byte aligned: px, py, gx, gy, side (+-1), t, first, blocked (the last three: counts held as floats)
 *   draws       w = Philox words of (seed, element = episode0 + env, step, LDP_PHILOX_STREAM_ENV); u(w) = (w >> 8) * 2^-24
 *   reset       step 0: p = (-0.8, -0.5 + u(w0)), g = (0.8, -0.5 + u(w1)), side = (w2 & 1) ? +1 : -1, t = first = blocked = 0
 *   sub-step    with action a (only a[0], a[1] are read; NaN reads as 0; clamped to [-1, 1]):
 *               q = clamp(fma(DT, a, p), -1, 1);  fma(qx, qx, rn(qy * qy)) < R^2: the move is refused, blocked += 1;  otherwise p = q;
 *               t += 1;  d = p - g;  first == 0 and fma(dx, dx, rn(dy * dy)) <= TOL^2: first = t.  Success: first != 0 (latched).
 *   policies    r = (fma(2, u(w0), -1), fma(2, u(w1), -1)) from the draws of step 1 + t (t: the state's own time);
 *               expert: tgt = px < 0 ? (0, side * WY) : g;  d = rn(rn(tgt - p) * 12.5);  m = max(|dx|, |dy|, 1);
 *                       a = clamp(fma(noise, r, d / m), -1, 1);   straight: the same with tgt = g;   random: a = r
 *   observation pos (2) = p, goal (2) = g, latent (LDP_ENV_LATENT = 16) = Chebyshev T1..T4 of px, py, rn(rn(gx - px) * 0.5),
 *               rn(rn(gy - py) * 0.5), in that order: T1 = u, T2 = fma(2u, u, -1), T3 = fma(2u, T2, -u), T4 = fma(2u, T3, -T2).
 *               Every value lies in [-1, 1].
 * episode0 makes environment i the global episode episode0 + i whatever the split of a batch over calls. */
#define LDP_ENV_STATE 8
#define LDP_ENV_LATENT 16
#define LDP_ENV_EPISODE_LEN 48
#define LDP_ENV_POLICY_GIVEN 0     /* the actions argument */
#define LDP_ENV_POLICY_EXPERT 1
#define LDP_ENV_POLICY_STRAIGHT 2
#define LDP_ENV_POLICY_RANDOM 3

/* state (N, 8) <- the reset of episodes episode0 .. episode0 + N - 1.  LDP_ENV_EINVAL: N < 1, episode0 < 0, a null or misaligned state. */
LDP_ENV_API int ldp_env_reset(float* state, int32_t N, uint64_t seed, int64_t episode0, void* stream);

/* The observation of every environment as (N, 1, 2) / (N, 1, 2) / (N, 1, 16) floats; any of the three may be NULL (not all). */
LDP_ENV_API int ldp_env_observe(const float* state, int32_t N, float* pos, float* goal, float* latent, void* stream);

/* n_sub sub-steps of every environment in ONE launch, in place on state.  policy LDP_ENV_POLICY_GIVEN: sub-step j of environment i
 * takes actions[i, j, :2] of the device tensor actions (N, n_sub, A); a scripted policy (actions NULL) computes its own with `noise`
 * and the draws of (seed, episode0 + i).  Optional outputs (NULL: not written): actions_out (N, n_sub, A) the actions taken
 * (after NaN -> 0 and the clamp; components from 2 up are written as 0; must not alias actions), pos_out / goal_out / latent_out
 * (N, n_sub, 2 / 2 / 16) the observation IN FRONT OF every sub-step -- how demonstrations are recorded.
 * LDP_ENV_EINVAL names the argument: N < 1, n_sub < 1, A < 2, an unknown policy, a noise that is not finite, episode0 < 0, actions
 * without policy 0 or policy 0 without actions. */
LDP_ENV_API int ldp_env_step(float* state, int32_t N, int32_t n_sub, const float* actions, int32_t A, int32_t policy, float noise,
                             uint64_t seed, int64_t episode0, float* actions_out, float* pos_out, float* goal_out, float* latent_out,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LDP_ENV_H */
