/* libldp_hip.so -- C ABI of the MI355X-native LDP denoising hot path.
 *
 * The reference (amberxie88/latent_diffusion_planning) is pure Python on JAX/Flax; it has no
 * native layer and therefore no FFI of its own.  Each entry point below replaces one traced
 * JAX function of the reference's sampling path; a binding (ctypes, see
 * latent_diffusion_planning_amd/_lib.py and INTEGRATION.md) calls them with raw device
 * pointers.  No torch / C++ types cross this boundary.
 *
 * Conventions
 *   - every function returns 0 on success or a negative LDP_E* code; ldp_last_error() returns a
 *     thread-local message for the last failing call.  Nothing throws or exits across the ABI.
 *   - all tensors are contiguous float32 in device (HBM) memory unless marked "host";
 *     the caller owns them.  The handle owns weights, constant tables, workspaces and the
 *     hipGraphExec cache.
 *   - `stream` is a hipStream_t passed as void* (e.g. torch.cuda.current_stream().cuda_stream);
 *     all work is enqueued on it, nothing synchronises the device except ldp_finalize / destroy.
 *   - one handle per device; calls on one handle are not re-entrant.
 *   - layouts are the reference's channels-last ones: plans (B, T, D), images (N, H, W, 3).
 */
#ifndef LDP_HIP_H
#define LDP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: exactly the functions declared here are exported. */
#define LDP_API __attribute__((visibility("default")))

#define LDP_OK 0
#define LDP_EINVAL (-1)   /* bad argument / unsupported shape            */
#define LDP_ESTATE (-2)   /* call order (weights missing, not finalized) */
#define LDP_EHIP (-3)     /* a HIP runtime call failed                   */
#define LDP_ENOMEM (-4)
#define LDP_EKEY (-5)     /* unknown weight path / option name           */
#define LDP_EFAULT (-6)   /* results since the last ldp_poll_fault are invalid and must be recomputed: a split
                             work-group timed out on its peer (the handle switched to safe mode), or an operand
                             left the range of the two-fp16-plane convolutions (the handle switched them to
                             three bf16 planes, which have fp32's range) -- see the fault protocol below      */

#define LDP_SAMPLER_DDPM 0 /* FlaxDDPMScheduler.step semantics (reference) */
#define LDP_SAMPLER_DDIM 1 /* eta = 0, defined by this repo */
#define LDP_SAMPLER_DPMPP 2 /* DPM-Solver++(2M) on the clipped data prediction over a registered timestep table, defined by this repo
                             * ("solver sampler" below) */

#define LDP_MAX_LEVELS 4

/* Stream ids of the Philox4x32-10 noise source (counter word 3; "noise source primitives" below).  A draw is keyed by
 * (seed, global element index, step, stream id); no two kinds of draw share a stream id. */
#define LDP_PHILOX_STREAM_STEP 0u      /* scheduler noise of executed step i (planner / IDM / policy loops)          */
#define LDP_PHILOX_STREAM_INIT 1u      /* the initial state x_T / a_T of a loop                                      */
#define LDP_PHILOX_STREAM_LOSS_PLAN 7u /* add_noise of the planner / policy loss (get_metrics, update)               */
#define LDP_PHILOX_STREAM_LOSS_IDM 8u  /* add_noise of the IDM loss                                                  */
#define LDP_PHILOX_STREAM_VAE_EPS 9u   /* eps of the StableVAE posterior draw z = mean + std * eps (ldp_vae_posterior) */
#define LDP_PHILOX_STREAM_VAE_SAMPLE 10u /* the latents StableVAEModel.sample decodes (drawn through ldp_philox_normal)  */
#define LDP_PHILOX_STREAM_DATA 11u     /* the window indices of a training batch (ldp_data_draw / ldp_data_sample)   */
#define LDP_PHILOX_STREAM_CONSTRAIN 12u /* the noise of a repainted constraint at level j (ldp_plan_constrain, step = j)  */

/* Index of each scalar in the 11-float result of ldp_vae_metrics: the keys of StableVAEModel.loss
 * (model/stable_vae_model.py:42-53), in the reference's order. */
#define LDP_VAE_METRIC_IMG_MIN 0
#define LDP_VAE_METRIC_IMG_MAX 1
#define LDP_VAE_METRIC_IMG_MEAN 2
#define LDP_VAE_METRIC_IMG_STD 3
#define LDP_VAE_METRIC_LOSS 4
#define LDP_VAE_METRIC_LOSS_MSE 5
#define LDP_VAE_METRIC_LOSS_KL 6
#define LDP_VAE_METRIC_Z_MIN 7
#define LDP_VAE_METRIC_Z_MAX 8
#define LDP_VAE_METRIC_Z_MEAN 9
#define LDP_VAE_METRIC_Z_STD 10
#define LDP_VAE_N_METRICS 11

typedef struct ldp_handle ldp_handle;

/* Hyper-parameters fixed at construction (agent/ldp_agent.yaml:7-34,47-51 + the dims
 * LDPAgent.create derives, agent/ldp_agent.py:534-540). */
typedef struct ldp_config {
  int32_t obs_dim;            /* D: planner input_dim                                  */
  int32_t action_dim;         /* A                                                     */
  int32_t global_cond_dim;    /* obs_horizon * D (width of obs_cond)                   */
  int32_t pred_horizon;       /* T: planner sequence length, multiple of 2^(levels-1)  */
  int32_t action_horizon;     /* IDM rows per plan                                     */
  int32_t n_levels;           /* len(down_dims) (<= LDP_MAX_LEVELS)                    */
  int32_t down_dims[LDP_MAX_LEVELS];
  int32_t kernel_size;        /* 5                                                     */
  int32_t n_groups;           /* 8                                                     */
  int32_t step_embed_dim;     /* diffusion_step_embed_dim = 256                        */
  int32_t planner_train_steps;/* planner_n_diffusion_steps = 100                       */
  int32_t idm_train_steps;    /* idm_n_diffusion_steps = 100                           */
  int32_t idm_hidden;         /* 256                                                   */
  int32_t idm_blocks;         /* 3                                                     */
  int32_t idm_time_dim;       /* FourierFeatures output_size = 256                     */
  int32_t image_size;         /* 64 (StableVAE input H = W; 96 and 128 also built); 0 disables the VAE module */
  int32_t vae_latent_channels;/* 4                                                     */
  int32_t device;             /* HIP device ordinal                                    */
} ldp_config;

LDP_API const char* ldp_last_error(void);
LDP_API const char* ldp_version(void);

/* -- lifecycle ----------------------------------------------------------------------------
 * replaces: LDPAgent.create (agent/ldp_agent.py:516-672) for the inference-side state. */
LDP_API int ldp_create(const ldp_config* cfg, ldp_handle** out);
LDP_API int ldp_destroy(ldp_handle* h);

/* Upload one parameter leaf.  `path` = "<module>/<flax path>/<leaf>" with module in
 * {"planner","idm","vae","encoder0".."encoder3"}, e.g. "planner/ConditionalResidualBlock1D_3/Conv1dBlock_0/Conv_0/kernel"
 * or "encoder0/ResNetBlock_2/conv_proj/kernel" (the ResNet image encoders of DPAgent, below).
 * `host` is a host float32 array in the Flax layout (Conv (k,Cin,Cout); Dense (in,out)).
 * replaces: planner_state.params / idm_state.params / vae_params pytrees
 * (agent/ldp_agent.py:575,614,551; train_bc.py:210-240 load_snapshot). */
LDP_API int ldp_set_weight(ldp_handle* h, const char* path, const float* host, const int64_t* shape,
                   int32_t ndim);

/* Pack weights into the MFMA streaming layout and build the timestep-only tables
 * (time-MLP output, per-block FiLM time parts, IDM cond parts, scheduler coefficients).
 * `modules` is a bitmask: 1 planner, 2 idm, 4 vae, 8 the ResNet encoders (every slot encoder<i> that has leaves: its tree is
 * checked -- the first missing or mis-shaped leaf is named -- and its kernels are packed).  Synchronises `stream`. */
LDP_API int ldp_finalize(ldp_handle* h, int32_t modules, void* stream);

/* -- planner ------------------------------------------------------------------------------
 * eps = ConditionalUnet1D.apply(params, x, k, cond)   (networks/diffusion_nets_v2.py:113-169)
 * x (B,T,D), cond (B,global_cond_dim) -> eps (B,T,D).  Timestep: `k_dev` (B,) int32 device
 * array, or NULL to use the scalar `k` for every sample. */
LDP_API int ldp_unet_forward(ldp_handle* h, const float* x, const int32_t* k_dev, int32_t k,
                     const float* cond, float* eps, int32_t B, void* stream);

/* Test hook: ldp_unet_forward (same arguments, same contract, the same code: ldp_unet_forward IS this call without a tap) with what every
 * launch of the evaluation wrote copied out behind the launch (hipMemcpyAsync device-to-device on `stream`) into `taps`, and one row of
 * `table` per stage (LDP_UNET_TRACE_COLS int64 each; host memory, valid on return; -1 = does not apply):
 *   [0] offset into taps (floats)  [1] offset of the residual projection the launch also wrote  [2] B  [3] positions
 *   [4] stored channel stride  [5] real channels  [6] LDP_UNET_STAGE_*  [7] residual-block index  [8] level (positions = T >> level)
 *   [9] the stage whose output it read (xa)  [10] the skip it read behind it (xb)  [11] the stage its residual came from, [12] 1: that
 *   stage's residual projection, 0: its output
 *   [13..21] the plan exactly as handed to tconv_launch: mode, to, nwn, ks, cpi, res, mb, kws, split
 *   [22] cs: work-groups per GroupNorm group  [23] kw: work-groups the K loop is split over  [24] by_sample placement
 *   [25] split tile code (0: none; 16 / 17 / 32 / 33 / 34)  [26] column of the block's (scale|bias) slice in the FiLM tensors
 *   [27], [28] stored channels of xa / xb
 * Tensors are (B, positions, stride) row-major; the FiLM parts (B, 1, F).  Stages: the padded input state; the FiLM global part
 * Mish(cond) @ W[E:]; the FiLM time rows the call's timesteps select (an epilogue adds the two); per residual block its first half
 * (conv + GroupNorm + Mish + FiLM, and the 1x1 projection of the block's input where the widths differ) and its second half
 * (conv + GroupNorm + Mish + residual); the stride-2 convs; the transposed convs; the Conv1dBlock before the head; the 1x1 head (eps,
 * (B, T, D) unpadded: the tensor the call returns).
 * With taps == NULL the evaluation runs untapped and only *n_stages / *floats_needed are set (table may be NULL); they are set on every
 * call.  Not for captured graphs; the product paths never call it. */
#define LDP_UNET_TRACE_COLS 32
enum { LDP_UNET_STAGE_INPUT = 0, LDP_UNET_STAGE_FILM_G, LDP_UNET_STAGE_FILM_T, LDP_UNET_STAGE_RES1, LDP_UNET_STAGE_RES2, LDP_UNET_STAGE_DOWN,
       LDP_UNET_STAGE_UP, LDP_UNET_STAGE_FIN_BLOCK, LDP_UNET_STAGE_HEAD };
LDP_API int ldp_unet_trace(ldp_handle* h, const float* x, const int32_t* k_dev, int32_t k, const float* cond, float* eps, int32_t B,
                   float* taps, int64_t taps_floats, int64_t* table, int32_t table_rows, int32_t* n_stages, int64_t* floats_needed,
                   void* stream);

/* The planner fori_loop of sample_viz_step (agent/ldp_agent.py:459-476):
 *   x <- x_init (or N(0,I) from the Philox stream when x_init == NULL);
 *   for i in 0..n_steps-1: eps = unet(x, t_i, cond); x = scheduler.step(eps, t_i, x, z_i)
 * step_noise: (n_steps, B, T, D) explicit N(0,1) draws, row i used at executed step i
 * (parity mode), or NULL to draw z_i in-kernel from Philox4x32-10 keyed by
 * (seed, global element = (row_offset*T + local row)*32 + channel, step); row_offset = global
 * index of this call's first plan, so a plan's noise does not depend on how a batch is sharded.  sampler/n_steps: DDPM requires n_steps ==
 * planner_train_steps; DDIM requires n_steps | planner_train_steps.
 * use_graph != 0 replays a cached hipGraph of the whole loop (keyed by B, n_steps, sampler,
 * noise mode and the step range, here (0, n_steps): see ldp_plan_sample_range).  out: (B, T, D). */
LDP_API int ldp_plan_sample(ldp_handle* h, const float* cond, const float* x_init,
                    const float* step_noise, uint64_t seed, int64_t row_offset,
                    int32_t sampler, int32_t n_steps, float* out, int32_t B,
                    int32_t use_graph, void* stream);

/* -- inverse dynamics ---------------------------------------------------------------------
 * eps = MLPDiffusion.apply(params, s, a, k)   (networks/mlp_diffusion_nets.py:56-68)
 * s (R, 2D), a (R, A) -> eps (R, A). */
LDP_API int ldp_idm_forward(ldp_handle* h, const float* s, const float* a, const int32_t* k_dev,
                    int32_t k, float* eps, int32_t R, void* stream);

/* The IDM fori_loop (agent/ldp_agent.py:489-503; also :409-427, :368-386).
 * transition (R, 2D); a_init (R, A) or NULL; step_noise (n_steps, R, A) or NULL; out (R, A)
 * (still normalised; the caller applies unnormalize/clip, utils/data_utils.py:12-15,61-65).
 * row_offset = global index of this call's first row (any value; rows are keyed one by one). */
LDP_API int ldp_idm_sample(ldp_handle* h, const float* transition, const float* a_init,
                   const float* step_noise, uint64_t seed, int64_t row_offset,
                   int32_t sampler, int32_t n_steps, float* out, int32_t R,
                   int32_t use_graph, void* stream);

/* sample_viz_step without the image decode (agent/ldp_agent.py:452-505) as ONE call and, with
 * use_graph != 0, ONE captured hipGraph per (B, steps, sampler, noise modes):
 *   obs_cond = obs_emb[:, :obs_horizon].reshape(B, -1)                       (:459)
 *   x        = planner loop as in ldp_plan_sample                             (:461-476)
 *   plan     = concat(obs_emb[:, obs_horizon-1 : obs_horizon], x[:, :action_horizon])   (:478-479)
 *   s        = concat(plan[:, :-1], plan[:, 1:], -1) -> (B*action_horizon, 2D)           (:485-487)
 *   a        = IDM loop as in ldp_idm_sample on s                              (:488-503)
 *   action   = unnormalize(a) (utils/data_utils.py:12-15; act_mode 0) or clip (:61-65; act_mode 2)
 * obs_emb (B, obs_frames, D) normalised observation embeddings (get_obs_cond output), only the first
 * obs_horizon frames are read.  x_init (B,T,D) / x_noise (planner_steps,B,T,D) / a_init (B*ah,A) /
 * a_noise (idm_steps,B*ah,A): explicit-noise parity inputs or NULL for the Philox streams keyed by
 * (seed, row_offset + plan index).  Outputs: x_out (B,T,D) or NULL; plan_out (B, ah+1, D);
 * action_out (B*ah, A).  act_lo/act_hi: device bounds of length act_dim (1 or A), act_dim 0 = leave
 * the actions normalised. */
LDP_API int ldp_agent_sample(ldp_handle* h, const float* obs_emb, int32_t obs_frames, int32_t obs_horizon,
                     const float* x_init, const float* x_noise, const float* a_init,
                     const float* a_noise, uint64_t seed, int64_t row_offset, int32_t sampler,
                     int32_t planner_steps, int32_t idm_steps, float* x_out, float* plan_out,
                     float* action_out, const float* act_lo, const float* act_hi, int32_t act_dim,
                     int32_t act_mode, int32_t B, int32_t use_graph, void* stream);

/* DPVAEAgent.sample_step (agent/dp_repr_agent.py:169-201) as ONE call and, with use_graph != 0, ONE captured hipGraph per (B bucket,
 * n_steps, sampler, noise mode) -- the handle's planner module is the action U-Net (obs_dim = action_dim = A, global_cond_dim = obs_horizon * E):
 *   cond   = get_obs_cond: [img_0 .. img_{oh-1}, low_0 .. low_{oh-1}]  (:76-85; NOT the per-frame interleave of ldp_agent_sample)
 *   x      = the U-Net loop of ldp_plan_sample on (B, T, A) from x_init / N(0,I)  (:185-197)
 *   action = unnormalize(x[:, :action_horizon]) (act_mode 0) or clip (act_mode 2); act_dim 0 = leave it normalised  (:199-200)
 * obs_emb (B, obs_frames, E) per-frame [image latent (img_width floats) | low-dim (E - img_width)], only the first obs_horizon frames
 * are read; the gather into the condition layout is the call's first kernel (the captured loop is ldp_plan_sample's, under its key).
 * x_init (B,T,A) / x_noise (n_steps,B,T,A): explicit-noise parity inputs or NULL for the Philox streams keyed by (seed, row_offset + row).
 * action_out (B, action_horizon, A). */
LDP_API int ldp_policy_sample(ldp_handle* h, const float* obs_emb, int32_t obs_frames, int32_t obs_horizon, int32_t img_width,
                      const float* x_init, const float* x_noise, uint64_t seed, int64_t row_offset, int32_t sampler,
                      int32_t n_steps, float* action_out, const float* act_lo, const float* act_hi, int32_t act_dim,
                      int32_t act_mode, int32_t B, int32_t use_graph, void* stream);

/* -- best-of-N planning (defined by this repo; the reference draws one plan per observation) ----------------
 * B observations, N candidate plans each, K = T * D floats per candidate.  Rows are CANDIDATE-MAJOR everywhere below: global candidate
 * row r = c * B + b (candidate c of observation b), so a candidate range [c0, c0 + n_loc) is the contiguous row range
 * [c0 * B, (c0 + n_loc) * B) -- one rank's shard -- and with N = 1 row b is ldp_plan_sample's row b.  Lower cost is better.
 *
 * ldp_plan_candidates: the planner loop of ldp_plan_sample on the n_loc * B rows of candidates [c0, c0 + n_loc):
 *   cond[r] = obs_emb[r mod B, :obs_horizon].reshape(-1)        (one kernel, into handle memory; no tiled copy on the caller's side)
 *   x_out   = ldp_plan_sample(cond, x_init, step_noise, seed, row_offset = c0 * B, ...)   (that very call: its graph cache, range guard,
 *             fault protocol and batch split; the Philox stream of a candidate is keyed by its global row c * B + b)
 * obs_emb (B, obs_frames, D) as in ldp_agent_sample; x_init (n_loc * B, T, D) / step_noise (n_steps, n_loc * B, T, D): explicit-noise
 * parity inputs of THESE rows, or NULL; x_out (n_loc * B, T, D).  LDP_EINVAL: B < 1, c0 < 0, n_loc < 1, an obs_horizon that does not
 * match global_cond_dim. */
LDP_API int ldp_plan_candidates(ldp_handle* h, const float* obs_emb, int32_t obs_frames, int32_t obs_horizon, int32_t B, int32_t c0,
                                int32_t n_loc, const float* x_init, const float* step_noise, uint64_t seed, int32_t sampler,
                                int32_t n_steps, float* x_out, int32_t use_graph, void* stream);

/* score "density" (mode seeking): for the candidates i in [c0, c0 + n_loc) of every observation b
 *   cost_i = - sum_{j = 0 .. N-1} exp(-d2_ij / (2 h2)),  d2_ij = sum_k (x_ik - x_jk)^2,  h2 = bandwidth^2 * m_b,
 *   m_b = 2 * sum_k Var_k (biased variance over the N candidates) = the mean of d2 over all N^2 ordered pairs of observation b.
 * x_all (N * B, K): ALL candidates (every rank holds them); cost_out (n_loc * B): cost_out[(i - c0) * B + b].
 * m_b in float64 from all N candidates in a fixed order; d2 by direct differences in k order 0 .. K-1 (fp32 FMA chain; never
 * |x|^2 + |y|^2 - 2 x.y); the sum over j strictly in the order 0 .. N-1 in fp32.  No atomics, and nothing depends on c0 or n_loc: a
 * candidate's cost has the same bits whichever range (rank) computes it.  m_b = 0 (all candidates equal, N = 1): every cost is -N.
 * Stand-alone (no handle); two launches on `stream` and one stream-ordered allocation of B floats, nothing synchronises.
 * LDP_EINVAL, naming the argument: B < 1, N < 1, K < 1, c0 < 0, n_loc < 1, c0 + n_loc > N, bandwidth not finite or <= 0. */
LDP_API int ldp_plan_cost_density(const float* x_all, int32_t B, int32_t N, int32_t K, int32_t c0, int32_t n_loc, float bandwidth,
                                  float* cost_out, void* stream);

/* score "goal": cost[c * B + b] = sum_d weight[d] * (x[c * B + b, t_goal, d] - goal[b, d])^2 for the n candidates of this call
 * (x (n * B, T, D), any candidate range: a row's cost reads that row only), d in the order 0 .. D-1, fp32.  goal (B, D) normalised
 * embeddings, weight (D) non-negative (not checked: device memory), cost_out (n * B).  Stand-alone, one launch.
 * LDP_EINVAL: B, n, T, D < 1, t_goal outside 0 .. T-1. */
LDP_API int ldp_plan_cost_goal(const float* x, int32_t B, int32_t n, int32_t T, int32_t D, int32_t t_goal, const float* goal,
                               const float* weight, float* cost_out, void* stream);

/* The winner of every observation: best_index_out[b] = argmin_c cost_all[c * B + b] over c = 0 .. N-1, ties to the lowest c, a NaN
 * cost compared as +inf (all NaN / +inf: c = 0); best_cost_out[b] = that cost as stored; x_best_out[b] = x_all[best * B + b] (K floats,
 * a copy: the candidate's bits).  cost_all (N * B), x_all (N * B, K), best_index_out (B) int32, best_cost_out (B), x_best_out (B, K).
 * One work-group per observation, fixed comparison order.  Stand-alone, one launch.  LDP_EINVAL: B, N, K < 1. */
LDP_API int ldp_plan_select(const float* cost_all, const float* x_all, int32_t B, int32_t N, int32_t K, int32_t* best_index_out,
                            float* best_cost_out, float* x_best_out, void* stream);

/* -- warm-started replanning (defined by this repo; the reference starts every call from pure noise) ----------
 * Between two closed-loop calls the world moves by action_horizon states: the plan just computed, shifted by that many positions and
 * noised to an intermediate level, starts a loop that runs only the last k of n denoising steps (Janner et al. 2022, 5.4).
 *
 * ldp_plan_sample_range: ldp_plan_sample restricted to the executed steps [step_begin, step_end), 0 <= step_begin <= step_end <= n_steps.
 * Step i is the step i of the whole loop in every way (coefficients, timestep t_i = (n_steps-1-i) * stride, noise row i of step_noise
 * (n_steps, B, T, D), Philox key (seed, element, step i)), so ranges compose: (0, m) then (m, n) on its output gives ldp_plan_sample's
 * bits.  x_init == NULL draws x_T as ldp_plan_sample does; an empty range returns the drawn or given initial state.  A range has its own
 * captured graph (the key carries it).  ldp_plan_sample IS this call with (0, n_steps): the same batch split, range guard and fault
 * protocol.  LDP_EINVAL, naming the argument: step_begin outside 0 .. n_steps, step_end outside step_begin .. n_steps. */
LDP_API int ldp_plan_sample_range(ldp_handle* h, const float* cond, const float* x_init, const float* step_noise, uint64_t seed,
                                  int64_t row_offset, int32_t sampler, int32_t n_steps, int32_t step_begin, int32_t step_end,
                                  float* out, int32_t B, int32_t use_graph, void* stream);

/* The warm initial state, ONE launch (csrc/replan.hip plan_warm_init_kernel):
 *   xs[b, j, c]    = x_prev[src(b), min(j + shift, T-1), c]         (the edge is held: shift >= T gives the last state everywhere)
 *   x_out[b, j, c] = fma(a, xs, s * eps[b, j, c])                   (two fp32 roundings: the product s * eps, then the fused sum)
 * a = sqrt(abar_t), s = sqrt(1 - abar_t) at t = t_{step_begin} = (n_steps-1-step_begin) * (planner_train_steps / n_steps), computed on
 * the host in float64 from the float32 abar table (FlaxDDPMScheduler.add_noise's coefficients); eps = the LDP_PHILOX_STREAM_INIT draw of
 * ldp_plan_sample's x_T for the same (seed, row_offset): step 0, element ((row_offset + b) * T + j) * 32-padded width + c.
 * x_prev (n_slots, T, D); src(b) = slot[b], or b when slot == NULL (then B <= n_slots).  slot (B) int32 may live on the host or on the
 * device: a host table is checked (LDP_EINVAL names the entry outside 0 .. n_slots-1) and copied by the call; DEVICE-SIDE SLOT VALUES
 * ARE NOT CHECKED (an entry outside the table reads out of bounds).  x_out (B, T, D).  Exists for tests and tools: ldp_agent_resample
 * runs the same kernel straight into its loop state.  LDP_EINVAL: step_begin outside 0 .. n_steps-1, shift < 0, n_slots < 1. */
LDP_API int ldp_plan_warm_init(ldp_handle* h, const float* x_prev, const int32_t* slot, int32_t n_slots, int32_t shift, uint64_t seed,
                               int64_t row_offset, int32_t sampler, int32_t n_steps, int32_t step_begin, float* x_out, int32_t B,
                               void* stream);

/* ldp_agent_sample with two differences: the planner state comes from the warm-init kernel above (in the eager prologue, where
 * ldp_agent_sample draws x_T: the seed changes call to call), and the planner loop is [step_begin, planner_steps).  One captured graph
 * per (B bucket, steps, sampler, noise modes, step_begin); the IDM loop, the plan assembly and the action un-normalisation are
 * ldp_agent_sample's.
 * x_store (n_slots, T, D) device table: row slot[b] (row b with slot == NULL) is read as the previous plan, and the epilogue writes the
 * new full state x back to the same row (one launch; the padding columns of the loop state never reach the table).  Rows not named by
 * `slot` are untouched.  Slots must be distinct within a call (two rows writing one slot race).  slot: host or device, as above.
 * x_noise (planner_steps, B, T, D): row i is used at executed step i (rows below step_begin are not read); x_out (B, T, D) or NULL.
 * LDP_EINVAL: step_begin outside 0 .. planner_steps-1, shift < 0, n_slots < 1, a host slot outside the table. */
LDP_API int ldp_agent_resample(ldp_handle* h, const float* obs_emb, int32_t obs_frames, int32_t obs_horizon, float* x_store,
                               const int32_t* slot, int32_t n_slots, int32_t shift, int32_t step_begin, const float* x_noise,
                               const float* a_init, const float* a_noise, uint64_t seed, int64_t row_offset, int32_t sampler,
                               int32_t planner_steps, int32_t idm_steps, float* x_out, float* plan_out, float* action_out,
                               const float* act_lo, const float* act_hi, int32_t act_dim, int32_t act_mode, int32_t B,
                               int32_t use_graph, void* stream);

/* -- constrained planning (defined by this repo; the reference has nothing of the kind) -------------------------
 * A diffusion planner over states can be told where to be: after every denoising step the constrained entries of the trajectory are
 * overwritten with the known values at that step's noise level (inpainting: Janner et al. 2022 "Diffuser", Lugmayr et al. 2022
 * "RePaint").  One loop, the constraint met exactly: whole goal states, partial ones (some columns of one step), several waypoints.
 *
 * A loop of n executed steps has the levels 0 .. n: level j is the state in front of executed step j, level n the result.  Level j < n has
 * the timestep t_j = (n-1-j) * (planner_train_steps / n) and the coefficients a_j = sqrt(abar_t_j), s_j = sqrt(1 - abar_t_j), computed on
 * the host in float64 from the float32 abar table and cast to float32 (ldp_plan_warm_init's convention); level n has a = 1, s = 0.
 * target (B, T, D) float32, in the normalised embedding units of the plan itself (the scheduler clips its own x0 estimate to [-1, 1]:
 * targets belong there; the range is not checked); mask (B, T, D) uint8.  The constraint operation C_j replaces x[b, t, c] where
 * mask[b, t, c] != 0 and leaves every other element bit for bit as it was (a select, never a blend: a NaN in target under a zero mask
 * does not reach the state):
 *   LDP_CONSTRAIN_CLAMP    the replacement is target[b, t, c]                                             (Diffuser)
 *   LDP_CONSTRAIN_REPAINT  fma(a_j, target, s_j * z_j) with two fp32 roundings (the product s_j * z_j, then the fused sum);
 *                          z_j = the LDP_PHILOX_STREAM_CONSTRAIN draw for (seed, element ((row_offset + b) * T + t) * 32-padded width
 *                          + c, step j): the element index of the step noise, so a draw depends on the global row only.  At level n
 *                          the value written is target itself.
 * The constrained loop over the executed steps [begin, end):  x <- C_begin(x);  for i in begin .. end-1:  x <- C_{i+1}(step_i(x)).
 * step_i is ldp_plan_sample_range's step i; C_j is deterministic, so ranges compose bitwise and applying it twice is harmless.
 *
 * ldp_plan_constrain: C_level alone on caller memory, ONE launch (csrc/constrain.hip plan_constrain_kernel); x, x_out (B, T, D), x_out may
 * be x.  Exists for tests and tools: the loops below run the same kernel on their padded state, one launch behind every step, inside the
 * captured graph (seed and first row are read from the handle's control block there: a graph never bakes a seed).
 * LDP_EINVAL, naming the argument: a mode that is neither of the two, a NULL target or mask, a level outside 0 .. n_steps. */
#define LDP_CONSTRAIN_CLAMP 1
#define LDP_CONSTRAIN_REPAINT 2
LDP_API int ldp_plan_constrain(ldp_handle* h, const float* x, const float* target, const uint8_t* mask, int32_t mode, int32_t sampler,
                               int32_t n_steps, int32_t level, uint64_t seed, int64_t row_offset, float* x_out, int32_t B, void* stream);

/* ldp_plan_sample_range with the constraint: the constrained loop above over [step_begin, step_end); an empty range returns C_begin of
 * the drawn or given initial state.  target and mask are copied by the call into handle-owned padded buffers (graph nodes reference
 * handle memory only).  One captured graph per (B bucket, steps, sampler, noise mode, range, mode); an all-zero mask gives
 * ldp_plan_sample_range's bits.  (end - begin) + 1 launches more than the free loop.  A split batch hands each part its rows of target
 * and mask and its own row_offset. */
LDP_API int ldp_plan_sample_constrained(ldp_handle* h, const float* cond, const float* x_init, const float* step_noise, const float* target,
                                        const uint8_t* mask, int32_t mode, uint64_t seed, int64_t row_offset, int32_t sampler,
                                        int32_t n_steps, int32_t step_begin, int32_t step_end, float* out, int32_t B, int32_t use_graph,
                                        void* stream);

/* ldp_agent_sample whose planner loop is the constrained loop over (0, planner_steps): the plan assembly, the IDM loop and the action
 * un-normalisation are ldp_agent_sample's, on the constrained plan.  x_out, plan_out and action_out as there. */
LDP_API int ldp_agent_sample_constrained(ldp_handle* h, const float* obs_emb, int32_t obs_frames, int32_t obs_horizon, const float* x_init,
                                         const float* x_noise, const float* a_init, const float* a_noise, const float* target,
                                         const uint8_t* mask, int32_t mode, uint64_t seed, int64_t row_offset, int32_t sampler,
                                         int32_t planner_steps, int32_t idm_steps, float* x_out, float* plan_out, float* action_out,
                                         const float* act_lo, const float* act_hi, int32_t act_dim, int32_t act_mode, int32_t B,
                                         int32_t use_graph, void* stream);

/* -- solver sampler (defined by this repo; the reference has DDPM only) -----------------------------------------
 * LDP_SAMPLER_DPMPP is DPM-Solver++(2M) (Lu et al. 2022) on the clipped data prediction: a second-order multistep solver of the
 * probability-flow ODE that costs one U-Net evaluation per step, like DDIM, and pays off on a timestep grid uniform in log-SNR, which
 * t_i = (n-1-i) * stride cannot express.  The sampler therefore runs over a REGISTERED timestep table, one per step count.
 *
 * ldp_solver_timesteps: registers ts (n_steps int32 on the host; first executed step first) as the table sampler 2 uses whenever it is
 * called with this n_steps, and computes its coefficient rows (host, float64 from the float32 abar table, cast to float32), with
 * alpha = sqrt(abar), sigma = sqrt(1 - abar), lambda = 1/2 log(abar / (1 - abar)), row i the step from t = ts[i] to s = ts[i+1] and
 * h_i = lambda_s - lambda_t:
 *   inv_a = 1 / alpha_t,  sg = sigma_t,  c_x = sigma_s / sigma_t,  c_D = alpha_s - sigma_s alpha_t / sigma_t,  w = h_i / (2 h_{i-1})
 * The last row goes to the clean level (alpha_s = 1, sigma_s = 0: c_x = 0, c_D = 1); w = 0 in row 0 and in the last row.
 * LDP_EINVAL, naming the entry: n_steps outside 1 .. planner_train_steps, an entry outside 0 .. planner_train_steps-1, a table that is
 * not strictly decreasing, a last entry that is not 0.  Registering the same table again does nothing; a different table for an
 * n_steps that already has one replaces it and drops the captured graphs.
 *
 * The update of executed step i, ONE elementwise launch (csrc/compose.hip plan_compose_step_kernel<1, false, false>), each operation
 * rounded to fp32 once:
 *   x0     = clamp(fma(-sg, eps, x) * inv_a, -1, 1)             (the scheduler's clip_sample)
 *   Dv     = second ? fma(w, x0 - x0_prev, x0) : x0
 *   x_out  = fma(c_x, x, c_D * Dv);    x0_out = x0
 * ldp_plan_solver_step: that update on caller memory with row `step` of the table of n_steps; x, eps, x_out, x0_out (B, T, D), x0_prev
 * (B, T, D) or NULL; second = x0_prev != NULL && step < n_steps-1.  x_out may be x and x0_out may be x0_prev.  Exists for tests and
 * tools: the loop runs the same kernel on its own buffers.  LDP_ESTATE without a table for n_steps; LDP_EINVAL for a step outside
 * 0 .. n_steps-1.
 *
 * Under sampler 2, ldp_plan_sample / ldp_plan_sample_range (and through them ldp_plan_candidates), ldp_policy_sample and
 * ldp_agent_sample run, per executed step i of [begin, end): the U-Net at t = ts[i] writing eps only, then the solver launch, which
 * updates the loop state and the x0 history in place (one launch more per step than DDIM; no step noise is drawn
 * and step_noise is ignored, as for DDIM).  Step i is second order iff i > begin and i < n_steps-1.  EVERY CALL STARTS WITH AN EMPTY
 * HISTORY, so a range that starts at begin > 0 starts first order: under this sampler ranges do NOT compose bit for bit ((0, m) then
 * (m, n) differs from (0, n) in step m).  x_T is ldp_plan_sample's Philox draw, whatever the sampler.  ldp_agent_sample's IDM loop
 * then runs DDIM with idm_steps.  Without a table for n_steps these calls fail with LDP_ESTATE, naming ldp_solver_timesteps.
 * ldp_idm_sample, ldp_plan_warm_init, ldp_agent_resample, ldp_plan_constrain, ldp_plan_sample_constrained and
 * ldp_agent_sample_constrained refuse sampler 2 with LDP_EINVAL (not built: their level coefficients assume the uniform grid). */
LDP_API int ldp_solver_timesteps(ldp_handle* h, const int32_t* ts_host, int32_t n_steps);
LDP_API int ldp_plan_solver_step(ldp_handle* h, const float* x, const float* eps, const float* x0_prev, int32_t n_steps, int32_t step,
                                 float* x_out, float* x0_out, int32_t B, void* stream);

/* -- guided planning (defined by this repo; the reference has nothing of the kind) ------------------------------
 * The guided sampling of "Planning with Diffusion" (Janner et al. 2022, Alg. 1) with analytic costs: every denoising step moves the
 * clipped data prediction one projected gradient step down a cost, then takes the scheduler's own step from there.  The cost of sample b
 * on y (T, D), all weights >= 0:
 *   J_b(y) = 1/2 sum_{t,c} wg[b,t,c] (y[t,c] - target[b,t,c])^2                                             soft goals / waypoints
 *          + 1/2 sum_c lam[c] ( sum_{t=0..T-2} (y[t+1,c] - y[t,c])^2 + [anchor] (y[0,c] - anchor[b,c])^2 )   smoothness, continuity
 *          + 1/2 sum_{t,c} beta[c] ( max(y - hi[c], 0)^2 + max(lo[c] - y, 0)^2 )                             box bounds
 * g = grad_y J: elementwise plus a three-point stencil along T (row 0 has only its forward difference without an anchor).  Executed
 * step i of a guided loop, with row i of the scheduler's coefficients (DDPM or DDIM) and the step size rho[i]:
 *   y  = clip((x - sqrt(1 - abar_t) eps) / sqrt(abar_t), -1, 1);    y' = clip(y - rho[i] g(y), -1, 1)
 *   x <- c_x0 y' + c_x x + c_eps eps + sigma z
 * eps is used as the network wrote it; z is the fused step's draw (LDP_PHILOX_STREAM_STEP, step i, element (row_offset * T + r) * padded
 * width + c) or the explicit step noise, so with rho = 0 the guided loop is the free loop up to rounding.  Every operation is rounded to
 * fp32 once, in the order csrc/compose.hip states.  With L = max wg + 4 max lam + max beta, rho[i] L <= 1 guarantees J(y') <= J(y); the
 * library does not check this bound (guide.build_guide does).
 *
 * ldp_plan_guide_step: that step on caller memory, ONE launch (csrc/compose.hip plan_compose_step_kernel<0, true, false>: a work-group
 * owns whole samples, the stencil goes through LDS).  All pointers are device memory: x, x_out (B, T, ldx) with ldx >= D (x_out may be x; columns beyond D
 * are neither read nor written), eps and noise (B, T, D; noise NULL: the Philox draw of (seed, row_offset)), target, wg (B, T, ldg) and
 * anchor (B, ldg) or NULL with ldg >= D, lam, beta, lo, hi (D), rho (n_steps; entry `step` is read).  pred_horizon <= 16, obs_dim <= 128.
 * ldp_plan_guide_cost: out[r] = J of row r of x (rows, T, D) under guide row r / n_per (rows = B * n_per: n_per candidates per
 * observation), ONE launch, one wave per sample with a fixed summation order: bitwise the same whatever the batch.  target, wg
 * (B, T, D), anchor (B, D) or NULL.
 *
 * ldp_plan_sample_guided: ldp_plan_sample_range with the guided loop over [step_begin, step_end): per executed step the U-Net writing
 * eps only, then the guided step -- one launch more per step than the free loop; step i is the same step whatever the range, so ranges
 * compose bit for bit.  target, wg, anchor (NULL: no continuity term) are device memory, copied by the call into handle-owned padded
 * buffers; lam, beta, lo, hi (D) and rho (n_rho) are HOST arrays, checked and copied by the call.  One captured graph per (B bucket,
 * steps, sampler, noise mode, range, anchor or not); a graph bakes no value of the guide.  The free loops keep their graphs and launches.
 * ldp_agent_sample_guided: ldp_agent_sample whose planner loop is the guided loop over (0, planner_steps).
 * LDP_EINVAL, naming the argument: sampler 2 (not built), a NULL array, n_rho != n_steps, a negative or non-finite lam / beta / rho
 * entry, lo[c] > hi[c], ldx or ldg below D.  A guide together with a constraint or a warm start is not built. */
LDP_API int ldp_plan_guide_step(ldp_handle* h, const float* x, const float* eps, const float* noise, const float* target, const float* wg,
                                const float* anchor, const float* lam, const float* beta, const float* lo, const float* hi,
                                const float* rho, int32_t sampler, int32_t n_steps, int32_t step, uint64_t seed, int64_t row_offset,
                                float* x_out, int32_t ldx, int32_t ldg, int32_t B, void* stream);
LDP_API int ldp_plan_guide_cost(ldp_handle* h, const float* x, const float* target, const float* wg, const float* anchor, const float* lam,
                                const float* beta, const float* lo, const float* hi, int64_t rows, int32_t n_per, float* out, void* stream);
LDP_API int ldp_plan_sample_guided(ldp_handle* h, const float* cond, const float* x_init, const float* step_noise, const float* target,
                                   const float* wg, const float* anchor, const float* lam, const float* beta, const float* lo,
                                   const float* hi, const float* rho, int32_t n_rho, uint64_t seed, int64_t row_offset, int32_t sampler,
                                   int32_t n_steps, int32_t step_begin, int32_t step_end, float* out, int32_t B, int32_t use_graph,
                                   void* stream);
LDP_API int ldp_agent_sample_guided(ldp_handle* h, const float* obs_emb, int32_t obs_frames, int32_t obs_horizon, const float* x_init,
                                    const float* x_noise, const float* a_init, const float* a_noise, const float* target, const float* wg,
                                    const float* anchor, const float* lam, const float* beta, const float* lo, const float* hi,
                                    const float* rho, int32_t n_rho, uint64_t seed, int64_t row_offset, int32_t sampler,
                                    int32_t planner_steps, int32_t idm_steps, float* x_out, float* plan_out, float* action_out,
                                    const float* act_lo, const float* act_hi, int32_t act_dim, int32_t act_mode, int32_t B,
                                    int32_t use_graph, void* stream);

/* -- composed planning (defined by this repo; the reference has nothing of the kind) ----------------------------
 * A warm start, a constraint and a guide in ONE planner call, under any of the three samplers.  The calls above keep their refusals;
 * these take the optional parts in one struct.  A part is absent when its device arrays are NULL.
 *   warm start   x_store (n_slots, T, D), slot (B; host or device; NULL: rows 0 .. B-1), n_slots, shift      (ldp_agent_resample's)
 *   constraint   target (B, T, D) float32, mask (B, T, D) uint8, mode LDP_CONSTRAIN_*                        (ldp_plan_sample_constrained's)
 *   guide        g_target, g_wg (B, T, D), g_anchor (B, D) or NULL, lam, beta, lo, hi (D), rho (n_rho = n_steps)   (ldp_plan_sample_guided's)
 * The composed step i of n, ONE launch (csrc/compose.hip plan_compose_step_kernel), is the existing operations in sequence, every
 * operation rounded to fp32 once:
 *   1  y  = clip((x - s_i eps) / a_i, -1, 1)             the data prediction; (a_i, s_i) of the scheduler's row i (DDPM / DDIM) or of the
 *                                                        registered timestep table (sampler 2)
 *   2  y' = clip(y - rho[i] g(y), -1, 1)                 with a guide (g: ldp_plan_guide_step's gradient), else y' = y
 *   3  DDPM / DDIM:  x' = c_x0 y' + c_x x + c_eps eps + sigma z                      (z: the step noise of ldp_plan_sample)
 *      sampler 2:    Dv = second ? y' + w (y' - x0_prev) : y';  x' = c_x x + c_D Dv;  x0_out = y'
 *                    -- the history holds the GUIDED data prediction (the denoiser the loop actually follows)
 *   4  where mask != 0:  x' = C_{i+1}: target, or under LDP_CONSTRAIN_REPAINT below level n  a_{i+1} target + s_{i+1} z_c  with
 *      ldp_plan_constrain's draw z_c at level i + 1.  A select, never a blend; the history is not overwritten.
 * Constraint levels under sampler 2: level j < n has (sqrt(abar_ts[j]), sqrt(1 - abar_ts[j])) of the registered table (float64 from the
 * float32 abar table, cast once), level n exactly (1, 0).  The constraint is NOT imposed on y in front of the guide (the smoothness
 * stencil does not see the pinned goal): a possible follow-up.
 *
 * ldp_plan_compose_step: that step on caller memory.  EVERY pointer of `parts` is device memory here (as in ldp_plan_guide_step: lam,
 * beta, lo, hi, rho too), and its warm-start fields are not read.  x, x_out, x0_prev, x0_out (B, T, ldx) with ldx >= D (x_out may be x,
 * x0_out may be x0_prev; columns beyond D are neither read nor written), eps and noise (B, T, D; noise NULL: the Philox draw of (seed,
 * row_offset)), the guide's arrays with row stride ldg, the constraint's target and mask with row stride ldc.  Under sampler 2 x0_out is
 * required and the step is second order iff second != 0 (then x0_prev is required) and step < n_steps-1; under DDPM / DDIM second,
 * x0_prev and x0_out are ignored.
 *
 * ldp_plan_sample_composed: ldp_plan_sample_range with the parts.  In these two calls lam, beta, lo, hi, rho are HOST arrays (as in
 * ldp_plan_sample_guided); a warm start is read from x_store (not written back) and noised to the level of step_begin.  Where a guide
 * meets a constraint, or either meets sampler 2, the loop is the composed one: C_begin once in front, then per executed step the U-Net
 * writing eps only and one composed launch -- (end - begin) launches more than the free DDIM loop, plus 1 with a constraint.  Every
 * other combination runs the loop the dedicated call runs (bit-identical to it).  One captured graph per (B bucket, steps, sampler, noise
 * mode, range, mode, anchor or not, composed or not); a graph bakes nothing of a guide, a constraint or a seed.  Under DDPM / DDIM step
 * ranges compose bit for bit; UNDER SAMPLER 2 THE HISTORY STARTS EMPTY WITH EVERY CALL, so ranges do not compose there.
 * ldp_agent_sample_composed: ldp_agent_sample (no warm start: step_begin must be 0) / ldp_agent_resample (warm start: the planner loop
 * is [step_begin, planner_steps) and the new planner state is written back to the same rows of x_store) with the parts; the IDM loop,
 * the plan assembly and the action un-normalisation are theirs.
 * LDP_EINVAL, naming the argument: whatever the dedicated calls refuse for their part (a negative or non-finite lam / beta / rho entry,
 * lo[c] > hi[c], n_rho != n_steps, a bad mode, a NULL array of a part that is present, a host slot outside the table, x_init together
 * with a warm start); LDP_ESTATE under sampler 2 without a registered table for n_steps. */
typedef struct ldp_plan_compose {
  float* x_store; const int32_t* slot; int32_t n_slots, shift;                                        /* warm start */
  const float* target; const uint8_t* mask; int32_t mode;                                             /* constraint */
  const float* g_target; const float* g_wg; const float* g_anchor;                                    /* guide */
  const float* lam; const float* beta; const float* lo; const float* hi; const float* rho; int32_t n_rho;
} ldp_plan_compose;
LDP_API int ldp_plan_compose_step(ldp_handle* h, const float* x, const float* eps, const float* noise, const float* x0_prev,
                                  const ldp_plan_compose* parts, int32_t sampler, int32_t n_steps, int32_t step, int32_t second,
                                  uint64_t seed, int64_t row_offset, float* x_out, float* x0_out, int32_t ldx, int32_t ldg, int32_t ldc,
                                  int32_t B, void* stream);
LDP_API int ldp_plan_sample_composed(ldp_handle* h, const float* cond, const float* x_init, const float* step_noise,
                                     const ldp_plan_compose* parts, uint64_t seed, int64_t row_offset, int32_t sampler, int32_t n_steps,
                                     int32_t step_begin, int32_t step_end, float* out, int32_t B, int32_t use_graph, void* stream);
LDP_API int ldp_agent_sample_composed(ldp_handle* h, const float* obs_emb, int32_t obs_frames, int32_t obs_horizon, const float* x_init,
                                      const float* x_noise, const float* a_init, const float* a_noise, const ldp_plan_compose* parts,
                                      int32_t step_begin, uint64_t seed, int64_t row_offset, int32_t sampler, int32_t planner_steps,
                                      int32_t idm_steps, float* x_out, float* plan_out, float* action_out, const float* act_lo,
                                      const float* act_hi, int32_t act_dim, int32_t act_mode, int32_t B, int32_t use_graph, void* stream);

/* -- StableVAE ----------------------------------------------------------------------------
 * FlaxAutoencoderKL.encode(x).latent_dist.mean   (call site agent/ldp_agent.py:55-60)
 * img (N, S, S, 3) NHWC already normalised to [-1,1] -> mean (N, S/32, S/32, latent_channels)
 * NHWC, i.e. the (h, w, c) flattening order the agent reshapes to (B, H, 16). */
LDP_API int ldp_vae_encode(ldp_handle* h, const float* img_nhwc, float* mean_out, int32_t N,
                   void* stream);

/* FlaxAutoencoderKL.decode(z).sample   (call site agent/ldp_agent.py:81-84; "next" row 8f-1)
 * z (N, S/32, S/32, latent_channels) NHWC, already un-normalised -> image (N, 3, S, S) NCHW.
 * Needs the decoder weights (vae/post_quant_conv, vae/decoder/...) to have been finalized. */
LDP_API int ldp_vae_decode(ldp_handle* h, const float* z_nhwc, float* img_nchw_out, int32_t N, void* stream);

/* FlaxAutoencoderKL.encode(x).latent_dist.parameters   (model/stable_vae_model.py:29; diffusers
 * FlaxDiagonalGaussianDistribution.__init__: `mean, logvar = jnp.split(parameters, 2, axis=-1)`)
 * The encoder exactly as ldp_vae_encode runs it, keeping every quant_conv channel:
 * moments_out (N, S/32, S/32, 2 * latent_channels) NHWC, channels [0, LC) the mean -- bitwise what ldp_vae_encode
 * returns -- and [LC, 2 LC) the (unclamped) log-variance. */
LDP_API int ldp_vae_moments(ldp_handle* h, const float* img_nhwc, float* moments_out, int32_t N, void* stream);

/* FlaxDiagonalGaussianDistribution.sample / .kl on N images' moments (model/stable_vae_model.py:31,38), one fused kernel:
 *   logvar <- clip(logvar, -30, 20);  std = exp(0.5 logvar);  var = exp(logvar)
 *   z_out (N, hl, hl, LC) = mean + std * eps;   kl_out[n] = 0.5 * sum_{h,w,c}(mean^2 + var - 1 - logvar)
 *   stats_out[0..3] = min, max, mean, population std of z (may be NULL);  std_out as z_out (may be NULL)
 * eps (N, hl, hl, LC): explicit noise, or NULL for the Philox stream LDP_PHILOX_STREAM_VAE_EPS keyed by
 * (seed, element (row_offset + n) * hl * hl * LC + e, step 0): a shard draws what the unsharded batch draws, and an eps buffer
 * filled by ldp_philox_normal with the same key gives the same bits.  hl = image_size / 32 and LC come from the handle's config;
 * no weights are needed.  Every reduction has a fixed order (no atomics): two runs give the same bits. */
LDP_API int ldp_vae_posterior(ldp_handle* h, const float* moments, const float* eps, uint64_t seed, int64_t row_offset,
                      float* z_out, float* std_out, float* kl_out, float* stats_out, int32_t N, void* stream);

/* Test hook: ONE chunk (N <= 256) of the encoder (decode == 0: in = frames (N, S, S, 3), out = moments exactly as ldp_vae_moments) or of the
 * decoder (decode != 0: in = z, out = image exactly as ldp_vae_decode) through the same code as those calls, with every stage's output
 * tensor copied out behind the stage (hipMemcpyAsync device-to-device on `stream`) into `taps`, and one row of `table` per stage
 * (LDP_VAE_TRACE_COLS int64 each; host memory, valid on return):
 *   [0] offset into taps (floats)  [1] N  [2] H  [3] W  [4] stored channel stride  [5] real channels  [6] LDP_VAE_STAGE_*
 *   [7], [8] the stage(s) whose output it read (-1: the call's input / none)  [9] LDP_VAE_FAM_* of its convolution
 *   [10..12] (nwn, ks, cpi) of a tconv tile  [13] LDP_VAE_STATS_* of its GroupNorm  [14] 1: its conv left column sums for the next GroupNorm
 *   [15] 1: the tensor is (N, C, H, W), 0: (N, H, W, stride)
 * Stages -- encoder: conv_in; per ResnetBlock2D conv1(swish(norm1 x)), the 1x1 shortcut where present, conv2(swish(norm2 h)) + skip; each
 * Downsample2D; the attention block; conv_norm_out + conv_out; quant_conv.  Decoder: post_quant_conv (into the 64-channel padded tensor),
 * conv_in, the same block stages, upsample + conv (preceded by an auxiliary row LDP_VAE_STAGE_UPSAMPLED: the replicated tensor the conv
 * read), conv_norm_out + conv_out, the NCHW transpose.
 * With taps == NULL the chunk runs untapped and only *n_stages / *floats_needed are set (table may be NULL); they are set on every call.
 * Not for captured graphs; the product paths never call it. */
#define LDP_VAE_TRACE_COLS 16
enum { LDP_VAE_STAGE_CONV_IN = 0, LDP_VAE_STAGE_RES1, LDP_VAE_STAGE_SHORTCUT, LDP_VAE_STAGE_RES2, LDP_VAE_STAGE_DOWN, LDP_VAE_STAGE_ATTN,
       LDP_VAE_STAGE_CONV_OUT, LDP_VAE_STAGE_QUANT, LDP_VAE_STAGE_POST_QUANT, LDP_VAE_STAGE_UP, LDP_VAE_STAGE_NCHW, LDP_VAE_STAGE_UPSAMPLED };
/* none (VALU kernels) / exact-fp32 tconv tile / sconv3 on three bf16 planes, six products / sconv3 on two fp16 planes, three products /
 * tconv tile on two fp16 planes, three products */
enum { LDP_VAE_FAM_NONE = 0, LDP_VAE_FAM_TCONV_F32, LDP_VAE_FAM_SCONV_BF16X6, LDP_VAE_FAM_SCONV_F16X3, LDP_VAE_FAM_TCONV_F16X3 };
/* no GroupNorm / column sums of the producing 3x3 conv / row sums of conv_in / gn_part + gn_final */
enum { LDP_VAE_STATS_NONE = 0, LDP_VAE_STATS_CONV, LDP_VAE_STATS_CONV_IN, LDP_VAE_STATS_GN_PART };
LDP_API int ldp_vae_trace(ldp_handle* h, int32_t decode, const float* in, float* out, int32_t N, float* taps, int64_t taps_floats,
                  int64_t* table, int32_t table_rows, int32_t* n_stages, int64_t* floats_needed, void* stream);

/* StableVAEModel.loss, forward only (model/stable_vae_model.py:25-55; get_metrics_step :78-87 after postprocess_batch):
 *   moments -> posterior draw -> decode -> mse = mean((img - pred_img)^2), kl = mean_n kl[n] (exactly 0 when use_kl == 0),
 *   loss = mse + beta * kl (== mse when use_kl == 0), and min / max / mean / population std of img and of z.
 * img (N, S, S, 3) NHWC normalised to [-1, 1]; metrics_out: LDP_VAE_N_METRICS device floats in LDP_VAE_METRIC_* order, valid in
 * stream order (the caller reads them once).  eps / seed / row_offset as ldp_vae_posterior.  z_out (N, hl, hl, LC) NHWC and
 * rec_out (N, 3, S, S) NCHW receive the draw and the reconstruction when not NULL.  Runs in chunks of 256 images like
 * ldp_vae_encode / ldp_vae_decode; the loss reads the caller's frames in place (NHWC) against the decoder's NCHW output, and the
 * per-block partial results of all chunks are merged in a fixed order by one final kernel (centred variances, float64, no atomics).
 * Needs encoder and decoder weights; behind the fault check and the fp16-plane range guard like the two calls above. */
LDP_API int ldp_vae_metrics(ldp_handle* h, const float* img_nhwc, int32_t N, int32_t use_kl, float beta, const float* eps,
                    uint64_t seed, int64_t row_offset, float* metrics_out, float* z_out, float* rec_out, void* stream);

/* -- ResNet-18 image encoder of the diffusion-policy baseline (agent/dp_agent.py) -----------------
 * ResNetEncoder.apply (networks/resnet_v1.py:237-346, agent/encoder/bridge_resnet.yaml):
 * img (N, 64, 64, 3) NHWC in [-1, 1] -> feat_out (N, 1024) = [expected_x (512) | expected_y (512)]
 * conv_init 7x7 stride 2 -> GroupNorm(4, eps 1e-5) + ReLU -> max-pool 3x3 stride 2 (SAME, -inf padding) -> eight ResNetBlocks
 * (64 / 128 / 256 / 512 channels at 16 / 8 / 4 / 2 pixels; the first block of stages 1..3 has stride 2 and the conv_proj / norm_proj
 * residual) -> SpatialSoftmax (temperature 1).  No bias anywhere; every product is exact fp32 (fp32 MFMA).
 * `slot` 0..3 selects the weight module "encoder<slot>" (ldp_set_weight + ldp_finalize(h, 8)): one handle serves up to four cameras.
 * Works in chunks of 64 frames (the handle owns the ping-pong buffers: 44 MB), enqueues 39 launches per chunk on `stream` and does not
 * synchronise.  No atomics: two runs give the same bits, and a frame's features do not depend on N or on the frame's place in the call.
 * LDP_ESTATE before ldp_finalize(h, 8) of that slot; LDP_EINVAL for a bad slot or N <= 0. */
LDP_API int ldp_resnet_encode(ldp_handle* h, int32_t slot, const float* img_nhwc, float* feat_out,
                              int32_t N, void* stream);

/* Unit-testable primitives of the encoder (no handle): host weights in Flax layout, device tensors NHWC; each synchronises `stream`.
 * conv7x7_s2: conv_init -- 7x7, stride 2, padding (3, 3), cross-correlation; kernel (7, 7, Cin, Cout).  Built for H = W = 64, Cin = 3,
 *             Cout = 64 (LDP_EINVAL otherwise): x (N, 64, 64, 3) -> y (N, 32, 32, 64).
 * conv1x1_s2: conv_proj -- y(n, i, j, :) = x(n, 2i, 2j, :) @ kernel (1, 1, Cin, Cout); even H, W; Cin % 4 == 0, Cin <= 512, Cout % 64 == 0.
 * maxpool3x3_s2: nn.max_pool(x, (3, 3), (2, 2), 'SAME') on even H, W (padding (0, 1), -inf); C % 4 == 0.
 * gn: y = [relu]( GroupNorm(x) [+ res | + GroupNorm'(res)] ) on (N, HW, C): `groups` groups of C / groups channels (a multiple of 4),
 *     statistics per sample over (HW, C / groups), two passes (centred variance); res (device, same shape) or NULL; scale2 / bias2 (host,
 *     both or neither): `res` is then the RAW projection output and is normalised with its own statistics first (the fused norm_proj).
 *     y may alias x.
 * spatial_softmax: x (N, H, W, C) -> out (N, 2 C) = [sum_p pos_x(p) softmax_p(x) | sum_p pos_y(p) softmax_p(x)], pos_x = linspace(-1, 1, W)
 *     by column, pos_y = linspace(-1, 1, H) by row. */
LDP_API int ldp_resnet_conv7x7_s2_f32(const float* x, const float* kernel_host, float* y, int32_t N, int32_t H, int32_t W, int32_t Cin,
                                      int32_t Cout, void* stream);
LDP_API int ldp_resnet_conv1x1_s2_f32(const float* x, const float* kernel_host, float* y, int32_t N, int32_t H, int32_t W, int32_t Cin,
                                      int32_t Cout, void* stream);
LDP_API int ldp_resnet_maxpool3x3_s2_f32(const float* x, float* y, int32_t N, int32_t H, int32_t W, int32_t C, void* stream);
LDP_API int ldp_resnet_gn_f32(const float* x, const float* res, float* y, const float* scale_host, const float* bias_host,
                              const float* scale2_host, const float* bias2_host, int32_t N, int32_t HW, int32_t C, int32_t groups,
                              float eps, int32_t relu, void* stream);
LDP_API int ldp_resnet_spatial_softmax_f32(const float* x, float* out, int32_t N, int32_t H, int32_t W, int32_t C, void* stream);

/* -- elementwise pre/post-processing (utils/data_utils.py:9-16,61-65) ----------------------
 * y = (x - lo) / (hi - lo) * 2 - 1            (normalize != 0)
 * y = clip((x + 1) / 2 * (hi - lo) + lo, lo, hi)   (normalize == 0)
 * y = clip(x, lo, hi)                               (normalize == 2; the clip_min/clip_max entries)
 * lo/hi: device arrays of length `dim` broadcast over the trailing axis (dim == 1: scalar). */
LDP_API int ldp_normalize_bounds(const float* x, float* y, int64_t n, const float* lo, const float* hi,
                         int32_t dim, int32_t normalize, void* stream);

/* mean((a - b)^2) over n elements -> out[0] (device scalar): the `plan_mse` metric of
 * agent/ldp_agent.py:447-448,497-499 (a = sampled latents x_0, b = the batch's future latents).
 * One work-group, fixed summation order (bit-reproducible). */
LDP_API int ldp_mean_sq_diff(const float* a, const float* b, int64_t n, float* out, void* stream);

/* -- forward-only loss metrics (agent/ldp_agent.py:113-180, get_metrics_step :328-349) --------
 * noisy = FlaxDDPMScheduler.add_noise(x0, noise, t): out[r] = sqrt(abar[t[r]]) * x0[r] + sqrt(1 - abar[t[r]]) * noise[r]
 * (call sites agent/ldp_agent.py:119,136); x0 / noise / out (rows, width), t_dev (rows) int32 in [0, n_train);
 * abar = the float32 cumprod table of the squaredcos_cap_v2 schedule with n_train (<= 256) steps. */
LDP_API int ldp_add_noise(const float* x0, const float* noise, const int32_t* t_dev, int32_t n_train,
                  float* out, int64_t rows, int32_t width, void* stream);

/* out4[0..3] = min, max, mean, population std of n floats (the emb_* / action_* / <key>_min/_max
 * scalars of agent/ldp_agent.py:163-178: jnp.min / max / mean / std).  One work-group, fixed order. */
LDP_API int ldp_reduce_stats(const float* x, int64_t n, float* out4, void* stream);

/* -- training step (agent/ldp_agent.py:113-180 losses, :223-272 update / update_step, :274-323 update_mixed) ------------------------
 * The reference's step is `grads = jax.grad(loss)(params)`, `g_norm = optax.global_norm(grads)`, one `TrainState.apply_gradients` per
 * network with tx = optax.adam(warmup_cosine_decay_schedule) (:583-596, :621-634).  Here the handle keeps, per module (1 planner, 2 idm, 4 vae),
 * fp32 master parameters, gradients and the two Adam moments as flat arenas in the reference's Flax leaf layouts; every GEMM-shaped
 * piece of the forward and backward pass (Dense, k = 5 / stride-2 / transposed / 1x1 convolutions, dgrad and wgrad) runs on the exact-fp32
 * MFMA (csrc/train.hip).  Timesteps and noise are inputs (the reference draws them from its JAX key inside the traced step); the caller
 * evaluates the learning-rate schedule (optax evaluates it on the host-visible step count too).
 *
 * ldp_train_init: TrainStateEMA.create(params = the leaves last given with ldp_set_weight, tx = adam) -- moments zero, step 0; a module
 *                 whose EMA is enabled (ldp_train_ema) has it re-seeded from the parameters.
 *                 Synchronises the device.  Call again after ldp_set_weight to restart from other parameters.
 * Streams: ldp_train_planner_grad and ldp_train_idm_grad write disjoint state (one workspace lane per module) and may be enqueued on two
 * different streams so that the two tapes overlap; each also forks its weight-gradient GEMMs to an internal side stream and joins it before
 * it returns to `stream`'s order.  Whatever reads a gradient (grad_norm, apply, arena, read) must be ordered after both (the caller's join). */
LDP_API int ldp_train_init(ldp_handle* h, int32_t modules, void* stream);

/* alpha * plan_loss (agent/ldp_agent.py:113-127, 146) and its gradient w.r.t. every planner leaf:
 *   noisy = add_noise(x0, noise, t); pred = ConditionalUnet1D(noisy, t, cond); loss = alpha * mean((pred - noise)^2)
 * x0 / noise (B, T, D) = obs_emb[:, obs_horizon:] and the N(0,1) draw; t_dev (B) int32 in [0, planner_train_steps); cond (B, global_cond_dim);
 * loss_out: device scalar.  The gradients replace the module's gradient arena. */
LDP_API int ldp_train_planner_grad(ldp_handle* h, const float* x0, const float* noise, const int32_t* t_dev, const float* cond,
                                   float alpha, float* loss_out, int32_t B, void* stream);

/* ldp_train_planner_grad plus d loss / d cond: dcond_out (B, global_cond_dim), device, receives the gradient w.r.t. the condition -- what
 * the diffusion policy's image encoders are trained with (agent/dp_agent.py:87-110: obs_cond is a function of the encoder parameters).
 * The launches are those of ldp_train_planner_grad plus one copy inside the tape: loss and gradient arena are bitwise the same.
 * LDP_EINVAL on a handle with global_cond_dim = 0. */
LDP_API int ldp_train_planner_grad_cond(ldp_handle* h, const float* x0, const float* noise, const int32_t* t_dev, const float* cond,
                                        float alpha, float* loss_out, float* dcond_out, int32_t B, void* stream);

/* The ResNet-18 image encoders as training modules: bit 8 << slot (slot 0..3 = weight module "encoder<slot>") is accepted by
 * ldp_train_init / _apply / _ema / _step_count / _read / _write / _arena / _grad_norm / _publish(_ema) like bits 1, 2 and 4.
 * ldp_train_init(h, 8 << slot) before the slot has its 60 leaves: LDP_ESTATE.  Publishing repacks that slot's sampling weights, as
 * ldp_finalize(h, 8) does.  conv_init/kernel lies in the arena as [160][64] (K = 7 * 7 * 3 = 147 padded with 13 zero rows).
 *
 * ldp_train_encoder_forward: ResNetEncoder.apply (see ldp_resnet_encode) on the slot's MASTER parameters with every activation kept:
 *   img (N, 64, 64, 3) NHWC in [-1, 1] -> feat_out (N, 1024), both on the device.  1 <= N <= 1024 per call (LDP_EINVAL otherwise, with
 *   the limit in the message).  Each slot has its own tape workspace (about 4 MB per frame), so the tapes of several slots are alive at once.
 * ldp_train_encoder_backward: the VJP of the slot's last forward: the gradients of <dfeat, features> w.r.t. all 60 leaves REPLACE the
 *   slot's gradient arena (padding written as zeros).  dfeat (N, 1024) on the device, N that of the forward; LDP_ESTATE without a
 *   matching forward (none yet, another N, or ldp_train_init of the slot since).
 * Exact fp32 products (csrc/resnet_train.hpp); no atomics: the same state and batch give the same arena bit for bit; rows are padded
 * to 32 with zero frames, which contribute exactly zero.  Neither call synchronises. */
LDP_API int ldp_train_encoder_forward(ldp_handle* h, int32_t slot, const float* img_nhwc, float* feat_out, int32_t N, void* stream);
LDP_API int ldp_train_encoder_backward(ldp_handle* h, int32_t slot, const float* dfeat, int32_t N, void* stream);

/* alpha * idm_loss (agent/ldp_agent.py:129-140, 154) and its gradient: s (R, 2D) = s_sprime rows, a0 / noise (R, A), t_dev (R). */
LDP_API int ldp_train_idm_grad(ldp_handle* h, const float* s, const float* a0, const float* noise, const int32_t* t_dev, float alpha,
                               float* loss_out, int32_t R, void* stream);

/* StableVAEModel.loss (model/stable_vae_model.py:25-55, 57-73) and its gradient w.r.t. every leaf of module 4 (vae; ldp_train_init(h, 4)):
 *   moments = encoder(img); z = mean + exp(clip(logvar, -30, 20) / 2) eps; rec = decoder(z); loss = mse(img, rec) + beta mean(kl) (use_kl)
 * on the module's master parameters, exact fp32 forward with saved activations, hand-written backward (csrc/vae_train.hpp).  The gradients
 * replace module 4's gradient arena; metrics_out receives the LDP_VAE_N_METRICS scalars in LDP_VAE_METRIC_* order as device floats.
 * img (N, S, S, 3) NHWC normalised to [-1, 1]; eps / seed / row_offset as ldp_vae_metrics (explicit (N, S/32, S/32, LC) noise, or Philox
 * stream LDP_PHILOX_STREAM_VAE_EPS element (row_offset + n) * (S/32)^2 * LC + e).  64-pixel frames, 1 <= N <= 256 per call (LDP_EINVAL
 * otherwise, with the limit in the message); no atomics: the same state and batch give the same gradients bit for bit.
 * Module bit 4 also takes part in ldp_train_apply / _ema / _step_count / _read / _write / _arena / _publish(_ema) (which rebuild the
 * VAE's sampling weights) / _grad_norm; a handle created with image_size = 0 refuses it with LDP_EINVAL. */
LDP_API int ldp_train_vae_grad(ldp_handle* h, const float* img_nhwc, int32_t N, int32_t use_kl, float beta, const float* eps, uint64_t seed,
                               int64_t row_offset, float* metrics_out, void* stream);

/* The gradient of PART of a batch: what chunked and data-parallel VAE training are built from.  The call differentiates the mean loss over
 * n_total frames restricted to these N of them, i.e. (N / n_total) * grad loss(these N frames), so that the parts of a batch sum to the
 * gradient of the whole batch: G(batch) = sum_c G(part c).  n_total enters at the two places where the batch size enters the backward pass
 * (d rec = 2 (rec - img) / (n_total 3 S^2), and the beta ... / n_total terms of the posterior's backward), exactly where ldp_train_vae_grad
 * uses N: there is no scaling pass over the arena, and n_total = N gives ldp_train_vae_grad's bits.
 *   accumulate = 0: the gradients REPLACE module 4's gradient arena (ldp_train_vae_grad is this call with n_total = N, accumulate = 0).
 *   accumulate = 1: they are ADDED to it element by element, old value first: the tape writes a second arena, and after its side streams
 *     have joined one launch adds that to the gradient arena.  Every leaf takes part (the deferred column sums, the GroupNorm parameters,
 *     the exact-zero key/bias); the arena's padding stays zero, and the zero frames that pad a part to 32 rows add exactly zero.  One
 *     owner and one add per element, no atomics: the same calls in the same order give the same arena bit for bit.  The second arena
 *     (the size of the gradient arena) is allocated by the first accumulate = 1 call; a process that never accumulates never has it.
 * metrics_out receives the LDP_VAE_N_METRICS scalars of THESE N frames alone; the caller merges the parts' (StableVAEModel's
 * merge_vae_metrics).  row_offset: the global index of the part's first frame, as in ldp_train_vae_grad (a frame's Philox eps does not
 * depend on how the batch is cut).  LDP_EINVAL, with the limit in the message, for N < 1, N > 256, n_total < N, accumulate not 0 or 1,
 * and everything ldp_train_vae_grad refuses (frames that are not 64 pixels among it).  Does not synchronise. */
LDP_API int ldp_train_vae_grad_part(ldp_handle* h, const float* img_nhwc, int32_t N, int32_t n_total, int32_t accumulate, int32_t use_kl,
                                    float beta, const float* eps, uint64_t seed, int64_t row_offset, float* metrics_out, void* stream);

/* optax.global_norm over the gradient arenas of the listed modules (agent/ldp_agent.py:253) -> out[0] (device scalar).  Two-stage
 * reduction in a fixed order (bit-reproducible).  Called AFTER ldp_train_apply of the same gradients it costs one small launch: the optimiser
 * kernel leaves the per-stripe sums of squares behind (same stripes, same order: the same bits as the stand-alone first stage). */
LDP_API int ldp_train_grad_norm(ldp_handle* h, int32_t modules, float* out, void* stream);

/* One TrainState.apply_gradients with tx = optax.adam(lr): mu = (1 - b1) g + b1 mu; nu = (1 - b2) g^2 + b2 nu; count += 1;
 * p += -lr * (mu / (1 - b1^count)) / (sqrt(nu / (1 - b2^count)) + eps)   (optax 0.2.2 scale_by_adam, eps_root = 0; one launch over the arena).
 * lr = schedule(count before the increment), evaluated by the caller.  b1 / b2 / eps are doubles, as optax receives them: 1 - b and
 * 1 - b^count are formed in double and rounded to float32 once (1 - (float)0.999 is 1.3e-5 short of (float)0.001). */
LDP_API int ldp_train_apply(ldp_handle* h, int32_t module, float lr, double b1, double b2, double eps, void* stream);

/* TrainStateEMA(ema_decay = decay, ema_params = params) (agent/dp_repr_agent.py:290-296): allocates the module's EMA arena and copies the
 * current parameters into it.  From then on every ldp_train_apply of the module also writes
 *   ema = ema * decay + p_new * (1 - decay)        (TrainStateEMA.apply_ema, utils/flax_utils.py:22-27; :155)
 * in the same launch (decay and 1 - decay each rounded to float32 once, 1 - decay formed in double), and ldp_train_init re-seeds it from
 * the parameters.  Synchronises `stream`. */
LDP_API int ldp_train_ema(ldp_handle* h, int32_t module, double decay, void* stream);

/* TrainState.step of a module: *out = the count (number of ldp_train_apply calls since init); set_to >= 0 overwrites it first (checkpoint
 * restore). */
LDP_API int ldp_train_step_count(ldp_handle* h, int32_t module, int64_t set_to, int64_t* out);

/* One leaf of a module's state, Flax layout, host float32: which = 0 parameters, 1 gradients, 2 Adam mu, 3 Adam nu, 4 EMA of the
 * parameters (after ldp_train_ema).  `path` is the Flax path
 * inside the module ("ConditionalResidualBlock1D_3/Conv1dBlock_0/Conv_0/kernel").  Both synchronise `stream`.
 * replaces: reading / restoring planner_state / idm_state (params, opt_state) in train_bc.py:203-240. */
LDP_API int ldp_train_read(ldp_handle* h, int32_t module, int32_t which, const char* path, float* host_out, int64_t numel, void* stream);
LDP_API int ldp_train_write(ldp_handle* h, int32_t module, int32_t which, const char* path, const float* host_in, int64_t numel,
                            void* stream);

/* The flat fp32 arena of a module's state on the device (which as above): *dev_out = its base, *numel_out = its length in floats (leaves
 * in Flax layouts at fixed offsets, zero padding between them; the padding of the gradient arena is written as zeros by every
 * ldp_train_*_grad).  The pointer stays valid until the next ldp_train_init / ldp_destroy.  This is the data-parallel seam: with the batch
 * rows split over processes (the reference shards its batch with PositionalSharding, utils/py_utils.py:27-39, and XLA inserts the gradient
 * all-reduce), the caller sums the gradient arenas over the ranks with ONE collective per module between ldp_train_*_grad and
 * ldp_train_grad_norm / ldp_train_apply, in order on `stream`.  Every trainable module uses it: the planner and the IDM, the VAE (module 4:
 * after the last ldp_train_vae_grad_part of the rank's frames) and the image encoders (module 8 << slot: after ldp_train_encoder_backward). */
LDP_API int ldp_train_arena(ldp_handle* h, int32_t module, int32_t which, float** dev_out, int64_t* numel_out);

/* Make the sampling path use the trained parameters: master parameters -> the handle's weight store -> ldp_finalize of the listed
 * modules (what train_bc.py:143-155 relies on when it evaluates the agent it is training).  Synchronises `stream`. */
LDP_API int ldp_train_publish(ldp_handle* h, int32_t modules, void* stream);
/* The same with the EMA arena (use_ema: agent/dp_repr_agent.py:176-179).  Synchronises `stream`. */
LDP_API int ldp_train_publish_ema(ldp_handle* h, int32_t modules, void* stream);

/* -- unit-testable primitives (one Conv1dBlock / sampling conv of the U-Net) ----------------
 * y = [FiLM](Mish(GroupNorm8(Conv1d_k5_pad2(x) + b)))  with kernel in Flax layout on the host.
 * x (B,T,Cin) device, kernel (5,Cin,Cout)/bias/gn_scale/gn_bias host; film (B, 2*Cout)
 * device or NULL; y (B,T,Cout) device.  Cin is zero-padded to a multiple of 32 internally;
 * Cout must be a multiple of 8*16.  Synchronises `stream` (it packs weights on the fly). */
LDP_API int ldp_conv1d_gn_mish_film_f32(const float* x, const float* kernel_host, const float* bias_host,
                                const float* gn_scale_host, const float* gn_bias_host,
                                const float* film, float* y, int32_t B, int32_t T, int32_t Cin,
                                int32_t Cout, void* stream);

/* y = Conv1d(k=3, stride 2, XLA 'SAME' => pads (0,1))(x)  (Downsample1d, :51-56);
 * x (B,T,C) -> y (B,T/2,C). */
LDP_API int ldp_downsample1d_f32(const float* x, const float* kernel_host, const float* bias_host,
                         float* y, int32_t B, int32_t T, int32_t C, void* stream);

/* y = ConvTranspose(k=4, stride 2, 'SAME', transpose_kernel=False)(x)  (Upsample1d, :58-63);
 * x (B,T,C) -> y (B,2T,C). */
LDP_API int ldp_upsample1d_f32(const float* x, const float* kernel_host, const float* bias_host,
                       float* y, int32_t B, int32_t T, int32_t C, void* stream);

/* y = Conv3x3(x) of the StableVAE on NHWC images: stride 1 => pad 1 (ResnetBlock2D / conv_out),
 * stride 2 => pad (0,1),(0,1) + VALID (Downsample2D).  kernel (3,3,Cin,Cout) Flax layout, host.
 * Runs the exact-fp32 tile the engine's own plan picks for the shape with default options (one function decides both). */
LDP_API int ldp_conv2d_3x3_f32(const float* x, const float* kernel_host, const float* bias_host, float* y,
                       int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t stride,
                       void* stream);

/* The same stride-1 convolution on the bf16 matrix pipe through three-plane split operands
 * (csrc/sconv.hpp: x = h + m + l exactly, six of the nine plane products, fp32 accumulate;
 * |error| at the fp32 round-off level, see profiles/r04_split_probe.txt).  This is what
 * ldp_vae_encode / ldp_vae_decode run for their 64 / 32 / 16 pixel ResnetBlock2D convolutions
 * unless option "vae_split" is 0.  x (N,H,W,Cin) device fp32, H == W in {64, 32, 16},
 * Cin % 16 == 0, Cin <= 256, Cout % 128 == 0; res (N,H,W,Cout) device fp32 added to the result, or NULL;
 * stats_out (N*H*W/256, Cout, 2) device fp32: per 256-pixel tile (sum, sum of squares) of every
 * output column (what the following GroupNorm reads), or NULL; dual: 2 = the default form of the
 * library since late round 4: TWO fp16 planes per operand (x = h + l' / 2^11, h = fp16(x),
 * l' = fp16((x - h) * 2^11)) and THREE exact products, hh in one accumulator, hl' + l'h in a second
 * one (option "vae_split_f16"); 0 / 1 = three bf16 planes, six products, one
 * accumulator (round 4's two-accumulator A/B arm was removed in round 5).  With dual = 2, operands
 * outside the fp16 planes' range (|x| >= 65504) make this primitive rerun on the bf16 planes by itself
 * (ldp_range_fallbacks() counts).
 * Reference: fp32 nn.Conv of diffusers' ResnetBlock2D. */
LDP_API int ldp_conv2d_3x3_bf16x3(const float* x, const float* kernel_host, const float* bias_host,
                          const float* res, float* y, float* stats_out, int32_t N, int32_t H,
                          int32_t W, int32_t Cin, int32_t Cout, int32_t dual, void* stream);

/* -- introspection for bench.py -------------------------------------------------------------
 * Number of kernels enqueued by the last planner / IDM call (for a graph replay: the launches the
 * captured graph contains).  which: 0 = MFMA conv kernels (the dominant kernel), 1 = all kernels. */
LDP_API int ldp_launch_count(ldp_handle* h, int32_t which, int64_t* launches);
/* -- fault protocol of the in-launch exchanges ------------------------------------------------
 * At small batches a GroupNorm group (or a K range) is split over work-groups that exchange
 * partial results inside one launch; that needs the launch's whole grid co-resident, which holds
 * while the handle has the GPU to itself.  The wait is a bounded spin: a work-group whose peer
 * never answers stores 1 into a pinned host word instead of hanging.
 *   ldp_poll_fault : host read of the pinned words, no stream is synchronised.  *faulted != 0 if a
 *                    fault was recorded since the last poll (bit 0: exchange fault -- the handle has
 *                    switched to safe mode, no in-launch exchange at all; bit 1: range fault, below);
 *                    captured graphs are dropped (the first fault of a kind waits for the handle's own
 *                    graph replays, nothing else) and the results of calls enqueued since the previous
 *                    poll must be recomputed.  Poll after synchronising on the results.
 *   ldp_check_fault: hipStreamSynchronize(stream) + poll; LDP_EFAULT when a fault was recorded.
 * Every sampling / VAE entry point also looks at the words first and fails with LDP_EFAULT while an
 * unacknowledged fault is pending, so a caller that never polls cannot keep consuming bad results.
 *
 * Range guard of the split-operand convolutions.  Above 256 plans and in the StableVAE the large
 * convolutions run on the 16-bit matrix pipe with every fp32 operand split into TWO fp16 planes
 * (x = h + l' / 2^11: 22 significand bits).  fp16 planes hold |x| < 65504 where the
 * reference's fp32 nn.Conv holds 3.4e38.  Weights are checked when their planes are packed (a conv
 * with |w| >= 65504 keeps three bf16 planes, which have fp32's range); activations are checked by the
 * kernels that touch them anyway (the plane producer of the StableVAE convs; the planner tiles see
 * the non-finite sum of squares an overflowed plane always produces).  A violation raises the second
 * pinned word: the calls since the last poll are reported faulted exactly like an exchange fault, and
 * the handle runs every split convolution on three bf16 planes from then on ("range_fallback" = 1,
 * readable / resettable through the options; "range_faults_seen" counts).  Results are then those of
 * fp32-range arithmetic: never inf / NaN where the reference's are finite. */
LDP_API int ldp_poll_fault(ldp_handle* h, int32_t* faulted);
LDP_API int ldp_check_fault(ldp_handle* h, void* stream);

/* Times a handle-less primitive (ldp_conv2d_3x3_bf16x3 with dual = 2) left the fp16 planes for the
 * bf16 ones because a weight or an activation was outside their range (process-wide; tests). */
LDP_API int64_t ldp_range_fallbacks(void);

/* -- runtime options --------------------------------------------------------------------------
 * Work-splitting switches (results stay correct to fp32 round-off): "no_csplit", "no_mb2",
 * "no_kw", "kw_min_it", "kw_bmax", "by_sample" (XCD placement threshold), "idm_hs",
 * "idm_rt_major", "idm_noring", "idm_unfused", "safe_mode", "range_fallback"; "vae_split" (1: the StableVAE's
 * large 3x3 convs on split operands of the 16-bit matrix pipe, 0: exact-fp32 MFMA), "vae_split_f16"
 * (1: two fp16 planes / three products, 0: three bf16 planes / six), "vae_split_s2" (its stride-2 convs on fp16 planes too); the planner
 * above 256 plans: "planner_split" (0: exact fp32 everywhere), "planner_split_f16" (as for the
 * StableVAE), "planner_split_mb2", "planner_split_t16"; the IDM above 256 plans: "idm_f16" (1: its MLPResNet blocks on two fp16 planes over 32-row
 * tiles, 0: exact fp32), "idm_f16_min_rows", "idm_f16_hs"; and the A/B switches listed in
 * csrc/engine.hpp; read-only counters "stat_mb2_launches", "stat_f16_launches", "stat_train_gemm_<nn|nt|tn>_<32|64|128>[_ki2]",
 * "stat_train_gemm_fused", "stat_train_gemm_reduce" (training GEMM launches per kernel instantiation), "stat_idm_f32_hs<1|2|4|8>[_ring][_nt]",
 * "stat_idm_f16_hs<2|4>", "stat_idm_unfused" (fused IDM launches per kernel instantiation; calls of the unfused path).  Timing ablations for
 * tools/ (results WRONG by construction): "dbg" (bit mask), "repeat".  Test hook: "inject_fault" (1: an
 * exchange fault, 2: a range fault).
 * Read-only through ldp_get_option: "any_debug", "faults_seen", "range_faults_seen", "n_cu", "graphs".
 * Nothing is ever read from the environment. */
LDP_API int ldp_set_option(ldp_handle* h, const char* name, int64_t value);
LDP_API int ldp_get_option(ldp_handle* h, const char* name, int64_t* value);

/* -- noise source primitives (tests) ----------------------------------------------------------
 * The in-kernel generator is Philox4x32-10 with counter (elem lo, elem hi, step, stream_id) and key
 * (seed lo, seed hi); element i of a call uses elem0 + i.  raw: 4 uint32 words per element
 * (out_dev has 4n words); normal: one N(0,1) per element (Box-Muller on words 0, 1). */
LDP_API int ldp_philox_raw(uint64_t seed, uint64_t elem0, uint32_t step, uint32_t stream_id,
                   uint32_t* out_dev, int64_t n, void* stream);
LDP_API int ldp_philox_normal(uint64_t seed, uint64_t elem0, uint32_t step, uint32_t stream_id,
                      float* out_dev, int64_t n, void* stream);

/* -- device-resident training data (csrc/data.hip) ----------------------------------
 * The welded episode tables of a dataset (or of a mixture: its datasets welded one behind the other)
 * live in HBM; one launch draws the B window indices of a batch and gathers the episode-clamped
 * windows of every key.  Stateless: no handle, no workspace, no atomics -- the outputs are a pure
 * function of the arguments.  Arrays marked "host" are read during the call and travel as kernel
 * arguments (no copy is enqueued); nothing synchronises.
 * replaces: RobomimicLatentDataset._sample / get_item / _get_batch (data/robomimic_latent_data.py:112-147,
 * the same in data/alohasim_latent_data.py), RobomimicMixedLatentData._sample
 * (data/robomimic_mixed_latent_data.py:84-88), the DataLoader collation behind them and the
 * `tensor.numpy()` map + device_put of train_bc.py:78. */
#define LDP_DATA_MAX_KEYS 16
#define LDP_DATA_MAX_SETS 8

typedef struct ldp_data_key {
  const void* table;  /* device: welded table of this key, (total_rows, row_bytes) bytes, any element type        */
  void* out;          /* device: (B, n_rows, row_bytes) bytes                                                     */
  int64_t row_bytes;  /* multiple of 4; table and out must be 4-byte aligned (16: rows move as 16-byte vectors)   */
  int32_t first_row;  /* first window row this key takes: 0 (observations) or frame_stack - 1 (actions)           */
  int32_t n_rows;     /* window rows it takes; first_row + n_rows <= W = frame_stack + seq_length - 1             */
} ldp_data_key;

/* The draw alone.  Sample b, global row r = row_offset + b, takes the Philox words w of (seed, elem = r, step,
 * LDP_PHILOX_STREAM_DATA): dataset d = the first with w[1] < thr[d] (thr = floor(cumulative split * 2^32) as uint64;
 * the last one is taken as 2^32 whatever is passed), index_out[b] = dataset_base[d] + ((uint64) w[0] * dataset_total[d] >> 32)
 * -- a multiply-shift map onto [0, total) whose bias is below total / 2^32, hence dataset_total[d] < 2^31.  Deliberately
 * not NumPy's randint stream.  dataset_base / dataset_total / thr: host, n_sets (1 .. LDP_DATA_MAX_SETS) entries.
 * replaces: `np.random.randint(self.total_n_sequences)` (robomimic_latent_data.py:113) and `random.choices(..., train_split)`
 * (robomimic_mixed_latent_data.py:86) of one batch. */
LDP_API int ldp_data_draw(const int64_t* dataset_base, const int64_t* dataset_total, const uint64_t* thr, int32_t n_sets,
                          uint64_t seed, int64_t row_offset, uint32_t step, int32_t B, int64_t* index_out, void* stream);

/* One batch in ONE launch, whatever n_keys (1 .. LDP_DATA_MAX_KEYS; keys: host).  Sample b has the welded row i = index_in[b]
 * (device int64, clamped to [0, total_rows) so that nothing outside the tables is ever read) or, with index_in NULL, the draw
 * above; bounds (device int32, (total_rows, 2)) holds the episode [s, e) of every welded row.  Window row j of key k is welded
 * row clamp(i - (frame_stack - 1) + first_row + j, s, e - 1), j < n_rows.  index_out (device int64, B) may be NULL.
 * total_rows < 2^31 and n_rows * row_bytes < 2^31; all byte offsets are 64-bit. */
LDP_API int ldp_data_sample(const ldp_data_key* keys, int32_t n_keys, const int32_t* bounds, int64_t total_rows,
                            const int64_t* dataset_base, const int64_t* dataset_total, const uint64_t* thr, int32_t n_sets,
                            uint64_t seed, int64_t row_offset, uint32_t step, int32_t B, int32_t frame_stack, int32_t seq_length,
                            const int64_t* index_in, int64_t* index_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LDP_HIP_H */
