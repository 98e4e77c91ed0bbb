// engine.hpp -- host-side state of one ldp_handle: weight store, packed device weights,
// constant tables, per-batch workspaces and the hipGraphExec cache.
#pragma once
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "common.hpp"
#include "tconv.hpp"

namespace ldp {

struct HostTensor {
  std::vector<int64_t> shape;
  std::vector<float> data;
  int64_t numel() const {
    int64_t n = 1;
    for (auto s : shape) n *= s;
    return n;
  }
};

// one convolution's device-resident parameters
struct ConvW {
  DevBuf w, bias, gn_scale, gn_bias, bres;      // w holds nj (+1 with has_res: the 1x1 projection) taps per chunk
  DevBuf wsplit;                                // the same kernel as three bf16 planes, or empty: 3x3 convs of the StableVAE (sconv.hpp); planner k = 5 convs on 32-row tiles (tconv SPLIT)
  DevBuf wsplith;                               // 32-row tiles' weights as two fp16 planes (tconv SPLIT = 4), or empty
  DevBuf wsplit16h;                             // the same convs as two fp16 planes (tconv SPLIT = 3, option planner_split_f16), or empty
  DevBuf wsplit16;                              // planner k = 5 convs on 16-row split tiles (tconv SPLIT, MB = 1), or empty
  bool f16_refused = false;                     // a weight of this conv is outside the fp16 planes' range (|w| >= 65504 or not finite): bf16 planes / exact fp32 only
  int nj = 0, cin = 0, cout = 0, cin_p = 0, cout_p = 0;
  bool has_gn = false, has_res = false;
  bool t2s = false;                             // w is packed for the shared-product form of two positions (t2pack.hpp): W2, W3 - W2, W1 - W2 (+ projection)
  bool t4s = false;                             // w is packed for the nine-product form of four positions (t4pack.hpp): nine combinations (+ projection)
};

struct ResBlock {
  ConvW c1, c2;          // c1 carries the fused 1x1 residual projection when proj
  bool proj = false;
  int cin = 0, cout = 0;
  int film_off = 0;      // column offset of this block's (scale|bias) slice in the FiLM tables
  std::string prefix;    // weight-store path of the block (the plane-packed copies are built lazily from it)
};

struct PlannerState {
  bool ready = false;
  int D = 0, DP = 0, G = 0, T = 0, L = 0, E = 0, n_train = 0;
  int C0P = 128;                  // input-channel chunk the first conv is packed for (DP real, rest zero)
  std::vector<int> dims;
  std::vector<ResBlock> blocks;
  std::vector<ConvW> down, up;
  ConvW fin_block, fin_conv;
  int F = 0;                      // total FiLM width = sum 2*Cout
  DevBuf film_t;                  // (n_train, F): Mish(temb_k) @ W[:E] + b
  DevBuf wfilm_g;                 // (G, F): rows E.. of every block's FiLM Dense kernel
  // workspaces (sized for ws_B samples)
  int ws_B = 0;
  DevBuf state, cond, film_g, bufA, bufB, bufC, bufR, noise, xchg, kw_slab;
  DevBuf solver_eps, solver_x0;   // sampler 2 (solver.hip): the evaluation's eps (B, T, D) unpadded, and the previous step's clipped x0 padded like `state`
  DevBuf ctarget, cmask;          // constrained planning (constrain.hip): the call's target (float) and mask (uint8) padded like `state`, zero beyond D and the real rows
  DevBuf gtarget, gwg, ganchor;   // guided planning (guide.hip): the call's target and weights (B, T, DP) and anchor (B, DP), padded like `state`
  DevBuf gcol;                    // ... and its host vectors: [lam | beta | lo | hi] at 128 floats each, then the step sizes rho[n_steps]
  size_t xchg_stride = 0;         // granules per conv launch
  uint64_t calls = 0;             // planner calls on this handle (slab hygiene, see planner_prepare)
  std::vector<DevBuf> skip;
};

struct IdmState {
  bool ready = false;
  int D = 0, A = 0, AP = 0, H = 0, NB = 0, n_train = 0, TD = 0;
  ConvW in_a;                      // (A, H) rows of MLPResNet_0/Dense_0 (kept in Flax layout, VALU)
  DevBuf w_in_s, b_in;             // (2D, H) rows + bias
  DevBuf ctab;                     // (n_train, H): cond_k @ W0[A+2D:]
  struct Blk { DevBuf ln_s, ln_b; ConvW d0, d1; };
  std::vector<Blk> blks;
  ConvW out;                       // (H -> AP)
  DevBuf wout_t, bout;             // fused path: Dense_1 kernel transposed to (A, H) + bias (A)
  int ws_R = 0;
  DevBuf state, state2, spart, h0, h1, y, z, noise, trans, part0, part1;
  int state_cur = 0;               // fused path: which of state / state2 holds the current a_t
};

struct GraphKey {
  int kind, B, n_steps, sampler, noise_mode;      // kind 0 planner loop, 1 IDM loop, 2 joint sample()
  int n_steps2 = 0, noise_mode2 = 0;              // joint graph: the IDM loop's step count / noise mode
  int begin = 0, end = -1;                        // planner loops (kind 0, 2): the executed steps [begin, end) of n_steps; (0, -1) = no planner range (the IDM loop, kind 1)
  int constrain = 0;                              // planner loops: 0 = the free loop, else the LDP_CONSTRAIN_* mode whose launches the graph carries (constrain.hip)
  int guide = 0;                                  // planner loops: 0 = no guide, else LDP_GUIDE_ON / LDP_GUIDE_ANCHOR: the guide the stepped loop's launches carry
  bool operator<(const GraphKey& o) const {
    if (kind != o.kind) return kind < o.kind;
    if (B != o.B) return B < o.B;
    if (n_steps != o.n_steps) return n_steps < o.n_steps;
    if (sampler != o.sampler) return sampler < o.sampler;
    if (noise_mode != o.noise_mode) return noise_mode < o.noise_mode;
    if (n_steps2 != o.n_steps2) return n_steps2 < o.n_steps2;
    if (noise_mode2 != o.noise_mode2) return noise_mode2 < o.noise_mode2;
    if (begin != o.begin) return begin < o.begin;
    if (end != o.end) return end < o.end;
    if (constrain != o.constrain) return constrain < o.constrain;
    return guide < o.guide;
  }
};

// Runtime options (ldp_set_option).  The first group changes how work is split over work-groups
// (results stay correct, to fp32 round-off); `dbg` / `repeat` are timing ablations for tools/
// (results wrong by construction; bench.py marks such a run INVALID).  Nothing here is read from
// the environment.
struct Options {
  int no_csplit = 0;      // one work-group per GroupNorm group at any B
  int no_mb2 = 0;         // one 16-sample row block per work-group at any B
  int planner_split_8w = 1;  // 257 .. 512 plans (one work-group per CU): the four-wave fp16-plane tiles of the T = 4 / T = 8 layers as eight waves (twice the K slices)
  int planner_split_t2res16 = 1;  // 353 .. 512 plans: the T = 2 convs with the projection on fp16 planes as 16-row tiles over whole groups (else: bf16 planes, 32-row tile over half groups)
  int planner_split_t2all16 = 1;  // ... and the T = 2 convs WITHOUT the projection likewise (0: the 32-row fp16 tile over half groups with its in-launch statistics exchange)
  int t2_mb2 = 0;         // A/B (round 5): the 1024 -> 1024 T = 2 convs at 129..256 plans as quarter groups x two row blocks (profiles/r05_t2_mb2_ab.txt)
  int no_kw = 0;          // no K split over work-groups
  int kw_min_it = 1, kw_bmax = 128;
  int vae_split = 1;      // StableVAE stride-1 3x3 convs at 64 / 32 / 16 pixels on split bf16 operands (sconv.hpp: 6 plane products, fp32 accumulate); 0 = exact-fp32 MFMA
  int vae_split_f16 = 1;  // those convs on TWO fp16 planes / THREE products (sconv3 NPL = 2: x = h + l' / 2^11) instead of three bf16 planes / six (0, A/B)
  int vae_split_s2 = 1;   // the StableVAE's stride-2 convs (Downsample2D) on two fp16 planes too (tconv MODE_K3S, SPLIT = 3; round 5)
  int vae_split_gn_only = 0; // split operands only behind a GroupNorm (the resnet convs), not for the decoder's upsampler convs on raw inputs (A/B)
  int vae_no_conv_stats = 0;    // GroupNorm statistics always by their own pass (cross-check of the sums the 3x3 convs leave in their epilogue)
  int vae_no_conv_in_stats = 0; // the same for conv_in
  int planner_split = 1;  // planner: k = 5 convs of the 256- / 512- / 1024-channel levels on split bf16 operands (tconv SPLIT) above 256 plans, i.e. where one
                          // work-group owns a whole GroupNorm group (0: exact-fp32 kernels everywhere; 2: at any batch whose plan has no column / K split -- tests); the
                          // plane-packed weights are built at the first call that needs them
  int planner_split_cs2 = 1;    // the T = 2 layers around 512 plans on 32-row split tiles with every GroupNorm group over two work-groups (0: exact fp32 there)
  int planner_split_updown = 1; // the stride-2 / transposed convs between the levels on 16-row split tiles too (0: exact fp32; A/B)
  int planner_split_c256 = 1;   // 0: the 256-channel level stays on the exact-fp32 kernel (A/B)
  int planner_split_mb2 = 1;    // 16-row split tiles of the 1024-channel T = 4 layers over two row blocks per wave (tconv SPLIT = 2) once 32-sample
                                // work-groups cover the chip (from 993 plans); 0 = one row block (A/B; the plans are bit-identical either way)
  int planner_split_f16 = 1;    // the k = 5 split tiles on TWO fp16 planes and THREE products (tconv SPLIT = 3 / 4: x = h + l' / 2^11) instead of three
                                // bf16 planes and six: half the matrix instructions, two thirds of the operand bytes, the same margins; 0 = the bf16 form (A/B)
  int planner_split_t16 = 1;    // pred_horizon 16's (16, 256) level on fp16 planes too (needs planner_split_f16; 0: exact fp32 there, A/B)
  int planner_split_t2res = 1;  // the two T = 2 convs with the projection on 16-row fp16 tiles over two row blocks per wave from 993 plans (0: 32-row bf16 tiles; A/B)
  int up_full_depth = 0;  // transposed convs on 256-channel chunks (the round-2 choice) instead of 128
  int no_fin_rows = 0;    // final 1x1 conv over whole samples (round-2 launch shape) instead of position pairs
  int no_batch_split = 0; // never run the leading power-of-two part of an in-between batch as its own loop (batch_split())
  int idm_unfused = 0;    // IDM as one launch per Dense / LayerNorm (the round-1 path)
  int by_sample = 2;      // XCD affinity by sample block while weights < by_sample x input activations (0: always by group)
  int place2d = 0;          // split tiles (> 256 plans): two-dimensional XCD placement of the group-major launches (tconv.hpp; A/B)
  int idm_noring = 0;     // fused IDM: never use the ringed (one work-group per CU) variant
  int idm_rt_major = 1;   // fused IDM: XCD affinity by row tile (1) or by hidden slice (0)
  int idm_stream = -1;    // fused IDM: K-partials non-temporal (1), plain (0), by row count (-1)
  int idm_hs = 0;         // hidden slices per row tile of the fused IDM block (0 = by row count)
  int idm_f16 = 1;        // fused IDM blocks on two fp16 planes / three products over 32-row tiles (idm.hip idm_block_h16_kernel) for every batch above 256 plans (idm_f16_min_rows rows)
  int idm_f16_min_rows = 1040;      // (the first 16-row bucket above 256 plans x 4 rows)
  int idm_f16_hs = 0;     // A/B: hidden slices of that kernel (0 = four, 2)
  int train_fuse_reduce = 1; // training GEMMs: the last work-group of a split-K tile adds the partials up inside the launch (0: a reduce launch per GEMM; A/B)
  int train_sides = 1;       // training: side streams per module the weight-gradient work is dealt to (1 .. 3)
  int train_gn4 = 1;         // training: the one-pass GroupNorm kernels where a (sample, group) block has exactly 256 values (0: the generic two-pass kernels; A/B)
  int train_group_proj = 1;  // training: a projection block's two convolutions over its input (and their two data gradients) as one launch each (0: two; A/B)
  int train_intra_split = 0; // training GEMMs: the first factor of two of a K split inside the work-group (two wave quartets, hand-over through LDS) instead of over
                            // work-groups (1; measured 3.45 - 3.55 ms per step against 3.40 - 3.42: no partial block and no ticket, but 512-thread work-groups place worse)
  int train_streams = 1;     // training: weight-gradient GEMMs and parameter column sums on a side stream next to the data-gradient chain (0: one stream; A/B)
  int train_split = 1;      // training GEMMs: split the K steps of a launch over work-groups until the grid fills the chip (0: never; A/B)
  int train_wg_target = 384; // ... until the launch has this many work-groups (192 / 384 / 768 / 1536: 5.47 / 4.99 / 5.19 / 5.67 ms per step)
  int train_big = 0;        // training GEMMs: 128 x 128 tiles where both M and N reach 128 (1; measured slower than the 32 / 64-row tiles with split K: profiles/r06_update_gemm_ab.txt)
  int train_small_wg = 1 << 20; // training GEMMs (train.hip seg_gemm): 32-row tiles when the 64-row tiling has fewer work-groups than this.  Final tree at 256
                            // samples: 128 / 256 / 512 / 768 / always = 3.52 / 3.44 / 3.38 / 3.35 / 3.33 ms per step (the 64-row tiles were worth it before the
                            // in-launch split-K finish and the side streams: 5.44 -> 4.99 ms then)
  int dbg = 0, repeat = 1;
  int64_t timeline_ptr = 0;   // device buffer of tools/timeline.py (64 slots x 1 MiB); only -DLDP_TIMELINE builds write to it
  bool any_debug() const { return dbg != 0 || repeat != 1 || timeline_ptr != 0; }
};

constexpr int LDP_STAT_GEMM_FUSED = 15, LDP_STAT_GEMM_REDUCE = 16;      // ldp_handle::stat_train_gemm
constexpr int LDP_STAT_IDM_F16_HS2 = 16, LDP_STAT_IDM_F16_HS4 = 17, LDP_STAT_IDM_UNFUSED = 18;      // ldp_handle::stat_idm
inline int stat_idm_f32(int hs, bool ringed, bool stream) { return (hs == 1 ? 0 : hs == 2 ? 4 : hs == 4 ? 8 : 12) + (ringed ? 2 : 0) + (stream ? 1 : 0); }

// sampler 2 (solver.hip): one row of schedule.solver_coefficients, and the table registered for one step count
struct SolverCoef { float t, inv_a, sg, c_x, c_D, w; };
struct SolverTable {
  std::vector<int32_t> ts;        // timesteps, first executed step first: strictly decreasing, the last is 0
  std::vector<SolverCoef> rows;
};

struct GraphEntry {
  hipGraphExec_t exec;
  int64_t conv_launches, total_launches;
  uint64_t last_use = 0;          // handle's graph clock at the last replay (LRU eviction)
  hipEvent_t done = nullptr;      // recorded behind every replay on the caller's stream: what drop_graphs waits for (not the whole device)
};

}  // namespace ldp

struct ldp_handle {
  ldp_config cfg;
  std::map<std::string, ldp::HostTensor> weights;
  ldp::PlannerState pl;
  ldp::IdmState idm;
  // device control words, one block of 4 uint64 per loop: {seed, first global row, call epoch, unused};
  // block 0 = planner, block 1 = IDM.  Written by set_seed_launch on the caller's stream before a loop
  // (or its captured graph) runs, so captured graphs never bake a seed.
  ldp::DevBuf seed;
  uint64_t epoch_planner = 0, epoch_idm = 0;   // host-side call epochs, handed to set_seed_launch (never read back from the device)
  uint64_t* ctl_planner() const { return seed.as<uint64_t>(); }
  uint64_t* ctl_idm() const { return seed.as<uint64_t>() + 4; }
  // Fault word: pinned host memory mapped into the device.  A split work-group whose peer never
  // answered (bounded spin) stores 1 here; the host reads it without synchronising anything.
  volatile unsigned int* fault_host = nullptr;
  unsigned int* fault_dev = nullptr;
  int fault_pending = 0;                 // faults seen and not yet acknowledged through ldp_poll_fault (bit 0: exchange, bit 1: fp16-plane range)
  int64_t faults_seen = 0;
  bool safe_mode = false;                // after a fault: no in-launch cross-work-group exchange any more
  // Range guard of the two-fp16-plane operand form: fp16 planes hold |x| < 65504 where fp32 (and the three
  // bf16 planes) hold 3.4e38.  Word 1 of the pinned fault block is raised by the producers / consumers of fp16 planes
  // when an operand left that range (planes_kernel: |x| >= 65504 or not finite; tconv F16 tiles: a non-finite conv
  // output, which an overflowed plane always produces).  The host then treats the calls since the last poll as
  // faulted, and runs every split conv on three bf16 planes (fp32 range) from then on.
  bool range_fallback = false;           // sticky until ldp_set_option("range_fallback", 0)
  int64_t range_faults_seen = 0;
  unsigned int* range_dev() const { return fault_dev ? fault_dev + 1 : nullptr; }
  bool f16_planner() const { return opt.planner_split_f16 != 0 && !range_fallback; }
  bool f16_vae() const { return opt.vae_split_f16 != 0 && !range_fallback; }
  ldp::Options opt;
  std::map<int, ldp::SolverTable> solver_tabs;   // ldp_solver_timesteps: n_steps -> the table sampler 2 runs with that step count
  ldp::DevBuf plan_out, act_out, obs_last;   // joint sample(): handle-owned outputs the graph writes
  ldp::DevBuf cand_cond;                 // ldp_plan_candidates (select.hip): the condition tiled over the candidate rows (no graph node reads it)
  ldp::DevBuf slot_buf;                  // ldp_plan_warm_init / ldp_agent_resample (replan.hip): a slot table given on the host (no graph node reads it)
  hipStream_t cap_stream = nullptr;      // internal stream used only for graph capture
  int n_cu = 256;                        // compute units of cfg.device (co-residency bound of the column split)
  // Captured loops, least-recently-used eviction at `graph_cap` entries.  Batches are bucketed to whole 16-row tiles
  // (bucket_rows): the env harness changes B call to call (utils/rm_env_utils.py:150-199) and a best-of-N service
  // asks for arbitrary N; every B of a bucket replays the same graph.
  std::map<ldp::GraphKey, ldp::GraphEntry> graphs;
  std::vector<ldp::GraphEntry> retired_execs;   // evicted from the cache, possibly still running: destroyed at the next idle point
  uint64_t graph_clock = 0;
  int graph_cap = 32;
  int64_t graphs_captured = 0, graphs_evicted = 0;
  int64_t last_conv_launches = 0, last_total_launches = 0;
  int64_t stat_f16_launches = 0;         // likewise: conv launches on fp16 planes
  int64_t stat_t2_shared_launches = 0;   // likewise: exact-fp32 k = 5 launches over two positions in the three-product form (tconv.hpp t2_shared)
  int64_t stat_t4_shared_launches = 0;   // likewise: exact-fp32 k = 5 launches over four positions in the nine-product form (tconv.hpp t4_shared)
  std::map<uint64_t, int64_t> plan_log;       // every distinct tconv instantiation this handle launched, keyed by plan_key (option "dump_plans" prints it: tools/r5/plans_used.py)
  int64_t stat_mb2_launches = 0;         // conv launches enqueued (eagerly or into a capture) on two-row-block split tiles since ldp_create: read-only option
  // training GEMM launches enqueued since ldp_create, per instantiation of train.hip's kernel family: [form (NN, NT, TN) * 5 + {32-row, 32-row KI = 2,
  // 64-row, 64-row KI = 2, 128 x 128}], then launches that finished split K in-launch and reduce_parts_kernel launches.  Read-only options
  // "stat_train_gemm_<nn|nt|tn>_<32|64|128>[_ki2]", "stat_train_gemm_fused", "stat_train_gemm_reduce"; the dry walk of a tape counts nothing.
  int64_t stat_train_gemm[17] = {};
  // fused IDM launches (with IF_BLOCK and tail-only alike) enqueued since ldp_create, per instantiation of idm.hip's block kernels:
  // idm_block_kernel<HS, RINGED, STREAM> at [4 log2(HS) + 2 RINGED + STREAM], idm_block_h16_kernel<2 / 4> at [16] / [17], and calls of
  // idm_forward_unfused at [18].  Read-only options "stat_idm_f32_hs<1|2|4|8>[_ring][_nt]", "stat_idm_f16_hs<2|4>", "stat_idm_unfused".
  int64_t stat_idm[19] = {};
  void* vae = nullptr;                   // VaeState (vae.hip)
  void* train = nullptr;                 // Trainer (train.hip): master parameters, gradients, Adam moments, launch tables; created by ldp_train_init
  void* resnet = nullptr;                // RnState (resnet.hip): the ResNet-18 image encoders of DPAgent (weight modules encoder0 .. encoder3)
};

namespace ldp {
std::map<std::string, int64_t> tconv_plan_log();       // tconv_misc.hip: every instantiation this process launched (a snapshot, as text)
uint64_t plan_key(const ConvPlan& p);
std::string plan_text(uint64_t key);
// schedule tables (host, float64 -> float32), mirror of schedule.py
void make_step_coefs(int n_train, int n_steps, int sampler, std::vector<StepCoef>& out);
void sinusoid_table(int n, int dim, bool cos_first, std::vector<float>& out);

// weight packing into the lane-linear MFMA fragment layout
std::vector<float> pack_conv(const float* w, int nj, int cin, int cout, int cin_p, int cout_p);

bool fits_f16_planes(const float* w, size_t n);
std::vector<uint16_t> pack_conv_split16h(const float* w, int nj, int cin, int cout);
int get_weight(ldp_handle* h, const std::string& path, const HostTensor** out,
               std::initializer_list<int64_t> shape);
// t_pos: positions a k = 5 conv runs at (0: not a k = 5 conv / unknown); two positions get the shared-product packing, four the nine-product one
int make_conv(ldp_handle* h, const std::string& prefix, int nj, int cin, int cout, int cin_p,
              int cout_p, const char* gn_prefix, hipStream_t s, ConvW& out, int t_pos = 0);

void drop_graphs(ldp_handle* h);
void reap_retired_graphs(ldp_handle* h);
// Rows a sampling loop is launched over: B rounded up to whole 16-row MFMA tiles.  The tiles compute all 16 rows
// anyway, rows never mix (GroupNorm / LayerNorm statistics are per row, MFMA rows are independent), the workspaces
// are sized in whole tiles, and only the B real rows are copied in and out (eagerly, outside the captured loop): the
// dead rows chew on whatever the buffers hold.  A row's bits therefore depend on its 16-bucket only, and every B of a
// bucket shares one launch plan and one captured graph.  Explicit step noise is laid out (steps, B, ...), i.e. its
// stride is B itself: those (parity-test) calls keep the exact B.
inline int bucket_rows(int B, bool explicit_noise) { return explicit_noise ? B : (B + 15) / 16 * 16; }
// the pieces of ldp_plan_sample / ldp_idm_sample, shared with the joint ldp_agent_sample
// begin / end: the executed steps [begin, end) of the planner loop, 0 <= begin <= end <= n_steps (every planner caller sets them; the whole
// loop is (0, n_steps)).  Step i is the same step whatever the range: coefficients, timestep, noise row, Philox key and exchange tag
// all carry i itself.  idm_loop always runs all n_steps and does not read them.  The default end = -1 is no range: planner_loop refuses
// it (LDP_EINVAL), so a planner caller that forgets the two fields fails loudly instead of running zero steps.
// constrain: 0, or the LDP_CONSTRAIN_* mode: C_begin in front of the first step and C_{i+1} behind step i, on the target / mask staged
// into P.ctarget / P.cmask.
// guide: 0, or LDP_GUIDE_ON / LDP_GUIDE_ANCHOR: the guide staged into P.gtarget / P.gwg / P.ganchor / P.gcol (ANCHOR: with the continuity term).
// planner_loop has two shapes, chosen by (sampler, guide) alone (stepped_loop):
//   fused    DDPM / DDIM without a guide: the U-Net's last launch does the scheduler step; a constraint is a launch of its own (constrain.hip)
//   stepped  a guide, or sampler 2: the U-Net writes eps only and ONE plan_compose_step_kernel launch behind it (compose.hip) does the guided
//            data prediction, the scheduler or solver update and C_{i+1}; C_begin runs once in front
struct LoopSpec { int n_steps = 0, sampler = 0; bool explicit_noise = false; int begin = 0, end = -1; int constrain = 0; int guide = 0; };
inline bool stepped_loop(const LoopSpec& L) { return L.guide != 0 || L.sampler == LDP_SAMPLER_DPMPP; }
constexpr int LDP_GUIDE_ON = 1, LDP_GUIDE_ANCHOR = 2;
int check_step_range(int begin, int end, int n_steps, const char* what);
struct WarmSpec;                                 // a warm start of the planner state (below)
// solver_h: the handle whose registered tables may serve LDP_SAMPLER_DPMPP (LDP_ESTATE when it has none for n_steps); nullptr where that
// sampler is not built (the IDM loop, warm starts, constraints: LDP_EINVAL)
int check_sampler(int sampler, int n_steps, int n_train, const char* what, const ldp_handle* solver_h = nullptr);
int entry_fault_check(ldp_handle* h);
int planner_pre(ldp_handle* h, const float* cond, const float* x_init, const float* step_noise, uint64_t seed,
                int64_t row_offset, const LoopSpec& L, int B, hipStream_t s, const WarmSpec* warm = nullptr);
int planner_loop(ldp_handle* h, int B, const LoopSpec& L, hipStream_t q);
int idm_pre(ldp_handle* h, const float* transition, const float* a_init, const float* step_noise, uint64_t seed,
            int64_t row_offset, const LoopSpec& L, int R, hipStream_t s);
int idm_loop(ldp_handle* h, int R, const LoopSpec& L, hipStream_t q);
const float* idm_result(ldp_handle* h);          // (R, AP) padded a_0 after idm_loop
int idm_workspace(ldp_handle* h, int R);
int planner_workspace(ldp_handle* h, int B);
int run_or_replay(ldp_handle* h, const GraphKey& key, bool use_graph, hipStream_t s,
                  const std::function<int(hipStream_t)>& enqueue);
int planner_finalize(ldp_handle* h, hipStream_t s);
struct UnetTap;                                  // engine.hip: the test hook of ldp_unet_trace (nullptr on every product path)
int planner_forward_launch(ldp_handle* h, int B, const int* k_dev, int k, bool step,
                           const StepCoef* coef, const float* noise, int step_idx, float* eps_out,
                           hipStream_t s, UnetTap* tap = nullptr);
int idm_finalize(ldp_handle* h, hipStream_t s);
int vae_finalize(ldp_handle* h, hipStream_t s);
void vae_destroy(ldp_handle* h);
int resnet_finalize(ldp_handle* h, hipStream_t s);         // resnet.hip: every encoder slot that has leaves
void resnet_invalidate(ldp_handle* h, int slot);
void resnet_destroy(ldp_handle* h);
void train_destroy(ldp_handle* h);
void betas_squaredcos(int n, std::vector<float>& betas, std::vector<float>& alphas, std::vector<float>& acp);

// ---- warm-started replanning (replan.hip) ------------------------------------------------------------------
// Where a warm planner state comes from: rows slot_dev[b] (or b) of `x_prev`, shifted by `shift` positions with the edge held, noised with
// the coefficients (a, s) of the first executed step (warm_coefs); the slot table is already on the device (stage_slots).
struct WarmSpec { const float* x_prev; const int32_t* slot_dev; int shift; float a, s; };
// a = sqrt(abar_t), s = sqrt(1 - abar_t) at t = t_begin = (n_steps - 1 - step_begin) * (n_train / n_steps): float64 from the float32 abar table, cast to float
int warm_coefs(int n_train, int n_steps, int step_begin, float* a, float* s);
// slot table -> device pointer: a host table is checked against 0 .. n_slots-1 (LDP_EINVAL names the entry) and copied into the handle's
// slot buffer; a device table is passed through unchecked; NULL stays NULL
int check_host_slots(const int32_t* slot, int n_slots, int B);      // the check alone: all B entries of a host table (NULL / device: nothing)
int stage_slots(ldp_handle* h, const int32_t* slot, int n_slots, int B, hipStream_t s, const int32_t** dev_out);
// dst (B, T, ld_out) <- a * x_prev[src(b), min(j + shift, T-1), c] + s * eps for c < D, 0 for D <= c < ld_out; eps = the Philox draw of
// philox_init_kernel for global row row0 + b * T + j (row0 = row_offset * T).  ld_out is DP (the loop state) or D (caller memory).
int plan_warm_init_launch(const float* x_prev, const int32_t* slot_dev, float* dst, int ld_out, int B, int T, int D, int DP, int shift,
                          float a, float s, uint64_t seed, uint64_t row0, hipStream_t st);
// dst[(slot[b] or b), j, c] <- src[b, j, c], c < D: the padded loop state (B, T, DP) into rows of an unpadded (n_slots, T, D) table
int unpad_rows_index_launch(const float* src, float* dst, const int32_t* slot_dev, int B, int T, int D, int DP, hipStream_t st);

// ---- constrained planning (constrain.hip) -------------------------------------------------------------------
int check_constrain_mode(int mode);              // LDP_EINVAL unless LDP_CONSTRAIN_CLAMP / LDP_CONSTRAIN_REPAINT
// level j in 0 .. n_steps: (a, s) = warm_coefs at t_j for j < n_steps, exactly (1, 0) at j = n_steps; LDP_EINVAL names `level` outside
int level_coefs(int n_train, int n_steps, int level, float* a, float* s);
// the same over a registered timestep table ts (sampler 2): level j < n_steps has the timestep ts[j], level n_steps is exactly (1, 0)
int table_level_coefs(int n_train, const std::vector<int32_t>& ts, int level, float* a, float* s);
// out <- mask != 0 ? (noise ? fma(a, target, rn(s * z)) : target) : x, all four with row stride ld; z = philox_normal(seed, (row0 + r) * DP
// + c, level, LDP_PHILOX_STREAM_CONSTRAIN) with (seed, row0) read from `ctl` when it is given (captured loops), else the arguments
int plan_constrain_launch(const float* x, const float* target, const uint8_t* mask, float* out, int ld, int64_t rows, int D, int DP, float a,
                          float s, int level, bool noise, const uint64_t* ctl, uint64_t seed, uint64_t row0, hipStream_t st);
// target / mask (B, T, D) in caller memory -> P.ctarget / P.cmask (Bg, T, DP), zero beyond D and beyond the B real rows (eager, one launch;
// the buffers grow with the workspace and drop the captured graphs when they move)
int constrain_stage(ldp_handle* h, const float* target, const uint8_t* mask, int B, int Bg, hipStream_t st);
// C_level on the loop state, read from the staged buffers and the planner's control block: one launch, counted in last_total_launches
int planner_constrain_level(ldp_handle* h, int Bg, const LoopSpec& L, int level, hipStream_t q);
// ---- DPM-Solver++(2M) sampler (solver.hip) -------------------------------------------------------------------
const SolverTable* solver_table(const ldp_handle* h, int n_steps);      // the table registered for n_steps, or nullptr
void make_solver_coefs(int n_train, const std::vector<int32_t>& ts, std::vector<SolverCoef>& out);
// P.solver_eps / P.solver_x0 for Bg rows (they grow with the workspace and drop the captured graphs when they move)
int solver_workspace(ldp_handle* h, int Bg);
// ---- guided planning (guide.hip) ----------------------------------------------------------------------------
// A call's guide as the sampling entry points receive it: target, wg (B, T, D) and anchor (B, D; nullptr: no continuity term) in device
// memory, lam, beta, lo, hi (D) and rho (n_rho) on the host.
struct GuideSpec {
  const float* target; const float* wg; const float* anchor;
  const float* lam; const float* beta; const float* lo; const float* hi;
  const float* rho; int n_rho;
};
// LDP_EINVAL naming the argument: sampler 2, a missing array, n_rho != n_steps, a negative or non-finite lam / beta / rho, lo > hi
int check_guide(const GuideSpec* g, int D, int n_steps, int sampler);
// the guide into the handle's buffers, padded like the loop state (eager: pad launches and one host copy; the buffers grow with the
// workspace and drop the captured graphs when they move)
int guide_stage(ldp_handle* h, const GuideSpec& g, int B, int Bg, hipStream_t st);
// what the guide kernels and the staged column block P.gcol are laid out for: one sample's data prediction in 8 KB of LDS, [lam | beta |
// lo | hi] at PLAN_MAX_D floats each, then up to PLAN_MAX_STEPS step sizes (check_sampler: a loop has at most 4094 steps)
constexpr int PLAN_MAX_T = 16, PLAN_MAX_D = 128, PLAN_MAX_STEPS = 4096;
int check_guide_shape(int T, int D);            // LDP_EINVAL unless 1 <= T <= PLAN_MAX_T and 1 <= D <= PLAN_MAX_D
// ---- composed planning (compose.hip) ------------------------------------------------------------------------
// Everything one launch of plan_compose_step_kernel reads, by value.  Pointers are device memory.
//   x / x_out (B, T, ldx), h_prev / h_out (B, T, ldx: the solver's history, SAMPLER 1 only), eps / noise (B, T, D),
//   g_target / g_wg (B, T, ldg), g_anchor (B, ldg) or nullptr, lam / beta / lo / hi (D), rho (entry `step` is read),
//   c_target (B, T, ldc) float, c_mask (B, T, ldc) bytes.
// Coefficients: s / inv_a of the data prediction; SAMPLER 0: c_y = c_x0, c_x, c_eps, sigma; SAMPLER 1: c_y = c_D, c_x, w.
// (ca, cs): the constraint's level coefficients of level step + 1; c_noise: repaint and that level is not the last.
struct ComposeArgs {
  const float* x; float* x_out; const float* eps; const float* noise; const float* h_prev; float* h_out;
  const float* g_target; const float* g_wg; const float* g_anchor; const float* lam; const float* beta; const float* lo; const float* hi;
  const float* rho;
  const float* c_target; const uint8_t* c_mask;
  const uint64_t* ctl; uint64_t seed, row0;
  int ldx, ldg, ldc, B, T, D, DP, step, second, c_noise;
  float s, inv_a, c_y, c_x, c_eps, sigma, w, ca, cs;
};
void set_scheduler_coefs(ComposeArgs& A, const StepCoef& k);      // a DDPM / DDIM step's row into A
void set_solver_coefs(ComposeArgs& A, const SolverCoef& k);       // a sampler-2 step's row into A
// one launch of the step kernel.  solver: SAMPLER 1; guide / constrain: which parts A carries (a guide: check_guide_shape first)
int plan_compose_launch(const ComposeArgs& A, bool solver, bool guide, bool constrain, hipStream_t st);
// (a, s) of constraint level `level` under `sampler`: level_coefs on the uniform grid, table_level_coefs of the registered table under sampler 2
int compose_level_coefs(const ldp_handle* h, int sampler, int n_steps, int level, float* a, float* s);
// C_level on the loop state in front of a stepped loop: planner_constrain_level, or its table-level counterpart under sampler 2; one launch, counted
int planner_constrain_begin(ldp_handle* h, int Bg, const LoopSpec& L, int level, hipStream_t q);
// step i of a stepped loop on the loop state: eps from P.solver_eps, the guide / constraint from the staged buffers as L names them, the
// history in P.solver_x0; k (DDPM / DDIM) or ks (sampler 2) is the step's coefficient row; one launch, counted
int planner_compose_step(ldp_handle* h, int Bg, const LoopSpec& L, const StepCoef* k, const SolverCoef* ks, const float* noise, int i,
                         bool second, hipStream_t q);
}  // namespace ldp
