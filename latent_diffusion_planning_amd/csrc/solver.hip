// solver.hip -- DPM-Solver++(2M) on the clipped data prediction over a registered timestep table (include/ldp_hip.h "solver sampler",
// DESIGN.md 4.18): the table and its coefficient rows (host, float64 -> float32), the buffers a sampler-2 loop keeps (the evaluation's
// eps and the previous step's x0) and the stand-alone entry point.  The solver update itself -- one elementwise launch behind every
// U-Net evaluation of that loop -- is compose.hip's plan_compose_step_kernel<1, false, false>.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "engine.hpp"

namespace ldp {
const SolverTable* solver_table(const ldp_handle* h, int n_steps) {
  const auto it = h->solver_tabs.find(n_steps);
  return it == h->solver_tabs.end() ? nullptr : &it->second;
}

// the rows of schedule.solver_coefficients: float64 from the float32 abar table until the final cast
void make_solver_coefs(int n_train, const std::vector<int32_t>& ts, std::vector<SolverCoef>& out) {
  std::vector<float> betas, alphas, acp;
  betas_squaredcos(n_train, betas, alphas, acp);
  const int n = (int)ts.size();
  out.assign(n, SolverCoef{});
  auto lam = [&](int t) { const double a = acp[t]; return 0.5 * std::log(a / (1.0 - a)); };
  double h_prev = 0.0;
  for (int i = 0; i < n; ++i) {
    const int t = ts[i];
    const double ab_t = acp[t];
    const double a_t = std::sqrt(ab_t), s_t = std::sqrt(1.0 - ab_t);
    SolverCoef c{};
    c.t = (float)t;
    c.inv_a = (float)(1.0 / a_t);
    c.sg = (float)s_t;
    if (i == n - 1) {                              // to the clean level: alpha_s = 1, sigma_s = 0
      c.c_x = 0.0f; c.c_D = 1.0f; c.w = 0.0f;
    } else {
      const int s = ts[i + 1];
      const double ab_s = acp[s];
      const double a_s = std::sqrt(ab_s), s_s = std::sqrt(1.0 - ab_s);
      const double hh = lam(s) - lam(t);
      c.c_x = (float)(s_s / s_t);
      c.c_D = (float)(a_s - s_s * a_t / s_t);
      c.w = i > 0 ? (float)(hh / (2.0 * h_prev)) : 0.0f;
      h_prev = hh;
    }
    out[i] = c;
  }
}

int solver_workspace(ldp_handle* h, int Bg) {
  PlannerState& P = h->pl;
  const size_t rows = (size_t)std::max(Bg, (P.ws_B + 15) / 16 * 16) * P.T;      // (grows with the workspace, not call by call)
  if (rows * P.D * 4 > P.solver_eps.bytes || rows * P.DP * 4 > P.solver_x0.bytes) {
    if (P.solver_eps.p || P.solver_x0.p) drop_graphs(h);     // captured solver nodes point into these buffers
    LDP_TRY(P.solver_eps.alloc(rows * P.D * 4));
    LDP_TRY(P.solver_x0.alloc(rows * P.DP * 4));
    LDP_HIP(hipMemset(P.solver_x0.p, 0, P.solver_x0.bytes));      // (its padding columns are never written: keep them defined)
  }
  return LDP_OK;
}

}  // namespace ldp

using namespace ldp;

extern "C" {

int ldp_solver_timesteps(ldp_handle* h, const int32_t* ts_host, int32_t n_steps) {
  if (!h) return fail(LDP_EINVAL, "bad argument");
  const int n_train = h->cfg.planner_train_steps;
  if (n_steps < 1 || n_steps > n_train) return fail(LDP_EINVAL, "n_steps must be in 1..planner_train_steps = %d, got %d", n_train, n_steps);
  if (!ts_host) return fail(LDP_EINVAL, "ts is required");
  for (int i = 0; i < n_steps; ++i) {
    if (ts_host[i] < 0 || ts_host[i] >= n_train)
      return fail(LDP_EINVAL, "ts[%d] = %d outside 0..planner_train_steps-1 = %d", i, ts_host[i], n_train - 1);
    if (i > 0 && ts_host[i] >= ts_host[i - 1])
      return fail(LDP_EINVAL, "ts[%d] = %d does not lie below ts[%d] = %d: the table must be strictly decreasing", i, ts_host[i], i - 1,
                  ts_host[i - 1]);
  }
  if (ts_host[n_steps - 1] != 0) return fail(LDP_EINVAL, "ts[%d] = %d: the last entry must be 0", n_steps - 1, ts_host[n_steps - 1]);
  std::vector<int32_t> ts(ts_host, ts_host + n_steps);
  auto it = h->solver_tabs.find(n_steps);
  if (it != h->solver_tabs.end()) {
    if (it->second.ts == ts) return LDP_OK;                // the same table again: nothing to do
    drop_graphs(h);                                        // captured solver launches carry the old rows by value
  }
  SolverTable tab;
  tab.ts = ts;
  make_solver_coefs(n_train, tab.ts, tab.rows);
  h->solver_tabs[n_steps] = std::move(tab);
  return LDP_OK;
}

int ldp_plan_solver_step(ldp_handle* h, const float* x, const float* eps, const float* x0_prev, int32_t n_steps, int32_t step, float* x_out,
                         float* x0_out, int32_t B, void* stream) {
  if (!h || !x || !eps || !x_out || !x0_out) return fail(LDP_EINVAL, "bad argument");
  if (B < 1) return fail(LDP_EINVAL, "B must be >= 1, got %d", B);
  const SolverTable* tab = solver_table(h, n_steps);
  if (!tab) return fail(LDP_ESTATE, "no timestep table registered for n_steps = %d: call ldp_solver_timesteps first", n_steps);
  if (step < 0 || step >= n_steps) return fail(LDP_EINVAL, "step %d outside 0..n_steps-1 = %d", step, n_steps - 1);
  const int D = h->cfg.obs_dim, T = h->cfg.pred_horizon;      // (elementwise on caller memory: no weights needed)
  ComposeArgs A{};
  A.x = x; A.x_out = x_out; A.eps = eps; A.h_prev = x0_prev; A.h_out = x0_out;
  A.ldx = D; A.B = B; A.T = T; A.D = D; A.DP = (D + 31) / 32 * 32; A.step = step;
  A.second = x0_prev != nullptr && step < n_steps - 1 ? 1 : 0;
  set_solver_coefs(A, tab->rows[step]);
  return plan_compose_launch(A, true, false, false, (hipStream_t)stream);
}

}  // extern "C"
