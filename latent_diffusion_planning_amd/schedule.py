"""Noise-schedule and timestep-embedding constant tables (host side, numpy).

These are weight-independent constants, built once on the host exactly the way the
reference builds its scheduler state (python float64 loop -> float32 arrays) and then
uploaded to HBM; the kernels only index them.

Reference anchors:
  * FlaxDDPMScheduler(num_train_timesteps=100, beta_schedule='squaredcos_cap_v2',
    clip_sample=True, prediction_type='epsilon')      agent/ldp_agent.py:637-650
    (diffusers==0.27.2, restated in SURVEY.md Appendix A.2)
  * SinusoidalPosEmb                                    networks/diffusion_nets_v2.py:21-31
  * FourierFeatures(learnable=False)                    networks/diffusion.py:7-22
  * DDIM (eta=0) is defined by this repository; the reference has no DDIM.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

SAMPLER_DDPM = 0
SAMPLER_DDIM = 1


def betas_squaredcos_cap_v2(n: int, max_beta: float = 0.999) -> np.ndarray:
    def alpha_bar(t: float) -> float:
        return math.cos((t + 0.008) / 1.008 * math.pi / 2.0) ** 2
    b = [min(1.0 - alpha_bar((i + 1) / n) / alpha_bar(i / n), max_beta) for i in range(n)]
    return np.asarray(b, dtype=np.float32)


@dataclass(frozen=True)
class NoiseSchedule:
    betas: np.ndarray            # (n,) f32
    alphas: np.ndarray           # (n,) f32
    alphas_cumprod: np.ndarray   # (n,) f32

    @property
    def n(self) -> int:
        return int(self.betas.shape[0])


def make_schedule(n_train: int = 100) -> NoiseSchedule:
    betas = betas_squaredcos_cap_v2(n_train)
    alphas = (np.float32(1.0) - betas).astype(np.float32)
    ac = np.cumprod(alphas, dtype=np.float32)
    return NoiseSchedule(betas, alphas, ac)


# Per-step coefficient rows consumed by the fused sampler epilogue.  One row per *executed*
# step i (i = 0 is the first, noisiest step).  Row layout (8 floats):
#   0: t (timestep index fed to the eps-model, as float)      1: 1/sqrt(abar_t)
#   2: sqrt(1-abar_t)                                          3: c_x0  (weight of clipped x0)
#   4: c_x   (weight of x_t; 0 for DDIM)                       5: c_eps (weight of eps; 0 for DDPM)
#   6: sigma (noise scale; 0 at t==0 and for DDIM)             7: unused
COEF_STRIDE = 8


def step_timesteps(n_train: int, n_steps: int, sampler: int) -> np.ndarray:
    """Timesteps visited, first executed step first."""
    if sampler == SAMPLER_DDPM:
        if n_steps != n_train:
            raise ValueError("the reference DDPM sampler visits every training timestep "
                             f"(n_steps must equal {n_train}, got {n_steps})")
        return np.arange(n_train - 1, -1, -1, dtype=np.int64)
    if n_train % n_steps != 0:
        raise ValueError(f"DDIM needs n_steps | n_train ({n_steps} vs {n_train})")
    stride = n_train // n_steps
    return (np.arange(n_steps - 1, -1, -1, dtype=np.int64) * stride)


def step_coefficients(sched: NoiseSchedule, n_steps: int, sampler: int) -> np.ndarray:
    ts = step_timesteps(sched.n, n_steps, sampler)
    ac = sched.alphas_cumprod.astype(np.float64)
    out = np.zeros((len(ts), COEF_STRIDE), dtype=np.float64)
    stride = sched.n // n_steps
    for i, t in enumerate(ts):
        a_t = ac[t]
        out[i, 0] = float(t)
        out[i, 1] = 1.0 / math.sqrt(a_t)
        out[i, 2] = math.sqrt(1.0 - a_t)
        if sampler == SAMPLER_DDPM:
            a_prev = ac[t - 1] if t > 0 else 1.0
            beta = float(sched.betas[t])
            alpha = float(sched.alphas[t])
            out[i, 3] = math.sqrt(a_prev) * beta / (1.0 - a_t)
            out[i, 4] = math.sqrt(alpha) * (1.0 - a_prev) / (1.0 - a_t)
            var = max((1.0 - a_prev) / (1.0 - a_t) * beta, 1e-20)
            out[i, 6] = math.sqrt(var) if t > 0 else 0.0
        else:
            tp = t - stride
            a_prev = ac[tp] if tp >= 0 else 1.0
            out[i, 3] = math.sqrt(a_prev)
            out[i, 5] = math.sqrt(1.0 - a_prev)
    return out.astype(np.float32)


# ---- DPM-Solver++(2M) on a registered timestep table (csrc/solver.hip) ------------------------------------------
SAMPLER_DPMPP = 2


def log_snr(sched: NoiseSchedule) -> np.ndarray:
    """lambda_t = 1/2 log(abar_t / (1 - abar_t)), float64 from the float32 abar table."""
    ac = sched.alphas_cumprod.astype(np.float64)
    return 0.5 * np.log(ac / (1.0 - ac))


def solver_timesteps(n_train: int, n_steps: int, spacing: str = "logsnr", t_first=None) -> np.ndarray:
    """The timesteps a solver loop of n_steps visits, first executed step first: int64 (n_steps,), strictly decreasing, from t_first
    (default n_train - max(1, n_train // n_steps): DDIM's first timestep when n_steps | n_train) down to 0.  'uniform' is DDIM's grid;
    'logsnr' takes n_steps points linearly spaced in lambda from lambda(t_first) to lambda(0), maps each to the timestep with the
    nearest lambda (ties to the lower timestep) and then forces the table strictly decreasing and long enough to reach 0."""
    n_train, n_steps = int(n_train), int(n_steps)
    if n_steps < 1:
        raise ValueError(f"n_steps must be >= 1, got {n_steps}")
    if spacing == "uniform":
        if n_train % n_steps != 0:
            raise ValueError(f"the uniform grid needs n_steps | n_train ({n_steps} vs {n_train})")
        if t_first is not None and int(t_first) != n_train - n_train // n_steps:
            raise ValueError(f"the uniform grid starts at {n_train - n_train // n_steps}, got t_first = {t_first}")
        return step_timesteps(n_train, n_steps, SAMPLER_DDIM)
    if spacing != "logsnr":
        raise ValueError(f"spacing must be 'logsnr' or 'uniform', got {spacing!r}")
    t_first = n_train - max(1, n_train // n_steps) if t_first is None else int(t_first)
    if not 0 <= t_first < n_train:
        raise ValueError(f"t_first must lie in 0..{n_train - 1}, got {t_first}")
    if n_steps > t_first + 1:
        raise ValueError(f"n_steps = {n_steps} distinct timesteps do not fit into t_first = {t_first} .. 0")
    if n_steps == 1:
        if t_first != 0:
            raise ValueError(f"a one-step table is [0]: t_first must be 0, got {t_first}")
        return np.zeros(1, dtype=np.int64)
    lam = log_snr(make_schedule(n_train))
    ts = np.zeros(n_steps, dtype=np.int64)
    for i, p in enumerate(np.linspace(lam[t_first], lam[0], n_steps)):
        ts[i] = int(np.argmin(np.abs(lam - p)))            # (argmin returns the first, i.e. the lower, timestep of a tie)
    ts[0], ts[-1] = t_first, 0
    for i in range(1, n_steps):
        ts[i] = max(min(ts[i], ts[i - 1] - 1), n_steps - 1 - i)
    return ts


def solver_coefficients(sched: NoiseSchedule, ts, dtype=np.float32) -> np.ndarray:
    """float32 (n, 8) rows of the solver kernel: [t, 1/alpha_t, sigma_t, c_x = sigma_s / sigma_t, c_D = alpha_s - sigma_s alpha_t /
    sigma_t, w = h_i / (2 h_{i-1}), 0, 0] for the step from t = ts[i] to s = ts[i+1]; the last step goes to the clean level (alpha_s = 1,
    sigma_s = 0: c_x = 0, c_D = 1).  w = 0 in row 0 and in the last row.  float64 until the final cast (dtype=np.float64: no cast)."""
    ts = np.asarray(ts, dtype=np.int64)
    n = len(ts)
    ac = sched.alphas_cumprod.astype(np.float64)
    lam = log_snr(sched)
    out = np.zeros((n, COEF_STRIDE), dtype=np.float64)
    h_prev = 0.0
    for i, t in enumerate(ts):
        a_t, s_t = math.sqrt(ac[t]), math.sqrt(1.0 - ac[t])
        out[i, 0] = float(t)
        out[i, 1] = 1.0 / a_t
        out[i, 2] = s_t
        if i == n - 1:
            out[i, 3], out[i, 4] = 0.0, 1.0
            continue
        s = ts[i + 1]
        a_s, s_s = math.sqrt(ac[s]), math.sqrt(1.0 - ac[s])
        h = lam[s] - lam[t]
        out[i, 3] = s_s / s_t
        out[i, 4] = a_s - s_s * a_t / s_t
        if i > 0:
            out[i, 5] = h / (2.0 * h_prev)
        h_prev = h
    return out.astype(dtype)


def _freqs(dim: int) -> np.ndarray:
    """exp(-j * ln(1e4)/(half-1)), evaluated in float32 like the reference's traced graph."""
    half = dim // 2
    step = np.float32(np.log(np.float32(10000.0))) / np.float32(half - 1)
    return np.exp(np.arange(half, dtype=np.float32) * -step).astype(np.float32)


def sinusoidal_table(n: int, dim: int, cos_first: bool) -> np.ndarray:
    """(n, dim) rows for timesteps 0..n-1.  cos_first=False: planner [sin | cos];
    cos_first=True: IDM FourierFeatures [cos | sin]."""
    f = _freqs(dim)
    arg = (np.arange(n, dtype=np.float32)[:, None] * f[None, :]).astype(np.float32).astype(np.float64)
    s, c = np.sin(arg), np.cos(arg)
    tab = np.concatenate([c, s], -1) if cos_first else np.concatenate([s, c], -1)
    return tab.astype(np.float32)


# ---- learning-rate schedule of the training step ---------------------------------------------------------------------------------
def warmup_cosine_decay_schedule(init_value: float, peak_value: float, warmup_steps: int, decay_steps: int, end_value: float,
                                 exponent: float = 1.0):
    """optax 0.2.2 `warmup_cosine_decay_schedule` (the reference's `lr_schedule`, agent/ldp_agent.py:583-589, 621-627) as a host function
    count -> learning rate: join_schedules([linear_schedule(init, peak, warmup_steps), cosine_decay_schedule(peak, decay_steps -
    warmup_steps, alpha = end / peak, exponent)], [warmup_steps]).  optax evaluates it in float32 inside the traced step; here float64 on the
    host, rounded to float32 when it is handed to the Adam kernel."""
    alpha = 0.0 if peak_value == 0.0 else end_value / peak_value
    cos_steps = decay_steps - warmup_steps
    if cos_steps <= 0:
        raise ValueError("The cosine_decay_schedule requires positive decay_steps!")          # (optax's own message)

    def schedule(count) -> float:
        count = int(count)
        if count < warmup_steps:                                       # linear_schedule = polynomial_schedule(power=1)
            frac = 1.0 - min(max(count, 0), warmup_steps) / warmup_steps
            return (init_value - peak_value) * frac + peak_value
        c = min(count - warmup_steps, cos_steps)
        decayed = (1.0 - alpha) * (0.5 * (1.0 + math.cos(math.pi * c / cos_steps))) ** exponent + alpha
        return peak_value * decayed
    return schedule
