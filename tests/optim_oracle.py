"""The optimiser of csrc/train.hip restated on the CPU: Adam, the parameter EMA and the global gradient norm, in float64 (the reference) and in
float32 with every operation rounded once (the `err32` restatement of DESIGN 4.11), plus the states the per-element tests run them on and
the error measures both are held to.  Plain numpy: no torch, no GPU.

One float64 definition of Adam stays: `adam_step64` calls `oracle.train.adam_apply`.

Conventions: `count` is the number of THIS step (1 = the first apply, the exponent of the bias corrections); every state array is a float32
array (what the arenas hold); `lr` is the float32 value the kernel receives; b1 / b2 / eps / the EMA decay are Python doubles, as optax and
flax receive them."""
import functools
from collections import OrderedDict

import numpy as np

from oracle import train as OT

F32, F64 = np.float32, np.float64
B1, B2, EPS = 0.9, 0.999, 1e-8
U24 = 2.0 ** -24                                           # half a float32 ulp, relative: one rounding
K_OPS = dict(mu=3, nu=4, update=8, ema=3)                  # rounded operations on each quantity's path
TINY32 = float(np.finfo(F32).tiny)
POOL = 1 << 15                                             # distinct element states; an arena draws its elements from them (`pool_index`)
SPECIAL = 2048                                             # elements per special block of `reachable_state`
# what tests/test_hip_optimizer.py runs (tests/test_optim_oracle_cpu.py holds the generator's promises for exactly these)
COUNTS = (1, 2, 10, 1000, 500000)
LRS = (1e-4, 1e-6, 0.0)
STATE_SEED = {c: 100 + i for i, c in enumerate(COUNTS)}
STATE_SEED.update({7: 120, 8: 121})                        # the count tests
TRAJ_SEED, TRAJ_STEPS, TRAJ_LR, TRAJ_DECAY = 140, 300, 1e-4, 0.999


# ---- float64 ---------------------------------------------------------------------------------------------------------------------------
def adam_step64(p, g, mu, nu, lr, count, b1=B1, b2=B2, eps=EPS):
    """One optax.adam step in float64 on the float32 inputs widened -> dict(p, mu, nu, du): du = -lr * u, p = p_old + du."""
    zero = OrderedDict(x=np.zeros(np.shape(g), F64))
    state = dict(mu=OrderedDict(x=np.asarray(mu, F64)), nu=OrderedDict(x=np.asarray(nu, F64)), count=int(count) - 1)
    new, st = OT.adam_apply(zero, OrderedDict(x=np.asarray(g, F64)), state, lambda c: float(F32(lr)), b1=b1, b2=b2, eps=eps)
    assert st["count"] == count
    du = new["x"]                                          # 0 + step_size * u: the product itself
    return dict(p=np.asarray(p, F64) + du, mu=st["mu"]["x"], nu=st["nu"]["x"], du=du)


def ema64(e, p_new, d):
    """TrainStateEMA.apply_ema: e * d + p_new * (1 - d)."""
    return np.asarray(e, F64) * d + np.asarray(p_new, F64) * (1.0 - d)


def grad_norm64(g):
    g = np.asarray(g, F64).reshape(-1)
    return float(np.sqrt(np.dot(g, g)))


# ---- float32, every operation rounded once, optax's order ----------------------------------------------------------------------------------
def adam_step32(p, g, mu, nu, lr, count, b1=B1, b2=B2, eps=EPS):
    """update_moment, bias_correction, mu_hat / (sqrt(nu_hat) + eps), scale(-lr), apply_updates with float32 arrays; the scalars 1 - b,
    1 - b**count are formed in double and rounded once (a Python double meets a float32 array as a weak type)."""
    p, g, mu, nu = (np.asarray(a, F32) for a in (p, g, mu, nu))
    b1f, b2f, omb1, omb2 = F32(b1), F32(b2), F32(1.0 - b1), F32(1.0 - b2)
    bc1, bc2 = F32(1.0 - b1 ** int(count)), F32(1.0 - b2 ** int(count))
    m = omb1 * g + b1f * mu
    v = omb2 * (g * g) + b2f * nu
    u = (m / bc1) / (np.sqrt(v / bc2) + F32(eps))
    du = F32(-F32(lr)) * u
    out = dict(p=p + du, mu=m, nu=v, du=du)
    assert all(a.dtype == F32 for a in out.values())
    return out


def ema32(e, p_new, d):
    return np.asarray(e, F32) * F32(d) + np.asarray(p_new, F32) * F32(1.0 - d)


def _wave_tree32(x):
    """Sum over the last axis (a power of two) in float32 by halving: a fixed-order tree, as a wave reduction is."""
    while x.shape[-1] > 1:
        h = x.shape[-1] // 2
        x = x[..., :h] + x[..., h:]
    return x[..., 0]


def grad_norm32_striped(g):
    """The kernel's own decomposition: float32 sum of squares per 1024-element stripe (four strided elements per thread, a tree over the
    256 threads), the stripes' sums added in double, the square root in double, the result rounded to float32."""
    g = np.asarray(g, F32).reshape(-1)
    nb = (g.size + 1023) // 1024
    x = np.zeros(nb * 1024, F32)
    x[:g.size] = g
    x = x.reshape(nb, 4, 256)
    s = np.zeros((nb, 256), F32)
    for u in range(4):
        s = s + x[:, u] * x[:, u]
    part = _wave_tree32(s)
    assert part.dtype == F32
    return float(F32(np.sqrt(part.astype(F64).sum())))


# ---- states ----------------------------------------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


class GradStream:
    """A synthetic gradient stream over n elements, float32.  Element i has a scale s_i, log-uniform in 1e-10 .. 1e2, and a sign; step t
    gives g_i = sign_i * s_i * max(|1 + 0.6 z_ti|, 1e-3): noisy over three decades and never of the other sign, so that (1 - b1) g + b1 mu
    adds like signs and the relative error of mu -- hence of the update -- is the roundings' and not a cancellation's (a stream of mixed
    signs cancels to 1e-4 of its terms in some element of 32768, and 3 * err32 would then bound nothing).  Opposite signs are what the
    third special block is for, where the cancellation is a fixed factor below 4.  The last 3 * SPECIAL elements:
      [n - 3S, n - 2S)  never touched: g = 0 at every step (mu = nu = 0)
      [n - 2S, n - S)   the gradient is exactly 0 from step `zero_from` on (non-zero moments behind it)
      [n - S, n)        sign-alternating: g = s * (1 + 0.02 z) * (+1 at even t, -3 at odd t).  Unequal magnitudes, because +-s would cancel
                        19-fold at step 2 (0.1 g_2 against 0.09 g_1); with these the terms of mu cancel at most 4-fold at any step"""
    NZ = 61

    def __init__(self, n, seed, zero_from):
        assert n > 4 * SPECIAL
        g = _rng(seed)
        self.n, self.zero_from = n, int(zero_from)
        self.scale = 10.0 ** g.uniform(-10.0, 2.0, n)
        self.sign = np.where(g.random(n) < 0.5, -1.0, 1.0)
        self.z = g.standard_normal((self.NZ, n))
        self.amp = g.uniform(0.5, 1.0, 257)
        S = SPECIAL
        self.never, self.zeroed, self.alt = slice(n - 3 * S, n - 2 * S), slice(n - 2 * S, n - S), slice(n - S, n)

    def __call__(self, t):
        z = self.z[t % self.NZ] * self.amp[t % 257]
        x = self.sign * self.scale * np.maximum(np.abs(1.0 + 0.6 * z), 1e-3)
        x[self.alt] = (-3.0 if t & 1 else 1.0) * self.scale[self.alt] * (1.0 + 0.02 * np.clip(z[self.alt], -3.0, 3.0))
        x[self.never] = 0.0
        if t >= self.zero_from:
            x[self.zeroed] = 0.0
        g32 = x.astype(F32)
        g2 = g32 * g32
        assert np.all((g32 == 0) | (g2 >= TINY32)), "a squared gradient is subnormal in float32"
        return g32


def _trained_like_p(n, seed):
    g = _rng(seed)
    return (np.where(g.random(n) < 0.5, -1.0, 1.0) * np.clip(10.0 ** g.normal(-1.5, 1.0, n), 1e-4, 10.0)).astype(F32).astype(F64)


@functools.lru_cache(maxsize=None)
def reachable_state(n, count, seed):
    """The state in front of Adam step `count`: min(count - 1, 3000) float64 Adam steps (lr 1e-4) over GradStream(n, seed) from zero moments
    and trained-like parameters -> dict(p, mu, nu, g) of float32 arrays, g the next gradient, `stream`, and `steps`.  mu and nu are what
    the stream left, so |mu| / sqrt(nu) is bounded as it is in training; independent random moments are not reachable and make the update
    meaningless.  Computed once per (n, count, seed), shared, never modified (the arrays are read-only)."""
    steps = min(int(count) - 1, 3000)
    stream = GradStream(n, seed, zero_from=steps)
    p, mu, nu = _trained_like_p(n, seed + 1), np.zeros(n, F64), np.zeros(n, F64)
    first = int(count) - steps
    for t in range(steps):
        r = adam_step64(p, stream(t), mu, nu, 1e-4, first + t)
        p, mu, nu = r["p"], r["mu"], r["nu"]
    out = dict(p=p.astype(F32), mu=mu.astype(F32), nu=nu.astype(F32), g=stream(steps))
    check_state(out, stream, steps, int(count))
    for a in out.values():
        a.setflags(write=False)
    out.update(stream=stream, steps=steps)
    return out


def check_state(st, stream, steps, count, b1=B1, b2=B2):
    """What the generator promises (asserted on every state it returns)."""
    g, mu, nu = st["g"], st["mu"], st["nu"]
    assert all(st[k].dtype == F32 and np.isfinite(st[k]).all() for k in ("p", "g", "mu", "nu"))
    assert np.all((nu == 0) | (nu >= TINY32)), "a second moment is subnormal in float32"
    assert np.all((g == 0) | (g * g >= TINY32)), "a squared gradient is subnormal in float32"
    assert np.all(nu >= 0)
    assert not g[stream.never].any() and not mu[stream.never].any() and not nu[stream.never].any()
    assert not g[stream.zeroed].any()
    live = np.ones(g.size, bool)
    live[stream.never] = live[stream.zeroed] = False
    assert np.all(g[live] != 0)
    if steps > 0:
        assert np.all(mu[stream.zeroed] != 0) and np.all(nu[stream.zeroed] > 0)
        assert np.all(nu[live] > 0)
        ratio = (np.abs(mu[nu > 0].astype(F64)) / (1.0 - b1 ** (count - 1))) / np.sqrt(nu[nu > 0].astype(F64) / (1.0 - b2 ** (count - 1)))
        assert ratio.max() <= 4.0, ratio.max()               # |mu_hat| / sqrt(nu_hat): of order 1 on a reachable state
    else:
        assert not mu.any() and not nu.any()
    if steps >= 2:
        a = stream.alt
        assert np.all(np.sign(g[a]) == -np.sign(stream(steps - 1)[a]))


def pool_index(sizes, n, seed):
    """{leaf: indices into the pool of n element states} for leaves of the given element counts: every pool element is used, in a seeded
    order (an arena larger than the pool repeats it; the kernels are element-wise, so equal inputs must give equal bits)."""
    g = _rng(seed)
    total = int(sum(sizes.values()))
    idx = np.concatenate([g.permutation(n) for _ in range((total + n - 1) // n)])[:total]
    out, o = OrderedDict(), 0
    for k, s in sizes.items():
        out[k] = idx[o:o + int(s)]
        o += int(s)
    return out


# ---- error measures (the issue's section 2 (a)) ----------------------------------------------------------------------------------------------
def ulp32(x):
    """The float32 ulp at each float64 value (0 at 0)."""
    a = np.abs(np.asarray(x, F64))
    _, e = np.frexp(a)
    return np.where(a > 0, np.ldexp(1.0, np.maximum(e - 1, -126) - 23), 0.0)


def _rel(err, denom):
    """-> (worst err / denom where denom > 0, number of entries with denom == 0 and err != 0)."""
    zero = denom == 0
    worst = float((err[~zero] / denom[~zero]).max()) if (~zero).any() else 0.0
    return worst, int(np.count_nonzero(err[zero]))


def step_errors(got, ref, st, b1=B1):
    """got: dict(p, mu, nu) of float32 results of one step from state st (dict p, g, mu, nu) whose float64 result is ref ->
    {quantity: (worst measure, entries that had to be exact and are not)}.
      nu      |got - ref| / ref                                  (every term is non-negative; got == 0 where ref == 0)
      mu      |got - ref| / ((1 - b1)|g| + b1 |mu_old|)
      update  (|got_p - ref_p| - ulp32(ref_p) / 2)+ / |du64|     (the rounding of p itself is not the update's error)"""
    a64 = lambda x: np.asarray(x, F64)
    out = {}
    out["nu"] = _rel(np.abs(a64(got["nu"]) - ref["nu"]), ref["nu"])
    out["mu"] = _rel(np.abs(a64(got["mu"]) - ref["mu"]), (1.0 - b1) * np.abs(a64(st["g"])) + b1 * np.abs(a64(st["mu"])))
    excess = np.maximum(np.abs(a64(got["p"]) - ref["p"]) - 0.5 * ulp32(ref["p"]), 0.0)
    out["update"] = _rel(excess, np.abs(ref["du"]))
    return out


def ema_error(got, e_old, p_new, d):
    """|got - ema64(e_old, p_new)| / (d |e| + (1 - d) |p_new|) -> (worst, entries that had to be exact and are not).  p_new is the float32
    parameter array the EMA was formed from (the step's own output, widened): what the parameters inherit from the update is measured on
    the parameters, and p_old + du may cancel to a p_new that is small against its own rounding."""
    ref = ema64(e_old, p_new, d)
    return _rel(np.abs(np.asarray(got, F64) - ref), d * np.abs(np.asarray(e_old, F64)) + (1.0 - d) * np.abs(np.asarray(p_new, F64)))


def bound(quantity, err32):
    """max(k * 2^-24, 3 * err32): k roundings for a kernel that may contract a * b + c, three times the float32 restatement's own error."""
    return max(K_OPS[quantity] * U24, 3.0 * err32)


@functools.lru_cache(maxsize=None)
def trajectory(n=POOL, seed=TRAJ_SEED, steps=TRAJ_STEPS, lr=TRAJ_LR, decay=TRAJ_DECAY):
    """`steps` Adam + EMA steps from zero moments over GradStream(n, seed) (its second block goes to zero half-way), once in float64 and
    once in the float32 restatement -> dict(p0, stream, r64 = dict(p, mu, nu, ema), r32 = the same).  Shared, never modified."""
    stream = GradStream(n, seed, zero_from=steps // 2)
    p0 = _trained_like_p(n, seed + 1).astype(F32)
    a = dict(p=p0.astype(F64), mu=np.zeros(n, F64), nu=np.zeros(n, F64), ema=p0.astype(F64))
    b = dict(p=p0, mu=np.zeros(n, F32), nu=np.zeros(n, F32), ema=p0)
    for t in range(steps):
        g = stream(t)
        r = adam_step64(a["p"], g, a["mu"], a["nu"], lr, t + 1)
        a = dict(p=r["p"], mu=r["mu"], nu=r["nu"], ema=ema64(a["ema"], r["p"], decay))
        r = adam_step32(b["p"], g, b["mu"], b["nu"], lr, t + 1)
        b = dict(p=r["p"], mu=r["mu"], nu=r["nu"], ema=ema32(b["ema"], r["p"], decay))
    for d in (a, b):
        for x in d.values():
            x.setflags(write=False)
    p0.setflags(write=False)
    return dict(p0=p0, stream=stream, r64=a, r32=b)
