"""HipEngine: PyTorch-ROCm tensors in, libldp_hip.so (hand-written gfx950 kernels) out.

torch is plumbing here -- device memory, the current stream, `torch.distributed` -- the
arithmetic of the hot path all happens inside the C-ABI calls.  Every method enqueues on
`torch.cuda.current_stream()` and returns without synchronising.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import (LDPHipError, LDPHipFault, LdpConfig, MOD_ENCODER, MOD_IDM, MOD_PLANNER, MOD_VAE, RESNET_FEATURES, RESNET_SLOTS,
                   SAMPLER_DDIM, SAMPLER_DDPM, SAMPLER_DPMPP, check)
from .schedule import solver_timesteps

_SAMPLERS = {"ddpm": SAMPLER_DDPM, "ddim": SAMPLER_DDIM, "dpmpp": SAMPLER_DPMPP}
_CONSTRAIN_MODES = {"clamp": _lib.CONSTRAIN_CLAMP, "repaint": _lib.CONSTRAIN_REPAINT}


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _f32(t, device) -> torch.Tensor:
    if not torch.is_tensor(t):
        t = torch.as_tensor(np.asarray(t, dtype=np.float32))
    return t.to(device=device, dtype=torch.float32).contiguous()


def _opt_f32(t, device) -> Optional[torch.Tensor]:
    return None if t is None else _f32(t, device)


def _u64(seed: int):
    return C.c_uint64(seed & (2**64 - 1))


def _want(name: str, t: Optional[torch.Tensor], shape) -> None:
    """Raw pointers cross the C ABI next: a wrong shape would be an out-of-bounds device read there,
    where the JAX reference raises a shape error."""
    if t is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")


def check_candidate_range(B: int, N: int, K: int, c0: int = 0, n_loc: Optional[int] = None, bandwidth: Optional[float] = None) -> None:
    """The argument rules of the best-of-N calls (include/ldp_hip.h), raised here with the argument's name before a pointer crosses
    the ABI: B observations, N candidates of K floats each, of which this call handles [c0, c0 + n_loc)."""
    n_loc = N - c0 if n_loc is None else n_loc
    if B < 1:
        raise ValueError(f"B must be >= 1, got {B}")
    if N < 1:
        raise ValueError(f"n_candidates (N) must be >= 1, got {N}")
    if K < 1:
        raise ValueError(f"K must be >= 1, got {K}")
    if c0 < 0 or n_loc < 1 or c0 + n_loc > N:
        raise ValueError(f"candidate range c0 = {c0}, n_loc = {n_loc} must be non-empty and lie in 0..N = {N}")
    if bandwidth is not None and not (np.isfinite(bandwidth) and bandwidth > 0):
        raise ValueError(f"bandwidth must be finite and > 0, got {bandwidth}")


def _candidate_dims(x: torch.Tensor, B: int):
    """(N, K) of a candidate-major tensor (N * B, ...)."""
    B = int(B)
    if B < 1 or x.dim() < 2 or x.shape[0] < B or x.shape[0] % B:
        raise ValueError(f"candidates must have shape (N * B, ...) with B = {B}, got {tuple(x.shape)}")
    return x.shape[0] // B, int(np.prod(x.shape[1:]))


class HipEngine:
    """One `ldp_handle` on one GPU."""

    def __init__(self, *, obs_dim: int, action_dim: int, global_cond_dim: int, pred_horizon: int,
                 action_horizon: int, down_dims: Sequence[int] = (256, 512, 1024), kernel_size: int = 5,
                 n_groups: int = 8, step_embed_dim: int = 256, planner_train_steps: int = 100,
                 idm_train_steps: int = 100, idm_hidden: int = 256, idm_blocks: int = 3,
                 idm_time_dim: int = 256, image_size: int = 64, vae_latent_channels: int = 4,
                 device: Optional[torch.device] = None):
        self.lib = _lib.load()                     # raises loudly when the extension is missing
        if not torch.cuda.is_available():
            raise _lib.LDPHipUnavailable("no HIP device visible: the LDP hot path has no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        cfg = LdpConfig()
        cfg.obs_dim, cfg.action_dim, cfg.global_cond_dim = obs_dim, action_dim, global_cond_dim
        cfg.pred_horizon, cfg.action_horizon = pred_horizon, action_horizon
        cfg.n_levels = len(down_dims)
        for i, d in enumerate(down_dims):
            cfg.down_dims[i] = int(d)
        cfg.kernel_size, cfg.n_groups, cfg.step_embed_dim = kernel_size, n_groups, step_embed_dim
        cfg.planner_train_steps, cfg.idm_train_steps = planner_train_steps, idm_train_steps
        cfg.idm_hidden, cfg.idm_blocks, cfg.idm_time_dim = idm_hidden, idm_blocks, idm_time_dim
        cfg.image_size, cfg.vae_latent_channels = image_size, vae_latent_channels
        cfg.device = self.device.index or 0
        self.cfg = cfg
        self.D, self.A, self.G, self.T = obs_dim, action_dim, global_cond_dim, pred_horizon
        self.ah = action_horizon
        self.image_size, self.latent_channels = int(image_size), int(vae_latent_channels)
        self.planner_train_steps, self.idm_train_steps = planner_train_steps, idm_train_steps
        # version token of the parameter tree last uploaded per module (LDPAgent compares it with its
        # ParamState.version: agents sharing one engine can never run on each other's weights)
        self.loaded = {"planner": None, "idm": None, "vae": None}
        self.loaded.update({f"encoder{i}": None for i in range(RESNET_SLOTS)})      # the ResNet image encoders of DPAgent
        self.encoder_uploads = [0] * RESNET_SLOTS     # load_encoder calls per slot (tests: an unchanged encoder is not uploaded again)
        # likewise for the training arenas (ldp_train_*): the token of the ParamState they currently represent
        self.train_token = {"planner": None, "idm": None}
        # and of the EMA arenas (ldp_train_ema): the token of the EMA tree they hold
        self.train_ema_token = {"planner": None, "idm": None}
        self.ema_decay = {}                           # module -> decay of its EMA arena (train_ema)
        # fault bookkeeping for callers that keep results on the device: every sampling call gets a sequence
        # number; a detected fault marks every call enqueued so far as suspect (calls are asynchronous: the word
        # may have been set by any of them)
        self.call_seq = 0
        self.fault_upto = -1
        self.fault_kinds = 0                          # every kind of fault this handle ever reported (poll_fault_kinds)
        self.last_fault_kinds = 0
        self._bounds_cache = {}
        self.solver_tables = {}                       # n_steps -> the timestep table registered for sampler "dpmpp" (set_solver_timesteps)
        self._h = C.c_void_p()
        check(self.lib.ldp_create(C.byref(cfg), C.byref(self._h)))

    # -- lifecycle ------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.ldp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def load_params(self, planner: Optional[Dict[str, np.ndarray]] = None,
                    idm: Optional[Dict[str, np.ndarray]] = None,
                    vae: Optional[Dict[str, np.ndarray]] = None, versions: Optional[dict] = None) -> None:
        """Upload flat Flax-path parameter dicts and build the packed layouts / tables.
        versions: optional {module: token} recorded in `self.loaded` (None = anonymous upload)."""
        mods = 0
        for name, tree, bit in (("planner", planner, MOD_PLANNER), ("idm", idm, MOD_IDM),
                                ("vae", vae, MOD_VAE)):
            if tree is None:
                continue
            mods |= bit
            for path, arr in tree.items():
                a = np.ascontiguousarray(np.asarray(arr), dtype=np.float32)
                shape = (C.c_int64 * a.ndim)(*a.shape)
                check(self.lib.ldp_set_weight(self._h, f"{name}/{path}".encode(),
                                              a.ctypes.data_as(C.c_void_p), shape, a.ndim))
        with torch.cuda.device(self.device):
            check(self.lib.ldp_finalize(self._h, mods, self._stream()))
        for name, tree in (("planner", planner), ("idm", idm), ("vae", vae)):
            if tree is not None:
                self.loaded[name] = (versions or {}).get(name, object())

    # -- ResNet image encoders (csrc/resnet.hip) ---------------------------------------------------
    def load_encoder(self, slot: int, params: Dict[str, np.ndarray], version=None) -> None:
        """Upload one ResNetEncoder tree (weights.resnet_shapes) into weight module encoder<slot> and pack it.  Only the slots given since
        the last finalize are re-packed on the device side; `version` is recorded in self.loaded["encoder<slot>"]."""
        if not 0 <= int(slot) < RESNET_SLOTS:
            raise ValueError(f"encoder slot {slot}: a handle has slots 0..{RESNET_SLOTS - 1}")
        name = f"encoder{int(slot)}"
        for path, arr in params.items():
            a = np.ascontiguousarray(np.asarray(arr), dtype=np.float32)
            shape = (C.c_int64 * a.ndim)(*a.shape)
            check(self.lib.ldp_set_weight(self._h, f"{name}/{path}".encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim))
        self.loaded[name] = None
        with torch.cuda.device(self.device):
            check(self.lib.ldp_finalize(self._h, MOD_ENCODER, self._stream()))
        self.loaded[name] = version if version is not None else object()
        self.encoder_uploads[int(slot)] += 1

    def resnet_encode(self, slot: int, img_nhwc: torch.Tensor) -> torch.Tensor:
        """ResNetEncoder.apply of encoder<slot>: (N, 64, 64, 3) NHWC frames in [-1, 1] -> (N, 1024) = [expected_x | expected_y]."""
        img = _f32(img_nhwc, self.device)
        n = img.shape[0]
        _want("img_nhwc", img, (n, 64, 64, 3))
        out = torch.empty((n, RESNET_FEATURES), device=self.device, dtype=torch.float32)
        check(self.lib.ldp_resnet_encode(self._h, int(slot), _ptr(img), _ptr(out), n, self._stream()))
        self.call_seq += 1
        return out

    # -- options / fault protocol (include/ldp_hip.h) -----------------------------------------------
    def set_option(self, name: str, value: int) -> None:
        check(self.lib.ldp_set_option(self._h, name.encode(), C.c_int64(int(value))))

    def get_option(self, name: str) -> int:
        v = C.c_int64()
        check(self.lib.ldp_get_option(self._h, name.encode(), C.byref(v)))
        return int(v.value)

    def active_debug_options(self) -> str:
        """Names of the timing-ablation options that are set (results are wrong while any is)."""
        on = []
        if self.get_option("dbg"):
            on.append(f"dbg={self.get_option('dbg')}")
        if self.get_option("repeat") != 1:
            on.append(f"repeat={self.get_option('repeat')}")
        return ",".join(on)

    FAULT_EXCHANGE, FAULT_RANGE = 1, 2

    def poll_fault_kinds(self) -> int:
        """No stream is synchronised.  Bit mask of the faults recorded since the last poll (include/ldp_hip.h):
        FAULT_EXCHANGE -- a split work-group timed out on its peer (the handle now runs in safe mode);
        FAULT_RANGE -- an operand left the range of the two-fp16-plane convolutions (the handle now runs them on three
        bf16 planes, which have fp32's range).  Either way the results enqueued since the previous poll are invalid."""
        f = C.c_int32()
        check(self.lib.ldp_poll_fault(self._h, C.byref(f)))
        if f.value:
            self.fault_upto = self.call_seq
            self.fault_kinds |= int(f.value)
            self.last_fault_kinds = int(f.value)       # of the poll that marked the calls up to fault_upto suspect (the warning names THIS fault)
        return int(f.value)

    def poll_fault(self) -> bool:
        """True if any fault was recorded since the last poll: results enqueued since then must be recomputed."""
        return self.poll_fault_kinds() != 0

    def vae_encode_checked(self, img_nhwc: torch.Tensor) -> torch.Tensor:
        """vae_encode for callers that keep no CallRecord (bulk pre-encoding): synchronises, and when the range guard
        of the fp16-plane convolutions fired (an activation beyond 65504: the result holds inf / NaN) encodes again --
        the handle has switched to the bf16 planes by then."""
        for _ in range(3):
            out = self.vae_encode(img_nhwc)
            torch.cuda.current_stream(self.device).synchronize()
            if not self.poll_fault_kinds():
                return out
        raise RuntimeError("libldp_hip: vae_encode faulted three times in a row")

    # -- planner --------------------------------------------------------------------------------
    def unet_forward(self, x: torch.Tensor, k, cond: Optional[torch.Tensor]) -> torch.Tensor:
        x = _f32(x, self.device)
        B = x.shape[0]
        cond_t = None if cond is None else _f32(cond, self.device)
        _want("x", x, (B, self.T, self.D))
        _want("cond", cond_t, (B, self.G))
        eps = torch.empty_like(x)
        if torch.is_tensor(k) or isinstance(k, np.ndarray):
            kd = torch.as_tensor(k).to(device=self.device, dtype=torch.int32).reshape(-1)
            if kd.numel() == 1:
                kd = kd.expand(B)
            kd = kd.contiguous()
            check(self.lib.ldp_unet_forward(self._h, _ptr(x), _ptr(kd), 0, _ptr(cond_t), _ptr(eps), B,
                                            self._stream()))
        else:
            check(self.lib.ldp_unet_forward(self._h, _ptr(x), None, int(k), _ptr(cond_t), _ptr(eps), B,
                                            self._stream()))
        self.call_seq += 1              # (a single evaluation can fault like a loop: column split, fp16-plane range)
        return eps

    # LDP_UNET_STAGE_* of include/ldp_hip.h, by value
    UNET_STAGE_KINDS = ("input", "film_g", "film_t", "res1", "res2", "down", "up", "fin_block", "head")

    def unet_trace(self, x: torch.Tensor, k, cond: Optional[torch.Tensor]):
        """Test hook (ldp_unet_trace): unet_forward through the same code, what every launch wrote tapped.  -> (eps, rows): rows[i] is a
        dict with the stage's `kind`, `block` and `level`, `xa` / `xb` / `res` (the stages it read, -1: none; `res_is_proj`: the residual
        is that stage's projection `t_res`), the `plan` handed to tconv_launch (mode, to, nwn, ks, cpi, res, mb, kws, split), `cs`, `kw`,
        `by_sample`, `tile`, `film_off`, `ca` / `cb`, `channels`, and `t`: the stored tensor on the device, (B, positions, channel
        stride) -- padding included -- with `t_res` the residual projection a first half wrote next to it (else None)."""
        x = _f32(x, self.device)
        B = x.shape[0]
        cond_t = None if cond is None else _f32(cond, self.device)
        _want("x", x, (B, self.T, self.D))
        _want("cond", cond_t, (B, self.G))
        eps = torch.empty_like(x)
        kd, ks = None, 0
        if torch.is_tensor(k) or isinstance(k, np.ndarray):
            kd = torch.as_tensor(k).to(device=self.device, dtype=torch.int32).reshape(-1)
            kd = (kd.expand(B) if kd.numel() == 1 else kd).contiguous()
            _want("k", kd, (B,))
        else:
            ks = int(k)
        ns, nf = C.c_int32(), C.c_int64()
        args = (self._h, _ptr(x), _ptr(kd) if kd is not None else None, ks, _ptr(cond_t), _ptr(eps), B)
        check(self.lib.ldp_unet_trace(*args, None, 0, None, 0, C.byref(ns), C.byref(nf), self._stream()))
        taps = torch.empty(nf.value, device=self.device, dtype=torch.float32)
        cols = 32                                                                   # LDP_UNET_TRACE_COLS
        table = np.full((ns.value, cols), -7, np.int64)
        check(self.lib.ldp_unet_trace(*args, _ptr(taps), nf.value, table.ctypes.data_as(C.c_void_p), ns.value, C.byref(ns), C.byref(nf),
                                      self._stream()))
        self.call_seq += 2
        assert ns.value == len(table) and nf.value == taps.numel()
        rows = []
        for r in table:
            r = [int(v) for v in r]
            off, off_res, n, pos, ld, ch, kind = r[:7]
            numel = n * pos * ld
            rows.append(dict(kind=self.UNET_STAGE_KINDS[kind], block=r[7], level=r[8], xa=r[9], xb=r[10], res=r[11], res_is_proj=r[12] == 1,
                             plan=tuple(r[13:22]), cs=r[22], kw=r[23], by_sample=r[24], tile=r[25], film_off=r[26], ca=r[27], cb=r[28],
                             channels=ch, t=taps[off:off + numel].view(n, pos, ld),
                             t_res=taps[off_res:off_res + numel].view(n, pos, ld) if off_res >= 0 else None))
        return eps, rows

    # -- DPM-Solver++(2M) sampler (csrc/solver.hip) ---------------------------------------------------
    def set_solver_timesteps(self, ts) -> np.ndarray:
        """Registers `ts` (strictly decreasing integers ending in 0, first executed step first) as the timestep table sampler "dpmpp"
        uses whenever it is called with n_steps = len(ts).  The same table again does nothing; another one replaces it (and drops the
        captured graphs)."""
        a = np.ascontiguousarray(np.asarray(ts.cpu() if torch.is_tensor(ts) else ts, dtype=np.int64).reshape(-1).astype(np.int32))
        check(self.lib.ldp_solver_timesteps(self._h, a.ctypes.data_as(C.c_void_p), int(a.size)))
        self.solver_tables[int(a.size)] = a.astype(np.int64)
        return self.solver_tables[int(a.size)]

    def _sampler(self, sampler: str, n_steps: int) -> int:
        """The sampler id of the C ABI.  "dpmpp" runs over a registered timestep table: when this engine holds none for n_steps, the
        log-SNR grid of schedule.solver_timesteps is registered first -- here, so every caller that passes `sampler` through gets it."""
        sid = _SAMPLERS[sampler]
        if sid == SAMPLER_DPMPP and int(n_steps) not in self.solver_tables:
            self.set_solver_timesteps(solver_timesteps(self.planner_train_steps, int(n_steps), "logsnr"))
        return sid

    def plan_solver_step(self, x: torch.Tensor, eps: torch.Tensor, step: int, n_steps: int, x0_prev: Optional[torch.Tensor] = None, *,
                         inplace: bool = False):
        """One solver update (one launch) with row `step` of the table registered for n_steps: x, eps (B, T, D), x0_prev (B, T, D) or None
        (first order) -> (x_next, x0), x0 the clipped data prediction the next step takes as x0_prev.  inplace: x and x0_prev (float32
        device tensors) are overwritten and returned."""
        if inplace:
            xt, hp = x, x0_prev
            for name, t in (("x", xt), ("x0_prev", hp)):
                if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                    raise ValueError(f"inplace: {name} must be a contiguous float32 device tensor")
        else:
            xt = _f32(x, self.device)
            hp = None if x0_prev is None else _f32(x0_prev, self.device)
        B = int(xt.shape[0])
        ep = _f32(eps, self.device)
        _want("x", xt, (B, self.T, self.D))
        _want("eps", ep, (B, self.T, self.D))
        _want("x0_prev", hp, (B, self.T, self.D))
        x_out = xt if inplace else torch.empty_like(xt)
        x0_out = hp if inplace else torch.empty_like(xt)
        check(self.lib.ldp_plan_solver_step(self._h, _ptr(xt), _ptr(ep), _ptr(hp), int(n_steps), int(step), _ptr(x_out), _ptr(x0_out), B,
                                            self._stream()))
        return x_out, x0_out

    def _plan_io(self, cond, B, x_init, step_noise, n_steps, step_end=None):
        """What every plan_sample* method marshals: cond (B, G), x_init (B, T, D) and step_noise (n_steps, B, T, D) as float32 device
        tensors (None stays None) with their shapes checked, B inferred from cond or x_init, the n_steps / step_end defaults and the
        (B, T, D) output -> (cond, x_init, step_noise, B, n_steps, step_end, out)."""
        cond_t = _opt_f32(cond, self.device)
        if B is None:
            B = cond_t.shape[0] if cond_t is not None else x_init.shape[0]
        n_steps = self.planner_train_steps if n_steps is None else int(n_steps)
        step_end = n_steps if step_end is None else int(step_end)
        xi, nz = _opt_f32(x_init, self.device), _opt_f32(step_noise, self.device)
        _want("cond", cond_t, (B, self.G))
        _want("x_init", xi, (B, self.T, self.D))
        _want("step_noise", nz, (n_steps, B, self.T, self.D))
        return cond_t, xi, nz, B, n_steps, step_end, torch.empty((B, self.T, self.D), device=self.device, dtype=torch.float32)

    def _agent_io(self, obs_emb, x_init, x_noise, a_init, a_noise, planner_steps, idm_steps, action_bounds, action_mode, use_graph,
                  parts=None):
        """What every agent_* sampling method marshals: obs_emb (B, H, D), the four optional noise tensors, the step-count defaults, the
        action bounds (length 1 or A) and the x / plan / action outputs.  parts(B), when given, runs right behind the obs_emb check (a
        method's own parts: their errors come before the noise tensors').  -> a namespace: B, H, ps, is_, parts, ob, noise (the four
        pointers x_init, x_noise, a_init, a_noise), out = (x, plan, act) and tail, the arguments every C call of the family ends with."""
        ob = _f32(obs_emb, self.device)
        B, H = ob.shape[0], ob.shape[1]
        _want("obs_emb", ob, (B, H, self.D))
        m = SimpleNamespace(ob=ob, B=B, H=H)
        m.parts = None if parts is None else parts(B)
        m.ps = self.planner_train_steps if planner_steps is None else int(planner_steps)
        m.is_ = self.idm_train_steps if idm_steps is None else int(idm_steps)
        R = B * self.ah
        xi, xn, ai, an = (_opt_f32(t, self.device) for t in (x_init, x_noise, a_init, a_noise))
        _want("x_init", xi, (B, self.T, self.D))
        _want("x_noise", xn, (m.ps, B, self.T, self.D))
        _want("a_init", ai, (R, self.A))
        _want("a_noise", an, (m.is_, R, self.A))
        lo, hi, adim = self._action_bounds(action_bounds, self.A)
        m.keep = (xi, xn, ai, an, lo, hi)
        m.noise = [_ptr(xi), _ptr(xn), _ptr(ai), _ptr(an)]
        m.out = (torch.empty((B, self.T, self.D), device=self.device, dtype=torch.float32),
                 torch.empty((B, self.ah + 1, self.D), device=self.device, dtype=torch.float32),
                 torch.empty((B, self.ah, self.A), device=self.device, dtype=torch.float32))
        m.tail = [m.ps, m.is_, *(_ptr(t) for t in m.out), _ptr(lo), _ptr(hi), adim, int(action_mode), B, 1 if use_graph else 0, self._stream()]
        return m

    def _action_bounds(self, action_bounds, n: int):
        """(lo, hi) of length 1 or n, or None -> (lo, hi, length) as the C ABI takes them (None, None, 0: actions stay normalised)."""
        if action_bounds is None:
            return None, None, 0
        lo, hi = self._bounds(*action_bounds)
        adim = lo.numel()
        if adim not in (1, n) or hi.numel() != adim:
            raise ValueError(f"action bounds must have length 1 or {n}")
        return lo, hi, adim

    def plan_sample(self, cond: Optional[torch.Tensor], B: Optional[int] = None,
                    x_init: Optional[torch.Tensor] = None, step_noise: Optional[torch.Tensor] = None,
                    seed: int = 0, row_offset: int = 0, sampler: str = "ddpm",
                    n_steps: Optional[int] = None, use_graph: bool = True) -> torch.Tensor:
        cond_t, xi, nz, B, n_steps, _, out = self._plan_io(cond, B, x_init, step_noise, n_steps)
        check(self.lib.ldp_plan_sample(self._h, _ptr(cond_t), _ptr(xi), _ptr(nz), _u64(seed), C.c_int64(row_offset),
                                       self._sampler(sampler, n_steps), n_steps, _ptr(out), B, 1 if use_graph else 0, self._stream()))
        self.call_seq += 1
        return out

    # -- warm-started replanning (csrc/replan.hip) ---------------------------------------------------
    def plan_sample_range(self, cond: Optional[torch.Tensor], step_begin: int, step_end: int, B: Optional[int] = None,
                          x_init: Optional[torch.Tensor] = None, step_noise: Optional[torch.Tensor] = None, seed: int = 0,
                          row_offset: int = 0, sampler: str = "ddpm", n_steps: Optional[int] = None, use_graph: bool = True) -> torch.Tensor:
        """plan_sample restricted to the executed steps [step_begin, step_end) of n_steps; step_noise stays (n_steps, B, T, D)."""
        cond_t, xi, nz, B, n_steps, _, out = self._plan_io(cond, B, x_init, step_noise, n_steps)
        check(self.lib.ldp_plan_sample_range(self._h, _ptr(cond_t), _ptr(xi), _ptr(nz), _u64(seed), C.c_int64(row_offset),
                                             self._sampler(sampler, n_steps), n_steps, int(step_begin), int(step_end), _ptr(out), B,
                                             1 if use_graph else 0, self._stream()))
        self.call_seq += 1
        return out

    def _slots(self, slot, B: int):
        """A slot table for the C ABI: None, a device int32 tensor (passed through: the library does not check device-side values) or
        host integers (copied by the call, which checks them) -> (pointer, whatever must stay alive until the call returns)."""
        if slot is None:
            return None, None
        if torch.is_tensor(slot) and slot.is_cuda:
            t = slot.to(device=self.device, dtype=torch.int32).contiguous()
            _want("slot", t, (B,))
            return C.c_void_p(t.data_ptr()), t
        a = np.ascontiguousarray(np.asarray(slot.cpu() if torch.is_tensor(slot) else slot, dtype=np.int32))
        if a.shape != (B,):
            raise ValueError(f"slot must have shape {(B,)}, got {a.shape}")
        return a.ctypes.data_as(C.c_void_p), a

    def _store(self, x_store: torch.Tensor) -> torch.Tensor:
        if not (torch.is_tensor(x_store) and x_store.is_cuda and x_store.dtype == torch.float32 and x_store.is_contiguous()):
            raise ValueError("x_store must be a contiguous float32 device tensor (n_slots, T, D)")
        _want("x_store", x_store, (x_store.shape[0], self.T, self.D))
        return x_store

    def plan_warm_init(self, x_prev: torch.Tensor, step_begin: int, *, slot=None, shift: Optional[int] = None, B: Optional[int] = None,
                       seed: int = 0, row_offset: int = 0, sampler: str = "ddim", n_steps: Optional[int] = None) -> torch.Tensor:
        """The warm initial state of a loop that resumes at executed step step_begin (one launch): rows slot[b] (or b) of x_prev
        (n_slots, T, D), shifted by `shift` positions (default action_horizon) with the edge held, noised to that step's level with the
        Philox draw of plan_sample's x_T for (seed, row_offset) -> (B, T, D)."""
        xp = self._store(_f32(x_prev, self.device))
        n_slots = int(xp.shape[0])
        B = (n_slots if slot is None else len(slot)) if B is None else int(B)
        sp, keep = self._slots(slot, B)
        n_steps = self.planner_train_steps if n_steps is None else int(n_steps)
        out = torch.empty((B, self.T, self.D), device=self.device, dtype=torch.float32)
        check(self.lib.ldp_plan_warm_init(self._h, _ptr(xp), sp, n_slots, self.ah if shift is None else int(shift),
                                          _u64(seed), C.c_int64(row_offset), _SAMPLERS[sampler], n_steps,
                                          int(step_begin), _ptr(out), B, self._stream()))
        del keep
        return out

    def agent_resample(self, obs_emb: torch.Tensor, obs_horizon: int, x_store: torch.Tensor, step_begin: int, *, slot=None,
                       shift: Optional[int] = None, x_noise=None, a_init=None, a_noise=None, seed: int = 0, row_offset: int = 0,
                       sampler: str = "ddim", planner_steps: Optional[int] = None, idm_steps: Optional[int] = None,
                       action_bounds=None, action_mode: int = 0, use_graph: bool = True):
        """agent_sample resumed from the previous plan: the planner state is the warm initial state of rows slot[b] (or b) of x_store
        (n_slots, T, D), the planner loop runs the steps [step_begin, planner_steps), and the new full state is written back IN PLACE to
        the same rows of x_store -> (x, plan, action) as agent_sample.  Slots must be distinct within a call."""
        m = self._agent_io(obs_emb, None, x_noise, a_init, a_noise, planner_steps, idm_steps, action_bounds, action_mode, use_graph,
                           parts=lambda B: (self._store(x_store), *self._slots(slot, B)))
        xs, sp, keep = m.parts
        check(self.lib.ldp_agent_resample(self._h, _ptr(m.ob), m.H, int(obs_horizon), _ptr(xs), sp, int(xs.shape[0]),
                                          self.ah if shift is None else int(shift), int(step_begin), *m.noise[1:], _u64(seed),
                                          C.c_int64(row_offset), _SAMPLERS[sampler], *m.tail))
        del keep
        self.call_seq += 1
        return m.out

    # -- constrained planning (csrc/constrain.hip) ----------------------------------------------------
    def _constraint(self, target, mask, mode, B: int):
        """target (B, T, D) float32, mask (B, T, D) uint8 (bool is taken as 0 / 1) and the LDP_CONSTRAIN_* mode for the C ABI.  `mode` is
        'clamp' / 'repaint' (anything else is a ValueError here) or the integer itself (the library checks it)."""
        if target is None or mask is None:
            raise ValueError("target and mask are both required")
        if isinstance(mode, str):
            if mode not in _CONSTRAIN_MODES:
                raise ValueError(f"mode must be one of {sorted(_CONSTRAIN_MODES)}, got {mode!r}")
            mode = _CONSTRAIN_MODES[mode]
        tg = _f32(target, self.device)
        mk = mask if torch.is_tensor(mask) else torch.as_tensor(np.asarray(mask))
        if mk.dtype not in (torch.uint8, torch.bool):
            raise ValueError(f"mask must be uint8 or bool, got {mk.dtype}")
        mk = mk.to(device=self.device, dtype=torch.uint8).contiguous()
        _want("target", tg, (B, self.T, self.D))
        _want("mask", mk, (B, self.T, self.D))
        return tg, mk, int(mode)

    def plan_constrain(self, x: torch.Tensor, target, mask, level: int, *, mode="repaint", seed: int = 0, row_offset: int = 0,
                       sampler: str = "ddim", n_steps: Optional[int] = None) -> torch.Tensor:
        """The constraint operation C_level alone (one launch): x (B, T, D) with the entries under `mask` replaced by `target` at the
        noise level of `level` in 0 .. n_steps -> a new (B, T, D) tensor; every other element keeps its bits."""
        xt = _f32(x, self.device)
        B = int(xt.shape[0])
        _want("x", xt, (B, self.T, self.D))
        tg, mk, md = self._constraint(target, mask, mode, B)
        n_steps = self.planner_train_steps if n_steps is None else int(n_steps)
        out = torch.empty_like(xt)
        check(self.lib.ldp_plan_constrain(self._h, _ptr(xt), _ptr(tg), _ptr(mk), md, _SAMPLERS[sampler], n_steps, int(level),
                                          _u64(seed), C.c_int64(row_offset), _ptr(out), B, self._stream()))
        return out

    def plan_sample_constrained(self, cond: Optional[torch.Tensor], target, mask, *, mode="repaint", step_begin: int = 0,
                                step_end: Optional[int] = None, B: Optional[int] = None, x_init: Optional[torch.Tensor] = None,
                                step_noise: Optional[torch.Tensor] = None, seed: int = 0, row_offset: int = 0, sampler: str = "ddpm",
                                n_steps: Optional[int] = None, use_graph: bool = True) -> torch.Tensor:
        """plan_sample_range with the constraint applied in the loop: C_begin in front of the first executed step and C_{i+1} behind
        step i, inside the captured graph (default range: the whole loop).  An empty range returns C_begin of the initial state."""
        cond_t, xi, nz, B, n_steps, step_end, out = self._plan_io(cond, B, x_init, step_noise, n_steps, step_end)
        tg, mk, md = self._constraint(target, mask, mode, B)
        check(self.lib.ldp_plan_sample_constrained(self._h, _ptr(cond_t), _ptr(xi), _ptr(nz), _ptr(tg), _ptr(mk), md,
                                                   _u64(seed), C.c_int64(row_offset), _SAMPLERS[sampler], n_steps,
                                                   int(step_begin), step_end, _ptr(out), B, 1 if use_graph else 0, self._stream()))
        self.call_seq += 1
        return out

    def agent_sample_constrained(self, obs_emb: torch.Tensor, obs_horizon: int, target, mask, *, mode="repaint", x_init=None,
                                 x_noise=None, a_init=None, a_noise=None, seed: int = 0, row_offset: int = 0, sampler: str = "ddpm",
                                 planner_steps: Optional[int] = None, idm_steps: Optional[int] = None, action_bounds=None,
                                 action_mode: int = 0, use_graph: bool = True, x_store=None):
        """agent_sample whose planner loop is the constrained one -> (x, plan, action) as agent_sample.  x_store (a warm start's table,
        agent_resample) is refused: a constraint together with a warm start is not built."""
        if x_store is not None:
            raise ValueError("a constraint (target / mask) together with a warm start (x_store) is not built")
        m = self._agent_io(obs_emb, x_init, x_noise, a_init, a_noise, planner_steps, idm_steps, action_bounds, action_mode, use_graph,
                           parts=lambda B: self._constraint(target, mask, mode, B))
        tg, mk, md = m.parts
        check(self.lib.ldp_agent_sample_constrained(self._h, _ptr(m.ob), m.H, int(obs_horizon), *m.noise, _ptr(tg), _ptr(mk), md, _u64(seed),
                                                    C.c_int64(row_offset), _SAMPLERS[sampler], *m.tail))
        self.call_seq += 1
        return m.out

    # -- guided planning (csrc/guide.hip) --------------------------------------------------------------
    def _guide(self, guide, B: int, ld: Optional[int] = None):
        """A guide (guide.Guide, or anything with its fields) for the C ABI: target, weight (B, T, D) and anchor (B, D) or None as device
        tensors -- (B, T, ld) / (B, ld) when a padded stride is asked for -- and lam, beta, lo, hi (D,) as host float32 arrays."""
        if getattr(guide, "anchor", None) is True:
            raise ValueError("anchor=True is resolved by LDPAgent.sample_guided (the batch's last observation embedding): give the "
                             "embeddings (B, D) here")
        tg, wg = _f32(guide.target, self.device), _f32(guide.weight, self.device)
        an = None if guide.anchor is None else _f32(guide.anchor, self.device)
        _want("target", tg, (B, self.T, self.D))
        _want("weight", wg, (B, self.T, self.D))
        _want("anchor", an, (B, self.D))
        if ld is not None and ld != self.D:
            pad = lambda t: torch.nn.functional.pad(t, (0, ld - self.D)).contiguous()
            tg, wg, an = pad(tg), pad(wg), None if an is None else pad(an)
        cols = []
        for name in ("lam", "beta", "lo", "hi"):
            a = np.ascontiguousarray(np.asarray(getattr(guide, name), dtype=np.float32))
            if a.shape != (self.D,):
                raise ValueError(f"{name} must have shape {(self.D,)}, got {a.shape}")
            cols.append(a)
        return tg, wg, an, cols

    @staticmethod
    def _host_ptr(a: np.ndarray):
        return a.ctypes.data_as(C.c_void_p)

    def plan_guide_step(self, x: torch.Tensor, eps: torch.Tensor, guide, rho, step: int, *, noise=None, seed: int = 0, row_offset: int = 0,
                        sampler: str = "ddim", n_steps: Optional[int] = None, ldg: Optional[int] = None, inplace: bool = False) -> torch.Tensor:
        """One guided step (one launch): x (B, T, ldx) with ldx >= D (a padded state: the columns beyond D keep their bits), eps (B, T, D),
        rho (n_steps,) step sizes of which entry `step` is used, noise (B, T, D) or None (the Philox draw of (seed, row_offset)) -> the
        new x.  ldg: the row stride the guide's target / weight / anchor are handed over with (default D).  inplace: x is overwritten."""
        xt = x if inplace else _f32(x, self.device).clone()
        if not (torch.is_tensor(xt) and xt.is_cuda and xt.dtype == torch.float32 and xt.is_contiguous()):
            raise ValueError("inplace: x must be a contiguous float32 device tensor")
        B, ldx = int(xt.shape[0]), int(xt.shape[-1])
        if xt.dim() != 3 or xt.shape[1] != self.T or ldx < self.D:
            raise ValueError(f"x must have shape {(B, self.T, self.D)} (or a wider last axis), got {tuple(xt.shape)}")
        ep = _f32(eps, self.device)
        nz = None if noise is None else _f32(noise, self.device)
        _want("eps", ep, (B, self.T, self.D))
        _want("noise", nz, (B, self.T, self.D))
        n_steps = self.planner_train_steps if n_steps is None else int(n_steps)
        ldg = self.D if ldg is None else int(ldg)
        tg, wg, an, cols = self._guide(guide, B, ldg)
        dev = [torch.as_tensor(a).to(self.device) for a in cols]
        rh = _f32(np.asarray(rho, dtype=np.float32).reshape(-1), self.device)
        _want("rho", rh, (n_steps,))
        check(self.lib.ldp_plan_guide_step(self._h, _ptr(xt), _ptr(ep), _ptr(nz), _ptr(tg), _ptr(wg), _ptr(an), _ptr(dev[0]), _ptr(dev[1]),
                                           _ptr(dev[2]), _ptr(dev[3]), _ptr(rh), _SAMPLERS[sampler], n_steps, int(step),
                                           _u64(seed), C.c_int64(row_offset), _ptr(xt), ldx, ldg, B, self._stream()))
        return xt

    def plan_guide_cost(self, x: torch.Tensor, guide, n_per: int = 1) -> torch.Tensor:
        """J of every row of x (rows, T, D) under row r // n_per of the guide (rows = B * n_per) -> (rows,) device costs, one launch."""
        xt = _f32(x, self.device)
        rows, n_per = int(xt.shape[0]), int(n_per)
        if n_per < 1 or rows < 1 or rows % n_per:
            raise ValueError(f"x must hold a positive multiple of n_per = {n_per} rows, got {rows}")
        _want("x", xt, (rows, self.T, self.D))
        tg, wg, an, cols = self._guide(guide, rows // n_per)
        dev = [torch.as_tensor(a).to(self.device) for a in cols]
        out = torch.empty((rows,), device=self.device, dtype=torch.float32)
        check(self.lib.ldp_plan_guide_cost(self._h, _ptr(xt), _ptr(tg), _ptr(wg), _ptr(an), _ptr(dev[0]), _ptr(dev[1]), _ptr(dev[2]),
                                           _ptr(dev[3]), C.c_int64(rows), n_per, _ptr(out), self._stream()))
        return out

    def plan_sample_guided(self, cond: Optional[torch.Tensor], guide, rho, *, step_begin: int = 0, step_end: Optional[int] = None,
                           B: Optional[int] = None, x_init: Optional[torch.Tensor] = None, step_noise: Optional[torch.Tensor] = None,
                           seed: int = 0, row_offset: int = 0, sampler: str = "ddim", n_steps: Optional[int] = None,
                           use_graph: bool = True) -> torch.Tensor:
        """plan_sample_range with the guided loop: per executed step the U-Net's eps, then one guided step with the step size rho[i]
        (default range: the whole loop).  rho: n_steps step sizes (the library checks the count)."""
        cond_t, xi, nz, B, n_steps, step_end, out = self._plan_io(cond, B, x_init, step_noise, n_steps, step_end)
        tg, wg, an, cols = self._guide(guide, B)
        rh = np.ascontiguousarray(np.asarray(rho, dtype=np.float32).reshape(-1))
        check(self.lib.ldp_plan_sample_guided(self._h, _ptr(cond_t), _ptr(xi), _ptr(nz), _ptr(tg), _ptr(wg), _ptr(an),
                                              *(self._host_ptr(a) for a in cols), self._host_ptr(rh), int(rh.size),
                                              _u64(seed), C.c_int64(row_offset), _SAMPLERS[sampler], n_steps,
                                              int(step_begin), step_end, _ptr(out), B, 1 if use_graph else 0, self._stream()))
        self.call_seq += 1
        return out

    def agent_sample_guided(self, obs_emb: torch.Tensor, obs_horizon: int, guide, rho, *, x_init=None, x_noise=None, a_init=None,
                            a_noise=None, seed: int = 0, row_offset: int = 0, sampler: str = "ddim", planner_steps: Optional[int] = None,
                            idm_steps: Optional[int] = None, action_bounds=None, action_mode: int = 0, use_graph: bool = True):
        """agent_sample whose planner loop is the guided one -> (x, plan, action) as agent_sample."""
        m = self._agent_io(obs_emb, x_init, x_noise, a_init, a_noise, planner_steps, idm_steps, action_bounds, action_mode, use_graph,
                           parts=lambda B: self._guide(guide, B))
        tg, wg, an, cols = m.parts
        rh = np.ascontiguousarray(np.asarray(rho, dtype=np.float32).reshape(-1))
        check(self.lib.ldp_agent_sample_guided(self._h, _ptr(m.ob), m.H, int(obs_horizon), *m.noise, _ptr(tg), _ptr(wg), _ptr(an),
                                               *(self._host_ptr(a) for a in cols), self._host_ptr(rh), int(rh.size), _u64(seed),
                                               C.c_int64(row_offset), _SAMPLERS[sampler], *m.tail))
        self.call_seq += 1
        return m.out

    # -- composed planning (csrc/compose.hip) ----------------------------------------------------------
    def _compose(self, B: int, n_steps: int, *, guide=None, rho=None, target=None, mask=None, mode="repaint", x_store=None, slot=None,
                 shift: Optional[int] = None, ldg: Optional[int] = None, ldc: Optional[int] = None, device_cols: bool = False):
        """The ldp_plan_compose of a call and whatever must stay alive until it returns.  guide with rho (n_steps step sizes), target with
        mask, x_store (with slot / shift): each part is optional.  device_cols: lam, beta, lo, hi, rho as device tensors (the stand-alone
        step) instead of host arrays (the sampling calls).  ldg / ldc: padded row strides of the guide's / the constraint's arrays."""
        pc, keep = _lib.LdpPlanCompose(), []
        if x_store is not None:
            xs = self._store(x_store)
            sp, k = self._slots(slot, B)
            keep += [xs, k]
            pc.x_store, pc.slot, pc.n_slots = xs.data_ptr(), sp, int(xs.shape[0])
            pc.shift = self.ah if shift is None else int(shift)
        elif slot is not None or shift is not None:
            raise ValueError("slot and shift describe a warm start: give x_store too")
        if (target is None) != (mask is None):
            raise ValueError("target and mask are both required")
        if target is not None:
            tg, mk, md = self._constraint(target, mask, mode, B)
            if ldc is not None and ldc != self.D:
                tg = torch.nn.functional.pad(tg, (0, ldc - self.D)).contiguous()
                mk = torch.nn.functional.pad(mk, (0, ldc - self.D)).contiguous()
            keep += [tg, mk]
            pc.target, pc.mask, pc.mode = tg.data_ptr(), mk.data_ptr(), md
        if (guide is None) != (rho is None):
            raise ValueError("guide and rho go together: give both or neither")
        if guide is not None:
            tg, wg, an, cols = self._guide(guide, B, ldg)
            rh = np.ascontiguousarray(np.asarray(rho, dtype=np.float32).reshape(-1))
            keep += [tg, wg, an]
            pc.g_target, pc.g_wg, pc.g_anchor = tg.data_ptr(), wg.data_ptr(), None if an is None else an.data_ptr()
            if device_cols:
                dev = [torch.as_tensor(a).to(self.device) for a in cols + [rh]]
                ptrs = [t.data_ptr() for t in dev]
                keep += dev
            else:
                ptrs = [a.ctypes.data for a in cols + [rh]]
                keep += cols + [rh]
            pc.lam, pc.beta, pc.lo, pc.hi, pc.rho = ptrs
            pc.n_rho = int(rh.size)
        return pc, keep

    def plan_compose_step(self, x: torch.Tensor, eps: torch.Tensor, step: int, *, guide=None, rho=None, target=None, mask=None,
                          mode="repaint", noise=None, x0_prev=None, second: bool = False, seed: int = 0, row_offset: int = 0,
                          sampler: str = "ddim", n_steps: Optional[int] = None, ldg: Optional[int] = None, ldc: Optional[int] = None,
                          inplace: bool = False):
        """One composed step (one launch): x (B, T, ldx) with ldx >= D (a padded state: the columns beyond D keep their bits), eps
        (B, T, D) -> the new x; under sampler "dpmpp" -> (x, x0) with x0 (B, T, ldx) the guided data prediction the next step takes as
        x0_prev (second: this step is second order, on x0_prev (B, T, ldx)).  guide with rho (n_steps,), target with mask: the optional
        parts.  noise (B, T, D) or None (the Philox draw of (seed, row_offset)).  inplace: x (and x0_prev, when given) are overwritten."""
        xt = x if inplace else _f32(x, self.device).clone()
        if not (torch.is_tensor(xt) and xt.is_cuda and xt.dtype == torch.float32 and xt.is_contiguous()):
            raise ValueError("inplace: x must be a contiguous float32 device tensor")
        B, ldx = int(xt.shape[0]), int(xt.shape[-1])
        if xt.dim() != 3 or xt.shape[1] != self.T or ldx < self.D:
            raise ValueError(f"x must have shape {(B, self.T, self.D)} (or a wider last axis), got {tuple(xt.shape)}")
        ep = _f32(eps, self.device)
        nz = None if noise is None else _f32(noise, self.device)
        _want("eps", ep, (B, self.T, self.D))
        _want("noise", nz, (B, self.T, self.D))
        n_steps = self.planner_train_steps if n_steps is None else int(n_steps)
        sid = self._sampler(sampler, n_steps)
        hp = h_out = None
        if sid == SAMPLER_DPMPP:
            if x0_prev is not None:
                hp = x0_prev if inplace else _f32(x0_prev, self.device).clone()
                if not (torch.is_tensor(hp) and hp.is_cuda and hp.dtype == torch.float32 and hp.is_contiguous()):
                    raise ValueError("inplace: x0_prev must be a contiguous float32 device tensor")
                _want("x0_prev", hp, tuple(xt.shape))
            h_out = hp if hp is not None else torch.zeros_like(xt)
        pc, keep = self._compose(B, n_steps, guide=guide, rho=rho, target=target, mask=mask, mode=mode, ldg=ldg, ldc=ldc, device_cols=True)
        check(self.lib.ldp_plan_compose_step(self._h, _ptr(xt), _ptr(ep), _ptr(nz), _ptr(hp), C.byref(pc), sid, n_steps, int(step),
                                             1 if second else 0, _u64(seed), C.c_int64(row_offset), _ptr(xt), _ptr(h_out),
                                             ldx, self.D if ldg is None else int(ldg), self.D if ldc is None else int(ldc), B, self._stream()))
        del keep
        return (xt, h_out) if sid == SAMPLER_DPMPP else xt

    def plan_sample_composed(self, cond: Optional[torch.Tensor], *, guide=None, rho=None, target=None, mask=None, mode="repaint",
                             x_store=None, slot=None, shift: Optional[int] = None, step_begin: int = 0, step_end: Optional[int] = None,
                             B: Optional[int] = None, x_init: Optional[torch.Tensor] = None, step_noise: Optional[torch.Tensor] = None,
                             seed: int = 0, row_offset: int = 0, sampler: str = "ddim", n_steps: Optional[int] = None,
                             use_graph: bool = True) -> torch.Tensor:
        """plan_sample_range with any of a guide (with rho), a constraint (target, mask, mode) and a warm start (x_store, slot, shift: the
        initial state is the warm one at the level of step_begin; x_store is not written), under any sampler.  With a guide,
        or under "dpmpp", the loop is the stepped one (one launch of the step kernel behind every U-Net evaluation does guide, update
        and constraint); otherwise the U-Net's last launch does the scheduler step and a constraint is a launch of its own."""
        cond_t, xi, nz, B, n_steps, step_end, out = self._plan_io(cond, B, x_init, step_noise, n_steps, step_end)
        pc, keep = self._compose(B, n_steps, guide=guide, rho=rho, target=target, mask=mask, mode=mode, x_store=x_store, slot=slot, shift=shift)
        check(self.lib.ldp_plan_sample_composed(self._h, _ptr(cond_t), _ptr(xi), _ptr(nz), C.byref(pc), _u64(seed),
                                                C.c_int64(row_offset), self._sampler(sampler, n_steps), n_steps, int(step_begin), step_end,
                                                _ptr(out), B, 1 if use_graph else 0, self._stream()))
        del keep
        self.call_seq += 1
        return out

    def agent_sample_composed(self, obs_emb: torch.Tensor, obs_horizon: int, *, guide=None, rho=None, target=None, mask=None,
                              mode="repaint", x_store=None, slot=None, shift: Optional[int] = None, step_begin: int = 0, x_init=None,
                              x_noise=None, a_init=None, a_noise=None, seed: int = 0, row_offset: int = 0, sampler: str = "ddim",
                              planner_steps: Optional[int] = None, idm_steps: Optional[int] = None, action_bounds=None,
                              action_mode: int = 0, use_graph: bool = True):
        """agent_sample (no x_store) / agent_resample (x_store: the planner loop is [step_begin, planner_steps) from the warm state, and
        the new state is written back IN PLACE to the same rows of x_store) with any of a guide and a constraint, under any sampler
        -> (x, plan, action)."""
        m = self._agent_io(obs_emb, x_init, x_noise, a_init, a_noise, planner_steps, idm_steps, action_bounds, action_mode, use_graph)
        pc, keep = self._compose(m.B, m.ps, guide=guide, rho=rho, target=target, mask=mask, mode=mode, x_store=x_store, slot=slot, shift=shift)
        check(self.lib.ldp_agent_sample_composed(self._h, _ptr(m.ob), m.H, int(obs_horizon), *m.noise, C.byref(pc), int(step_begin), _u64(seed),
                                                 C.c_int64(row_offset), self._sampler(sampler, m.ps), *m.tail))
        del keep
        self.call_seq += 1
        return m.out

    # -- best-of-N planning (csrc/select.hip): candidate-major rows r = c * B + b ---------------------
    def plan_candidates(self, obs_emb: torch.Tensor, obs_horizon: int, n_candidates: int, *, c0: int = 0, n_loc: Optional[int] = None,
                        x_init=None, step_noise=None, seed: int = 0, sampler: str = "ddpm", n_steps: Optional[int] = None,
                        use_graph: bool = True) -> torch.Tensor:
        """Candidates [c0, c0 + n_loc) of n_candidates plans per observation: obs_emb (B, frames, D) -> x (n_loc * B, T, D), row
        (c - c0) * B + b, each keyed by its global row c * B + b.  x_init (n_loc * B, T, D) / step_noise (n_steps, n_loc * B, T, D):
        explicit noise of these rows."""
        ob = _f32(obs_emb, self.device)
        B, H = ob.shape[0], ob.shape[1]
        _want("obs_emb", ob, (B, H, self.D))
        n_loc = int(n_candidates) - int(c0) if n_loc is None else int(n_loc)
        check_candidate_range(B, int(n_candidates), self.T * self.D, int(c0), n_loc)
        n_steps = self.planner_train_steps if n_steps is None else int(n_steps)
        rows = n_loc * B
        xi = None if x_init is None else _f32(x_init, self.device)
        nz = None if step_noise is None else _f32(step_noise, self.device)
        _want("x_init", xi, (rows, self.T, self.D))
        _want("step_noise", nz, (n_steps, rows, self.T, self.D))
        out = torch.empty((rows, self.T, self.D), device=self.device, dtype=torch.float32)
        check(self.lib.ldp_plan_candidates(self._h, _ptr(ob), H, int(obs_horizon), B, int(c0), n_loc, _ptr(xi), _ptr(nz),
                                           _u64(seed), self._sampler(sampler, n_steps), n_steps, _ptr(out),
                                           1 if use_graph else 0, self._stream()))
        self.call_seq += 1
        return out

    def plan_cost_density(self, x_all: torch.Tensor, B: int, bandwidth: float = 0.5, *, c0: int = 0,
                          n_loc: Optional[int] = None) -> torch.Tensor:
        """Density cost of candidates [c0, c0 + n_loc) against ALL candidates: x_all (N * B, ...) candidate-major -> (n_loc, B)."""
        x = _f32(x_all, self.device)
        N, K = _candidate_dims(x, B)
        n_loc = N - int(c0) if n_loc is None else int(n_loc)
        check_candidate_range(int(B), N, K, int(c0), n_loc, bandwidth=bandwidth)
        out = torch.empty((n_loc, int(B)), device=self.device, dtype=torch.float32)
        check(self.lib.ldp_plan_cost_density(_ptr(x), int(B), N, K, int(c0), n_loc, C.c_float(float(bandwidth)), _ptr(out), self._stream()))
        return out

    def plan_cost_goal(self, x: torch.Tensor, B: int, goal: torch.Tensor, weight=None, t_goal: Optional[int] = None) -> torch.Tensor:
        """Goal cost of the n candidates given: x (n * B, T, D) candidate-major, goal (B, D), weight (D,) >= 0 (default ones),
        t_goal (default action_horizon - 1) -> (n, B)."""
        x = _f32(x, self.device)
        if x.dim() != 3:
            raise ValueError(f"x must have shape (n * B, T, D), got {tuple(x.shape)}")
        n, _ = _candidate_dims(x, B)
        T, D = int(x.shape[1]), int(x.shape[2])
        g = _f32(goal, self.device)
        _want("goal", g, (int(B), D))
        w = torch.ones(D, device=self.device, dtype=torch.float32) if weight is None else _f32(weight, self.device).reshape(-1)
        _want("goal_weight", w, (D,))
        if weight is not None and not bool((np.asarray(torch.as_tensor(weight).detach().cpu()) >= 0).all()):
            raise ValueError("goal_weight must be non-negative")
        t_goal = self.ah - 1 if t_goal is None else int(t_goal)
        if not 0 <= t_goal < T:
            raise ValueError(f"t_goal must lie in 0..{T - 1}, got {t_goal}")
        out = torch.empty((n, int(B)), device=self.device, dtype=torch.float32)
        check(self.lib.ldp_plan_cost_goal(_ptr(x), int(B), n, T, D, t_goal, _ptr(g), _ptr(w), _ptr(out), self._stream()))
        return out

    def plan_select(self, cost_all: torch.Tensor, x_all: torch.Tensor, B: int):
        """argmin over the candidates of every observation (ties to the lowest index, NaN as +inf) and the winner's rows:
        cost_all (N, B), x_all (N * B, ...) -> (best_index (B,) int32, best_cost (B,), x_best (B, ...))."""
        x = _f32(x_all, self.device)
        N, K = _candidate_dims(x, B)
        cost = _f32(cost_all, self.device)
        if cost.numel() != N * int(B):
            raise ValueError(f"cost_all must hold N * B = {N * int(B)} costs, got shape {tuple(cost.shape)}")
        idx = torch.empty((int(B),), device=self.device, dtype=torch.int32)
        best = torch.empty((int(B),), device=self.device, dtype=torch.float32)
        xb = torch.empty((int(B),) + tuple(x.shape[1:]), device=self.device, dtype=torch.float32)
        check(self.lib.ldp_plan_select(_ptr(cost), _ptr(x), int(B), N, K, _ptr(idx), _ptr(best), _ptr(xb), self._stream()))
        return idx, best, xb

    # -- IDM ------------------------------------------------------------------------------------
    def idm_forward(self, s: torch.Tensor, a: torch.Tensor, k) -> torch.Tensor:
        s, a = _f32(s, self.device), _f32(a, self.device)
        R = s.shape[0]
        _want("s", s, (R, 2 * self.D))
        _want("a", a, (R, self.A))
        eps = torch.empty_like(a)
        if torch.is_tensor(k) or isinstance(k, np.ndarray):
            kd = torch.as_tensor(k).to(device=self.device, dtype=torch.int32).reshape(-1)
            if kd.numel() == 1:
                kd = kd.expand(R)
            kd = kd.contiguous()
            check(self.lib.ldp_idm_forward(self._h, _ptr(s), _ptr(a), _ptr(kd), 0, _ptr(eps), R, self._stream()))
        else:
            check(self.lib.ldp_idm_forward(self._h, _ptr(s), _ptr(a), None, int(k), _ptr(eps), R, self._stream()))
        self.call_seq += 1
        return eps

    def idm_sample(self, transition: torch.Tensor, a_init: Optional[torch.Tensor] = None,
                   step_noise: Optional[torch.Tensor] = None, seed: int = 0, row_offset: int = 0,
                   sampler: str = "ddpm", n_steps: Optional[int] = None, use_graph: bool = True) -> torch.Tensor:
        tr = _f32(transition, self.device)
        R = tr.shape[0]
        n_steps = self.idm_train_steps if n_steps is None else int(n_steps)
        ai = None if a_init is None else _f32(a_init, self.device)
        nz = None if step_noise is None else _f32(step_noise, self.device)
        _want("transition", tr, (R, 2 * self.D))
        _want("a_init", ai, (R, self.A))
        _want("step_noise", nz, (n_steps, R, self.A))
        out = torch.empty((R, self.A), device=self.device, dtype=torch.float32)
        check(self.lib.ldp_idm_sample(self._h, _ptr(tr), _ptr(ai), _ptr(nz), _u64(seed),
                                      C.c_int64(row_offset), _SAMPLERS[sampler], n_steps, _ptr(out), R,
                                      1 if use_graph else 0, self._stream()))
        self.call_seq += 1
        return out

    # -- planner + IDM as one call / one captured graph ---------------------------------------------
    def agent_sample(self, obs_emb: torch.Tensor, obs_horizon: int, *, x_init=None, x_noise=None, a_init=None,
                     a_noise=None, seed: int = 0, row_offset: int = 0, sampler: str = "ddpm",
                     planner_steps: Optional[int] = None, idm_steps: Optional[int] = None,
                     action_bounds=None, action_mode: int = 0, use_graph: bool = True):
        """sample_viz_step without the decode (agent/ldp_agent.py:452-505): -> (x, plan, action) with
        x (B,T,D), plan (B,ah+1,D), action (B,ah,A).  action_bounds = (lo, hi) device tensors of length
        1 or A (None: actions stay normalised); action_mode 0 = unnormalize + clip, 2 = clip."""
        m = self._agent_io(obs_emb, x_init, x_noise, a_init, a_noise, planner_steps, idm_steps, action_bounds, action_mode, use_graph)
        check(self.lib.ldp_agent_sample(self._h, _ptr(m.ob), m.H, int(obs_horizon), *m.noise, _u64(seed), C.c_int64(row_offset),
                                        self._sampler(sampler, m.ps), *m.tail))
        self.call_seq += 1
        return m.out

    # -- DP policy: condition gather + U-Net loop + action rows as one call / one captured graph ---------------------
    def policy_sample(self, obs_emb: torch.Tensor, obs_horizon: int, img_width: int, *, x_init=None, x_noise=None, seed: int = 0,
                      row_offset: int = 0, sampler: str = "ddpm", n_steps: Optional[int] = None, action_bounds=None,
                      action_mode: int = 0, use_graph: bool = True) -> torch.Tensor:
        """DPVAEAgent.sample_step (agent/dp_repr_agent.py:169-201) on this handle's planner module (the action U-Net: D = A):
        obs_emb (B, frames, E) per-frame [image latent (img_width) | low-dim] -> actions (B, action_horizon, A).  action_bounds /
        action_mode as in agent_sample."""
        ob = _f32(obs_emb, self.device)
        B, H = ob.shape[0], ob.shape[1]
        E = self.G // int(obs_horizon)
        _want("obs_emb", ob, (B, H, E))
        n_steps = self.planner_train_steps if n_steps is None else int(n_steps)
        xi, xn = _opt_f32(x_init, self.device), _opt_f32(x_noise, self.device)
        _want("x_init", xi, (B, self.T, self.D))
        _want("x_noise", xn, (n_steps, B, self.T, self.D))
        lo, hi, adim = self._action_bounds(action_bounds, self.D)
        act = torch.empty((B, self.ah, self.D), device=self.device, dtype=torch.float32)
        check(self.lib.ldp_policy_sample(self._h, _ptr(ob), H, int(obs_horizon), int(img_width), _ptr(xi), _ptr(xn),
                                         _u64(seed), C.c_int64(row_offset), self._sampler(sampler, n_steps), n_steps, _ptr(act),
                                         _ptr(lo), _ptr(hi), adim, int(action_mode), B, 1 if use_graph else 0, self._stream()))
        self.call_seq += 1
        return act

    # -- VAE ------------------------------------------------------------------------------------
    def vae_encode(self, img_nhwc: torch.Tensor) -> torch.Tensor:
        img = _f32(img_nhwc, self.device)
        n, s = img.shape[0], img.shape[1]
        _want("img_nhwc", img, (n, self.image_size, self.image_size, 3))
        out = torch.empty((n, s // 32, s // 32, self.cfg.vae_latent_channels), device=self.device,
                          dtype=torch.float32)
        check(self.lib.ldp_vae_encode(self._h, _ptr(img), _ptr(out), n, self._stream()))
        self.call_seq += 1              # (the fp16-plane range guard can fault this call)
        return out

    def vae_decode(self, z_nhwc: torch.Tensor) -> torch.Tensor:
        z = _f32(z_nhwc, self.device)
        n = z.shape[0]
        s = int(self.cfg.image_size)
        _want("z_nhwc", z, (n, s // 32, s // 32, self.latent_channels))
        out = torch.empty((n, 3, s, s), device=self.device, dtype=torch.float32)
        check(self.lib.ldp_vae_decode(self._h, _ptr(z), _ptr(out), n, self._stream()))
        self.call_seq += 1
        return out

    def vae_moments(self, img_nhwc: torch.Tensor) -> torch.Tensor:
        """The full quant_conv output (N, S/32, S/32, 2 LC): channels [0, LC) the posterior mean (the bits of vae_encode), [LC, 2 LC) the
        unclamped log-variance."""
        img = _f32(img_nhwc, self.device)
        n, s = img.shape[0], img.shape[1]
        _want("img_nhwc", img, (n, self.image_size, self.image_size, 3))
        out = torch.empty((n, s // 32, s // 32, 2 * self.latent_channels), device=self.device, dtype=torch.float32)
        check(self.lib.ldp_vae_moments(self._h, _ptr(img), _ptr(out), n, self._stream()))
        self.call_seq += 1
        return out

    # LDP_VAE_STAGE_* / LDP_VAE_FAM_* / LDP_VAE_STATS_* of include/ldp_hip.h, by value
    VAE_STAGE_KINDS = ("conv_in", "res1", "shortcut", "res2", "down", "attn", "conv_out", "quant", "post_quant", "up", "nchw", "upsampled")
    VAE_FAMILIES = ("none", "tconv_f32", "sconv_bf16x6", "sconv_f16x3", "tconv_f16x3")
    VAE_STATS_ROUTES = ("none", "conv", "conv_in", "gn_part")

    def vae_trace(self, x: torch.Tensor, decode: bool = False):
        """Test hook (ldp_vae_trace): one chunk of the encoder (x = frames (N, S, S, 3) -> moments) or of the decoder (x = z -> image)
        through the code of vae_moments / vae_decode, every stage's output tapped.  -> (out, rows): rows[k] is a dict with the stage's
        `kind`, `inputs` (stage indices, -1 = x), `family`, `tile` (nwn, ks, cpi), `stats` route, `fused_out`, `channels` and `t`, the
        stored tensor on the device: (N, H, W, channel stride) -- padding included -- or (N, C, H, W) for the final transpose."""
        x = _f32(x, self.device)
        n, s, lc = x.shape[0], int(self.image_size), self.latent_channels
        if decode:
            _want("z_nhwc", x, (n, s // 32, s // 32, lc))
            out = torch.empty((n, 3, s, s), device=self.device, dtype=torch.float32)
        else:
            _want("img_nhwc", x, (n, s, s, 3))
            out = torch.empty((n, s // 32, s // 32, 2 * lc), device=self.device, dtype=torch.float32)
        ns, nf = C.c_int32(), C.c_int64()
        check(self.lib.ldp_vae_trace(self._h, int(decode), _ptr(x), _ptr(out), n, None, 0, None, 0, C.byref(ns), C.byref(nf), self._stream()))
        taps = torch.empty(nf.value, device=self.device, dtype=torch.float32)
        cols = 16                                                                   # LDP_VAE_TRACE_COLS
        table = np.full((ns.value, cols), -7, np.int64)
        check(self.lib.ldp_vae_trace(self._h, int(decode), _ptr(x), _ptr(out), n, _ptr(taps), nf.value, table.ctypes.data_as(C.c_void_p), ns.value,
                                     C.byref(ns), C.byref(nf), self._stream()))
        self.call_seq += 2
        assert ns.value == len(table) and nf.value == taps.numel()
        rows = []
        for r in table:
            off, N, H, W, ld, ch, kind, in0, in1, fam, nwn, ks, cpi, route, fused, nchw = (int(v) for v in r)
            shape = (N, ch, H, W) if nchw else (N, H, W, ld)
            rows.append(dict(kind=self.VAE_STAGE_KINDS[kind], inputs=tuple(i for i in (in0, in1) if i >= 0) or (-1,), family=self.VAE_FAMILIES[fam],
                             tile=(nwn, ks, cpi), stats=self.VAE_STATS_ROUTES[route], fused_out=bool(fused), channels=ch, nchw=bool(nchw),
                             t=taps[off:off + int(np.prod(shape))].view(shape)))
        return out, rows

    def _vae_noise_args(self, noise, n, seed, row_offset):
        s = self.image_size // 32
        eps = None if noise is None else _f32(noise, self.device)
        _want("noise", eps, (n, s, s, self.latent_channels))
        if int(row_offset) < 0:
            raise ValueError(f"row_offset must be >= 0, got {row_offset}")
        return eps, C.c_uint64(int(seed) & (2**64 - 1)), C.c_int64(int(row_offset))

    def vae_posterior(self, moments: torch.Tensor, noise: Optional[torch.Tensor] = None, seed: int = 0, row_offset: int = 0):
        """z = mean + exp(0.5 clip(logvar, -30, 20)) * eps and the per-image KL of (N, S/32, S/32, 2 LC) moments; eps = `noise` or the
        Philox stream (seed, global element, PHILOX_STREAM_VAE_EPS).  -> z (N, s, s, LC), std (same), kl (N,), (min, max, mean, std) of z."""
        m = _f32(moments, self.device)
        n, s, lc = m.shape[0], self.image_size // 32, self.latent_channels
        _want("moments", m, (n, s, s, 2 * lc))
        eps, seed_c, row_c = self._vae_noise_args(noise, n, seed, row_offset)
        z = torch.empty((n, s, s, lc), device=self.device, dtype=torch.float32)
        std, kl = torch.empty_like(z), torch.empty((n,), device=self.device, dtype=torch.float32)
        stats = torch.empty((4,), device=self.device, dtype=torch.float32)
        check(self.lib.ldp_vae_posterior(self._h, _ptr(m), _ptr(eps), seed_c, row_c, _ptr(z), _ptr(std), _ptr(kl), _ptr(stats), n,
                                         self._stream()))
        return z, std, kl, stats

    def vae_metrics(self, img_nhwc: torch.Tensor, use_kl: bool = True, beta: float = 1e-5, seed: int = 0,
                    noise: Optional[torch.Tensor] = None, row_offset: int = 0, want: Sequence[str] = ()):
        """StableVAEModel.loss forward in ONE call: the eleven scalars as an (11,) device tensor in _lib.VAE_METRIC_KEYS order.
        want: any of "z" (the posterior draw, (N, s, s, LC) NHWC) and "rec" (the reconstruction, (N, 3, S, S)) -> (metrics, {name: tensor})."""
        img = _f32(img_nhwc, self.device)
        n, s = img.shape[0], self.image_size
        _want("img_nhwc", img, (n, s, s, 3))
        bad = [w for w in want if w not in ("z", "rec")]
        if bad:
            raise ValueError(f"want={bad}: vae_metrics can return 'z' and 'rec'")
        if not np.isfinite(float(beta)):
            raise ValueError(f"beta must be finite, got {beta}")
        eps, seed_c, row_c = self._vae_noise_args(noise, n, seed, row_offset)
        out = torch.empty((len(_lib.VAE_METRIC_KEYS),), device=self.device, dtype=torch.float32)
        extra = {}
        if "z" in want:
            extra["z"] = torch.empty((n, s // 32, s // 32, self.latent_channels), device=self.device, dtype=torch.float32)
        if "rec" in want:
            extra["rec"] = torch.empty((n, 3, s, s), device=self.device, dtype=torch.float32)
        check(self.lib.ldp_vae_metrics(self._h, _ptr(img), n, int(bool(use_kl)), C.c_float(float(beta)), _ptr(eps), seed_c, row_c,
                                       _ptr(out), _ptr(extra.get("z")), _ptr(extra.get("rec")), self._stream()))
        self.call_seq += 1              # ONE call for the fault protocol, like vae_encode / vae_decode
        return out, extra

    # -- elementwise ----------------------------------------------------------------------------
    def normalize_bounds(self, x: torch.Tensor, lo, hi, normalize) -> torch.Tensor:
        """normalize: True/1 -> to [-1,1]; False/0 -> back (+clip); 2 -> plain clip to [lo, hi]."""
        x = _f32(x, self.device)
        lo_t, hi_t = self._bounds(lo, hi)
        dim = lo_t.numel()
        if dim != 1 and x.shape[-1] != dim:
            raise ValueError(f"bounds of length {dim} do not match trailing axis {x.shape[-1]}")
        y = torch.empty_like(x)
        check(self.lib.ldp_normalize_bounds(_ptr(x), _ptr(y), x.numel(), _ptr(lo_t), _ptr(hi_t), dim,
                                            int(normalize), self._stream()))
        return y

    def mean_sq_diff(self, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        """mean((a - b)^2) as a device scalar (the `plan_mse` of agent/ldp_agent.py:497-499)."""
        a, b = _f32(a, self.device), _f32(b, self.device)
        if a.shape != b.shape:
            raise ValueError(f"shapes differ: {tuple(a.shape)} vs {tuple(b.shape)}")
        out = torch.empty((), dtype=torch.float32, device=self.device)
        check(self.lib.ldp_mean_sq_diff(_ptr(a), _ptr(b), a.numel(), _ptr(out), self._stream()))
        return out

    def add_noise(self, x0: torch.Tensor, noise: torch.Tensor, t: torch.Tensor, n_train: int) -> torch.Tensor:
        """FlaxDDPMScheduler.add_noise (agent/ldp_agent.py:119,136): x0 / noise (rows, ...), t (rows,) int."""
        x0, noise = _f32(x0, self.device), _f32(noise, self.device)
        rows = x0.shape[0]
        td = torch.as_tensor(t).to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
        _want("noise", noise, x0.shape)
        _want("t", td, (rows,))
        out = torch.empty_like(x0)
        check(self.lib.ldp_add_noise(_ptr(x0), _ptr(noise), _ptr(td), int(n_train), _ptr(out), rows, x0.numel() // rows,
                                     self._stream()))
        return out

    def reduce_stats(self, x: torch.Tensor) -> torch.Tensor:
        """(min, max, mean, population std) of x as a device tensor of 4 (agent/ldp_agent.py:163-178)."""
        x = _f32(x, self.device)
        out = torch.empty((4,), dtype=torch.float32, device=self.device)
        check(self.lib.ldp_reduce_stats(_ptr(x), x.numel(), _ptr(out), self._stream()))
        return out

    def _bounds(self, lo, hi):
        """Device copies of normalisation bounds, cached by value: a policy call normalises 4-5 keys and would
        otherwise pay two small (synchronous, pageable) host-to-device copies for each."""
        if torch.is_tensor(lo) and torch.is_tensor(hi):
            return _f32(lo, self.device).reshape(-1), _f32(hi, self.device).reshape(-1)
        lo_a = np.atleast_1d(np.asarray(lo, dtype=np.float32))
        hi_a = np.atleast_1d(np.asarray(hi, dtype=np.float32))
        key = (lo_a.tobytes(), hi_a.tobytes())
        hit = self._bounds_cache.get(key)
        if hit is None:
            if len(self._bounds_cache) > 256:
                self._bounds_cache.clear()
            hit = (_f32(lo_a, self.device), _f32(hi_a, self.device))
            self._bounds_cache[key] = hit
        return hit

    # -- training step (include/ldp_hip.h "training step"; agent/ldp_agent.py:113-180, 223-323) -----------------------
    _MODS = {"planner": MOD_PLANNER, "idm": MOD_IDM, "vae": MOD_VAE}
    _MODS.update({f"encoder{i}": MOD_ENCODER << i for i in range(RESNET_SLOTS)})      # the ResNet image encoders as training modules

    def _mask(self, modules) -> int:
        if isinstance(modules, str):
            modules = [modules]
        m = 0
        for name in modules:
            m |= self._MODS[name]
        return m

    def train_init(self, modules) -> None:
        """TrainState.create for the listed modules from the parameters last uploaded (load_params): moments zero, step 0."""
        with torch.cuda.device(self.device):
            check(self.lib.ldp_train_init(self._h, self._mask(modules), self._stream()))

    def train_load(self, module: str, params: Dict[str, np.ndarray], mu=None, nu=None, step: int = 0, token=None) -> None:
        """TrainState.create(params) -- or a restored TrainState (mu / nu / step from a checkpoint) -- for one module.  The parameters go through
        ldp_set_weight, so the SAMPLING side of that module is un-finalized afterwards (train_publish / load_params rebuild it)."""
        for path, arr in params.items():
            a = np.ascontiguousarray(np.asarray(arr), dtype=np.float32)
            shape = (C.c_int64 * a.ndim)(*a.shape)
            check(self.lib.ldp_set_weight(self._h, f"{module}/{path}".encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim))
        self.loaded[module] = None
        self.train_init([module])
        if mu is not None:
            self.train_write(module, self.TRAIN_MU, mu)
        if nu is not None:
            self.train_write(module, self.TRAIN_NU, nu)
        if step:
            self.train_step_count(module, set_to=step)
        self.train_token[module] = token if token is not None else object()

    def _timesteps(self, t, n_train: int, what: str) -> torch.Tensor:
        """int32 device vector of training timesteps; the range is checked where the values live (host values: no device round trip)."""
        tt = torch.as_tensor(t)
        if tt.numel() == 0 or int(tt.min()) < 0 or int(tt.max()) >= n_train:
            raise ValueError(f"{what} timesteps must lie in [0, {n_train})")
        return tt.to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()

    def aux_streams(self) -> Dict[str, "torch.cuda.Stream"]:
        """Two more streams of this engine's device for the training step: the IDM's tape next to the planner's, the statistics scalars next to both."""
        if getattr(self, "_aux_streams", None) is None:
            self._aux_streams = {"idm": torch.cuda.Stream(device=self.device), "stats": torch.cuda.Stream(device=self.device)}
        return self._aux_streams

    def train_planner_grad(self, x0: torch.Tensor, noise: torch.Tensor, t, cond: Optional[torch.Tensor], alpha: float = 1.0) -> torch.Tensor:
        """alpha * plan_loss and its gradients (agent/ldp_agent.py:113-127): x0 / noise (B, T, D), t (B,), cond (B, G) -> device scalar."""
        x0, noise = _f32(x0, self.device), _f32(noise, self.device)
        B = x0.shape[0]
        td = self._timesteps(t, self.planner_train_steps, "planner")
        cond_t = None if cond is None else _f32(cond, self.device)
        _want("x0", x0, (B, self.T, self.D)); _want("noise", noise, (B, self.T, self.D)); _want("t", td, (B,)); _want("cond", cond_t, (B, self.G))
        loss = torch.empty((), dtype=torch.float32, device=self.device)
        check(self.lib.ldp_train_planner_grad(self._h, _ptr(x0), _ptr(noise), _ptr(td), _ptr(cond_t), C.c_float(alpha), _ptr(loss), B, self._stream()))
        self._keep = (x0, noise, td, cond_t)           # the launches are asynchronous: the inputs must outlive them
        return loss

    def train_planner_grad_cond(self, x0: torch.Tensor, noise: torch.Tensor, t, cond: torch.Tensor, alpha: float = 1.0):
        """train_planner_grad plus d loss / d cond (ldp_train_planner_grad_cond) -> (loss device scalar, dcond (B, G)): what DPTrainAgent
        trains its image encoders with.  Loss and gradient arena are bitwise train_planner_grad's."""
        x0, noise, cond_t = _f32(x0, self.device), _f32(noise, self.device), _f32(cond, self.device)
        B = x0.shape[0]
        td = self._timesteps(t, self.planner_train_steps, "planner")
        _want("x0", x0, (B, self.T, self.D)); _want("noise", noise, (B, self.T, self.D)); _want("t", td, (B,)); _want("cond", cond_t, (B, self.G))
        loss = torch.empty((), dtype=torch.float32, device=self.device)
        dcond = torch.empty((B, self.G), dtype=torch.float32, device=self.device)
        check(self.lib.ldp_train_planner_grad_cond(self._h, _ptr(x0), _ptr(noise), _ptr(td), _ptr(cond_t), C.c_float(alpha), _ptr(loss), _ptr(dcond), B,
                                                   self._stream()))
        self._keep = (x0, noise, td, cond_t)
        return loss, dcond

    def train_encoder_forward(self, slot: int, img_nhwc: torch.Tensor) -> torch.Tensor:
        """ResNetEncoder.apply on the MASTER parameters of training module encoder<slot>, every activation kept for train_encoder_backward:
        (N, 64, 64, 3) NHWC frames in [-1, 1] -> (N, 1024).  1 <= N <= 1024."""
        img = _f32(img_nhwc, self.device)
        n = img.shape[0]
        _want("img_nhwc", img, (n, 64, 64, 3))
        out = torch.empty((n, RESNET_FEATURES), device=self.device, dtype=torch.float32)
        check(self.lib.ldp_train_encoder_forward(self._h, int(slot), _ptr(img), _ptr(out), n, self._stream()))
        self._keep_e = getattr(self, "_keep_e", {})
        self._keep_e[int(slot)] = img
        return out

    def train_encoder_backward(self, slot: int, dfeat: torch.Tensor) -> None:
        """The VJP of the slot's last train_encoder_forward: the gradients of <dfeat, features> replace the gradient arena of encoder<slot>."""
        d = _f32(dfeat, self.device)
        n = d.shape[0]
        _want("dfeat", d, (n, RESNET_FEATURES))
        check(self.lib.ldp_train_encoder_backward(self._h, int(slot), _ptr(d), n, self._stream()))
        self._keep_d = getattr(self, "_keep_d", {})
        self._keep_d[int(slot)] = d

    def train_idm_grad(self, s: torch.Tensor, a0: torch.Tensor, noise: torch.Tensor, t, alpha: float = 1.0) -> torch.Tensor:
        """alpha * idm_loss and its gradients (agent/ldp_agent.py:129-140): s (R, 2D), a0 / noise (R, A), t (R,) -> device scalar."""
        s, a0, noise = _f32(s, self.device), _f32(a0, self.device), _f32(noise, self.device)
        R = s.shape[0]
        td = self._timesteps(t, self.idm_train_steps, "IDM")
        _want("s", s, (R, 2 * self.D)); _want("a0", a0, (R, self.A)); _want("noise", noise, (R, self.A)); _want("t", td, (R,))
        loss = torch.empty((), dtype=torch.float32, device=self.device)
        check(self.lib.ldp_train_idm_grad(self._h, _ptr(s), _ptr(a0), _ptr(noise), _ptr(td), C.c_float(alpha), _ptr(loss), R, self._stream()))
        self._keep_i = (s, a0, noise, td)
        return loss

    def train_vae_grad(self, img: torch.Tensor, use_kl: bool = True, beta: float = 1e-5, seed: int = 0, noise: Optional[torch.Tensor] = None,
                       row_offset: int = 0) -> torch.Tensor:
        """StableVAEModel.loss and its gradients (model/stable_vae_model.py:25-73) on module "vae"'s master parameters: img (N, S, S, 3) NHWC
        normalised frames -> the eleven metrics as an (11,) device tensor in _lib.VAE_METRIC_KEYS order; the gradients replace the module's
        gradient arena.  noise / seed / row_offset: the eps of the posterior draw, as vae_metrics."""
        img = _f32(img, self.device)
        if img.dim() != 4:
            raise ValueError(f"img must have shape (N, {self.image_size}, {self.image_size}, 3), got {tuple(img.shape)}")
        n = img.shape[0]
        _want("img", img, (n, self.image_size, self.image_size, 3))
        if not np.isfinite(float(beta)):
            raise ValueError(f"beta must be finite, got {beta}")
        eps, seed_c, row_c = self._vae_noise_args(noise, n, seed, row_offset)
        out = torch.empty((len(_lib.VAE_METRIC_KEYS),), device=self.device, dtype=torch.float32)
        check(self.lib.ldp_train_vae_grad(self._h, _ptr(img), n, int(bool(use_kl)), C.c_float(float(beta)), _ptr(eps), seed_c, row_c, _ptr(out),
                                          self._stream()))
        self._keep_v = [(img, eps)]                    # the launches are asynchronous: the inputs must outlive them
        return out

    def train_vae_grad_part(self, img: torch.Tensor, n_total: int, accumulate: bool, use_kl: bool = True, beta: float = 1e-5, seed: int = 0,
                            noise: Optional[torch.Tensor] = None, row_offset: int = 0) -> torch.Tensor:
        """train_vae_grad for PART of a batch (ldp_train_vae_grad_part): img holds N of the `n_total` frames whose mean loss is trained on,
        the first of them global frame `row_offset`; the gradients are (N / n_total) * those of these frames' own mean loss, and they
        replace the gradient arena (accumulate False: the first part of a step) or are added to it (True: every later part) -> the eleven
        metrics of THESE frames as an (11,) device tensor (vae_model.merge_vae_metrics merges the parts')."""
        img = _f32(img, self.device)
        if img.dim() != 4:
            raise ValueError(f"img must have shape (N, {self.image_size}, {self.image_size}, 3), got {tuple(img.shape)}")
        n = img.shape[0]
        _want("img", img, (n, self.image_size, self.image_size, 3))
        if not np.isfinite(float(beta)):
            raise ValueError(f"beta must be finite, got {beta}")
        eps, seed_c, row_c = self._vae_noise_args(noise, n, seed, row_offset)
        out = torch.empty((len(_lib.VAE_METRIC_KEYS),), device=self.device, dtype=torch.float32)
        check(self.lib.ldp_train_vae_grad_part(self._h, _ptr(img), n, int(n_total), int(accumulate), int(bool(use_kl)), C.c_float(float(beta)),
                                               _ptr(eps), seed_c, row_c, _ptr(out), self._stream()))
        if not accumulate or getattr(self, "_keep_v", None) is None:
            self._keep_v = []                          # a new step begins: the previous step's inputs may go
        self._keep_v.append((img, eps))                # every part's inputs outlive their launches
        return out

    def train_grad_norm(self, modules) -> torch.Tensor:
        out = torch.empty((), dtype=torch.float32, device=self.device)
        check(self.lib.ldp_train_grad_norm(self._h, self._mask(modules), _ptr(out), self._stream()))
        return out

    def train_apply(self, module: str, lr: float, b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8) -> None:
        check(self.lib.ldp_train_apply(self._h, self._MODS[module], C.c_float(lr), C.c_double(b1), C.c_double(b2), C.c_double(eps), self._stream()))

    def train_step_count(self, module: str, set_to: Optional[int] = None) -> int:
        v = C.c_int64()
        check(self.lib.ldp_train_step_count(self._h, self._MODS[module], C.c_int64(-1 if set_to is None else int(set_to)), C.byref(v)))
        return int(v.value)

    TRAIN_PARAMS, TRAIN_GRADS, TRAIN_MU, TRAIN_NU, TRAIN_EMA = 0, 1, 2, 3, 4

    def train_ema(self, module: str, decay: float) -> None:
        """TrainStateEMA(ema_decay=decay, ema_params=params): the module's EMA arena starts as a copy of its parameters; every later
        train_apply updates it in the same launch, every train_init / train_load re-seeds it from the parameters."""
        with torch.cuda.device(self.device):
            check(self.lib.ldp_train_ema(self._h, self._MODS[module], C.c_double(decay), self._stream()))
        self.ema_decay[module] = float(decay)

    def train_read(self, module: str, which: int, shapes) -> Dict[str, np.ndarray]:
        """{flax path: array} of the module's parameters / gradients / Adam moments; `shapes` = {path: shape} (weights.planner_shapes / idm_shapes)."""
        out = {}
        for path, shape in shapes.items():
            a = np.empty(tuple(shape), dtype=np.float32)
            check(self.lib.ldp_train_read(self._h, self._MODS[module], int(which), path.encode(), a.ctypes.data_as(C.c_void_p), a.size, self._stream()))
            out[path] = a
        return out

    def train_write(self, module: str, which: int, tree) -> None:
        for path, arr in tree.items():
            a = np.ascontiguousarray(np.asarray(arr), dtype=np.float32)
            check(self.lib.ldp_train_write(self._h, self._MODS[module], int(which), path.encode(), a.ctypes.data_as(C.c_void_p), a.size, self._stream()))

    def train_arena(self, module: str, which: int) -> torch.Tensor:
        """The module's flat parameter / gradient / moment arena as a 1-D float32 device tensor that ALIASES the engine's memory (no copy):
        what dist.update_sharded hands to the gradient all-reduce.  Valid until the next train_init."""
        ptr, n = C.c_void_p(), C.c_int64()
        check(self.lib.ldp_train_arena(self._h, self._MODS[module], int(which), C.byref(ptr), C.byref(n)))
        return _alias_device_f32(ptr.value, n.value, self.device)

    def train_publish(self, modules, versions: Optional[dict] = None) -> None:
        """The sampling path takes over the trained parameters (packed layouts and tables are rebuilt)."""
        with torch.cuda.device(self.device):
            check(self.lib.ldp_train_publish(self._h, self._mask(modules), self._stream()))
        for name in ([modules] if isinstance(modules, str) else modules):
            self.loaded[name] = (versions or {}).get(name, object())

    def train_publish_ema(self, modules, versions: Optional[dict] = None) -> None:
        """The sampling path takes over the EMA of the trained parameters (use_ema)."""
        with torch.cuda.device(self.device):
            check(self.lib.ldp_train_publish_ema(self._h, self._mask(modules), self._stream()))
        for name in ([modules] if isinstance(modules, str) else modules):
            self.loaded[name] = (versions or {}).get(name, object())

    def check_fault(self) -> None:
        """Synchronises the current stream and raises LDPHipFault if a fault (exchange time-out or fp16-plane range,
        poll_fault_kinds) was recorded since the last check / poll."""
        check(self.lib.ldp_check_fault(self._h, self._stream()))

    def launch_counts(self):
        n_conv, n_all = C.c_int64(), C.c_int64()
        check(self.lib.ldp_launch_count(self._h, 0, C.byref(n_conv)))
        check(self.lib.ldp_launch_count(self._h, 1, C.byref(n_all)))
        return n_conv.value, n_all.value


# ---- unit-testable primitives (no handle) -------------------------------------------------------
def _host(a):
    a = np.ascontiguousarray(np.asarray(a), dtype=np.float32)
    return a, a.ctypes.data_as(C.c_void_p)


def conv1d_gn_mish_film(x: torch.Tensor, kernel, bias, gn_scale, gn_bias,
                        film: Optional[torch.Tensor] = None) -> torch.Tensor:
    lib = _lib.load()
    x = x.contiguous().float()
    B, T, cin = x.shape
    k, kp = _host(kernel)
    b, bp = _host(bias)
    gs, gsp = _host(gn_scale)
    gb, gbp = _host(gn_bias)
    cout = k.shape[2]
    y = torch.empty((B, T, cout), device=x.device, dtype=torch.float32)
    f = None if film is None else film.contiguous().float()
    check(lib.ldp_conv1d_gn_mish_film_f32(_ptr(x), kp, bp, gsp, gbp, _ptr(f), _ptr(y), B, T, cin, cout,
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return y


def conv2d_3x3(x: torch.Tensor, kernel, bias, stride: int = 1) -> torch.Tensor:
    lib = _lib.load()
    x = x.contiguous().float()
    n, h, w, cin = x.shape
    k, kp = _host(kernel)
    b, bp = _host(bias)
    cout = k.shape[3]
    y = torch.empty((n, h // stride, w // stride, cout), device=x.device, dtype=torch.float32)
    check(lib.ldp_conv2d_3x3_f32(_ptr(x), kp, bp, _ptr(y), n, h, w, cin, cout, stride,
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return y


def conv2d_3x3_split(x: torch.Tensor, kernel, bias, res: Optional[torch.Tensor] = None, dual: bool = True,
                     with_stats: bool = False):
    """The stride-1 3x3 convolution on split bf16 operands (ldp_conv2d_3x3_bf16x3: what the StableVAE's 64 / 32 / 16
    pixel ResnetBlock2D convolutions run on).  dual = 2: on two fp16 planes / three products instead of three bf16 planes / six.
    -> y, or (y, per-256-pixel-tile column (sum, sum of squares))."""
    lib = _lib.load()
    x = x.contiguous().float()
    n, h, w, cin = x.shape
    k, kp = _host(kernel)
    b, bp = _host(bias)
    cout = k.shape[3]
    y = torch.empty((n, h, w, cout), device=x.device, dtype=torch.float32)
    st = torch.empty((n * h * w // 256, cout, 2), device=x.device, dtype=torch.float32) if with_stats else None
    if res is not None:
        res = res.contiguous().float()
    check(lib.ldp_conv2d_3x3_bf16x3(_ptr(x), kp, bp, _ptr(res) if res is not None else None, _ptr(y),
                                    _ptr(st) if st is not None else None, n, h, w, cin, cout, 2 if dual == 2 else 1 if dual else 0,
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return (y, st) if with_stats else y


# ---- primitives of the ResNet image encoder (csrc/resnet.hip) ----
def _cur():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def resnet_conv7x7_s2(x: torch.Tensor, kernel) -> torch.Tensor:
    """conv_init: 7x7, stride 2, padding (3, 3); x (N, 64, 64, 3), kernel (7, 7, 3, 64) -> (N, 32, 32, 64)."""
    x = x.contiguous().float()
    n, h, w, cin = x.shape
    k, kp = _host(kernel)
    if k.shape[:3] != (7, 7, cin):
        raise ValueError(f"kernel {k.shape} does not match x {tuple(x.shape)}")
    y = torch.empty((n, h // 2, w // 2, k.shape[3]), device=x.device, dtype=torch.float32)
    check(_lib.load().ldp_resnet_conv7x7_s2_f32(_ptr(x), kp, _ptr(y), n, h, w, cin, k.shape[3], _cur()))
    return y


def resnet_conv1x1_s2(x: torch.Tensor, kernel) -> torch.Tensor:
    """conv_proj: 1x1, stride 2; x (N, H, W, Cin), kernel (1, 1, Cin, Cout) -> (N, H / 2, W / 2, Cout)."""
    x = x.contiguous().float()
    n, h, w, cin = x.shape
    k, kp = _host(kernel)
    if k.shape[:3] != (1, 1, cin):
        raise ValueError(f"kernel {k.shape} does not match x {tuple(x.shape)}")
    y = torch.empty((n, h // 2, w // 2, k.shape[3]), device=x.device, dtype=torch.float32)
    check(_lib.load().ldp_resnet_conv1x1_s2_f32(_ptr(x), kp, _ptr(y), n, h, w, cin, k.shape[3], _cur()))
    return y


def resnet_maxpool3x3_s2(x: torch.Tensor) -> torch.Tensor:
    x = x.contiguous().float()
    n, h, w, c = x.shape
    y = torch.empty((n, h // 2, w // 2, c), device=x.device, dtype=torch.float32)
    check(_lib.load().ldp_resnet_maxpool3x3_s2_f32(_ptr(x), _ptr(y), n, h, w, c, _cur()))
    return y


def resnet_gn(x: torch.Tensor, scale, bias, groups: int = 4, eps: float = 1e-5, relu: bool = False, res: Optional[torch.Tensor] = None,
              scale2=None, bias2=None) -> torch.Tensor:
    """y = [relu](GN(x) [+ res | + GN'(res)]) on (N, ..., C); scale2 / bias2: `res` is normalised with its own statistics first."""
    x = x.contiguous().float()
    n, c = x.shape[0], x.shape[-1]
    hw = x.numel() // (n * c)
    s, sp = _host(scale)
    b, bp = _host(bias)
    if s.shape != (c,) or b.shape != (c,):
        raise ValueError(f"scale / bias must have shape ({c},)")
    s2p = b2p = None
    if scale2 is not None:
        s2, s2p = _host(scale2)
        b2, b2p = _host(bias2)
        if s2.shape != (c,) or b2.shape != (c,):
            raise ValueError(f"scale2 / bias2 must have shape ({c},)")
    r = None
    if res is not None:
        r = res.contiguous().float()
        _want("res", r, x.shape)
    y = torch.empty_like(x)
    check(_lib.load().ldp_resnet_gn_f32(_ptr(x), _ptr(r), _ptr(y), sp, bp, s2p, b2p, n, hw, c, int(groups), C.c_float(float(eps)),
                                       int(bool(relu)), _cur()))
    return y


def resnet_spatial_softmax(x: torch.Tensor) -> torch.Tensor:
    x = x.contiguous().float()
    n, h, w, c = x.shape
    out = torch.empty((n, 2 * c), device=x.device, dtype=torch.float32)
    check(_lib.load().ldp_resnet_spatial_softmax_f32(_ptr(x), _ptr(out), n, h, w, c, _cur()))
    return out


def downsample1d(x: torch.Tensor, kernel, bias) -> torch.Tensor:
    lib = _lib.load()
    x = x.contiguous().float()
    B, T, c = x.shape
    k, kp = _host(kernel)
    b, bp = _host(bias)
    y = torch.empty((B, T // 2, c), device=x.device, dtype=torch.float32)
    check(lib.ldp_downsample1d_f32(_ptr(x), kp, bp, _ptr(y), B, T, c,
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return y


def upsample1d(x: torch.Tensor, kernel, bias) -> torch.Tensor:
    lib = _lib.load()
    x = x.contiguous().float()
    B, T, c = x.shape
    k, kp = _host(kernel)
    b, bp = _host(bias)
    y = torch.empty((B, 2 * T, c), device=x.device, dtype=torch.float32)
    check(lib.ldp_upsample1d_f32(_ptr(x), kp, bp, _ptr(y), B, T, c,
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return y


class _DevSpan:
    """__cuda_array_interface__ (v2) over a span of device memory somebody else owns."""

    def __init__(self, ptr: int, numel: int):
        self.__cuda_array_interface__ = {"shape": (int(numel),), "typestr": "<f4", "data": (int(ptr), False), "version": 2, "strides": None}


def _alias_device_f32(ptr: int, numel: int, device) -> torch.Tensor:
    with torch.cuda.device(device):
        t = torch.as_tensor(_DevSpan(ptr, numel), device=torch.device("cuda", torch.cuda.current_device()))
    if t.data_ptr() != ptr:
        raise LDPHipError(-2, "torch copied the arena instead of aliasing it")
    return t


# ---- noise-source primitives (tests/test_philox.py) -------------------------------------------------
def philox_raw(seed: int, elem0: int, step: int, stream_id: int, n: int, device=None) -> torch.Tensor:
    """(n, 4) uint32 words of Philox4x32-10 at counters (elem0 + i, step, stream_id), key = seed."""
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    out = torch.empty((n, 4), device=dev, dtype=torch.int32)
    check(lib.ldp_philox_raw(_u64(seed), C.c_uint64(elem0 & (2**64 - 1)), C.c_uint32(step),
                             C.c_uint32(stream_id), _ptr(out), n, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return out


def philox_normal(seed: int, elem0: int, step: int, stream_id: int, n: int, device=None) -> torch.Tensor:
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    out = torch.empty((n,), device=dev, dtype=torch.float32)
    check(lib.ldp_philox_normal(_u64(seed), C.c_uint64(elem0 & (2**64 - 1)), C.c_uint32(step),
                                C.c_uint32(stream_id), _ptr(out), n, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return out
