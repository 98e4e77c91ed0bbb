"""Warm-started replanning for closed-loop control (defined by this repository -- the reference starts every policy call
from pure noise).

Between two control calls the world moves by `action_horizon` states, so the plan just computed, shifted by that many positions and noised
to an intermediate level, starts a loop that runs only the last `warm_steps` of `n_steps` denoising steps (Janner et al. 2022, "Planning
with Diffusion", 5.4).  `Replanner` keeps the previous full planner state of every environment in a device table and decides per row whether
a call can be warm (`LDPAgent.replanner`); `LDPAgent.sample_warm` is the same computation for a caller who carries the state itself.

Whether warm-started plans control as well as cold ones has been measured on a toy task only (tools/toy_reach.py): this
module defines and tests the computation.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from .arrays import DeviceArray


def check_warm_steps(warm_steps, n_steps: int) -> int:
    """warm_steps = k runs the last k planner steps: 1 <= k <= n_steps -> step_begin = n_steps - k."""
    k = int(warm_steps)
    if not 1 <= k <= int(n_steps):
        raise ValueError(f"warm_steps must lie in 1..n_steps = {int(n_steps)}, got {warm_steps}")
    return int(n_steps) - k


def group_rows(valid: Sequence[bool], slots: Sequence[int]):
    """The one rule of Replanner.act: rows are reordered stably, warm rows (valid slot) first, then cold rows
    -> (order, n_warm): order[p] = caller's row at reordered position p."""
    warm = [i for i, s in enumerate(slots) if valid[s]]
    cold = [i for i, s in enumerate(slots) if not valid[s]]
    return warm + cold, len(warm)


class Replanner:
    """The previous planner state x (T, D) of `n_slots` environments, on the device, and a host flag per slot saying whether it holds one.

    act(batch, eval_rng, slots): row i of the batch belongs to environment slots[i].  Rows are reordered stably, warm rows first, then
    cold rows; each group is ONE contiguous engine call whose row_offset is the group's first position in the reordered batch -- warm rows
    `agent_resample` (warm initial state from the table, the last warm_steps steps, the new state written back in place), cold rows the
    full loop of `agent_sample`, whose x is then stored -- and the results come back in the caller's row order.  The result is a
    deterministic function of (weights, batch, seed, slots, valid flags).  reset(slots) invalidates slots (episode boundaries).

    Faults (include/ldp_hip.h, fault protocol): a warm row overwrites its slot, so a call cannot be repeated as it was.  Both the retry
    inside act() (the engine refused a call because of an earlier, unread fault) and the recompute at the first read of a faulted call's
    results run every row cold -- a valid plan -- and a late recompute stores only the slots no later act() has written.  Plans that later
    calls warm-started from a faulted state are themselves suspect (a fault marks every call enqueued before its poll) and are recomputed
    cold when THEY are read; a caller that never reads a call's results never learns of its fault, as with sample()."""

    def __init__(self, agent, n_slots: int, warm_steps: int, sampler: str = "ddim", n_steps: Optional[int] = None,
                 shift: Optional[int] = None):
        cfg = agent.config
        if int(n_slots) < 1:
            raise ValueError(f"n_slots must be >= 1, got {n_slots}")
        self.agent = agent
        self.n_slots = int(n_slots)
        self.sampler = sampler
        self.n_steps = int(cfg["planner_n_diffusion_steps"] if n_steps is None else n_steps)
        self.warm_steps = int(warm_steps)
        self.step_begin = check_warm_steps(warm_steps, self.n_steps)
        self.shift = int(cfg["action_horizon"] if shift is None else shift)
        if self.shift < 0:
            raise ValueError(f"shift must be >= 0, got {shift}")
        self.idm_steps = self.n_steps if sampler != "ddpm" else None        # one schedule for both loops, as sample_viz
        self.valid: List[bool] = [False] * self.n_slots
        self.table = None                                   # (n_slots, T, D) device tensor, allocated by the first act()
        self.calls = dict(warm=0, cold=0)                   # engine calls made so far, per kind
        self.gen: List[int] = [0] * self.n_slots            # act() calls that wrote each slot (a late fault recompute must not overwrite newer plans)
        self._slot_cache = {}                               # (slots, dtype) -> device tensor: a control loop repeats a few slot patterns

    def _slots(self, slots) -> List[int]:
        s = [int(v) for v in np.asarray(slots).reshape(-1)]
        bad = [v for v in s if not 0 <= v < self.n_slots]
        if bad:
            raise ValueError(f"slots must lie in 0..{self.n_slots - 1}, got {bad}")
        if len(set(s)) != len(s):
            raise ValueError(f"slots must be distinct within a call, got {s}")
        return s

    def reset(self, slots=None) -> None:
        """Invalidate `slots` (all of them with None): their next row starts from pure noise."""
        for s in (range(self.n_slots) if slots is None else self._slots(slots)):
            self.valid[s] = False

    def _table(self):
        if self.table is None:
            cfg = self.agent.config
            self.table = torch.zeros((self.n_slots, cfg["pred_horizon"], cfg["obs_dim"]), device=self.agent._device, dtype=torch.float32)
        return self.table

    def _dev_slots(self, slots, dtype):
        """The (already validated) slots as a device tensor, kept per pattern: the engine then takes the table as it is, with no host check
        and no copy from pageable host memory in front of every control call."""
        key = (tuple(slots), dtype)
        t = self._slot_cache.get(key)
        if t is None:
            if len(self._slot_cache) >= 64:
                self._slot_cache.clear()
            t = self._slot_cache[key] = torch.as_tensor(list(slots), dtype=dtype).to(self.agent._device)
        return t

    def _warm_call(self, eng, emb, table, slot_t, rows, extras, kw):
        """The engine call of the warm group: emb its rows (reordered), slot_t their slots on the device, rows their indices in the
        caller's batch -> (x, plan, action).  Controller overrides this."""
        return eng.agent_resample(emb, self.agent.config["obs_horizon"], table, self.step_begin, slot=slot_t, shift=self.shift, row_offset=0, **kw)

    def _cold_call(self, eng, emb, rows, row_offset, extras, kw):
        """The engine call of the cold group -> (x, plan, action).  Controller overrides this."""
        return eng.agent_sample(emb, self.agent.config["obs_horizon"], row_offset=row_offset, **kw)

    def _run(self, batch, seed, slots, order, n_warm, keep=None, extras=None):
        """The engine calls of one act() -> [action, plan, x] in the caller's row order (device tensors).  keep: per reordered cold row,
        whether its x is stored (None: all).  extras: what a subclass hands its group calls (Replanner: nothing)."""
        ag = self.agent
        eng, cfg = ag._engine, ag.config
        ag._sync_weights()
        obs_emb = ag.get_obs_cond(ag._vae_encode_t(ag._postprocess(batch)["obs"])).contiguous()
        if obs_emb.shape[0] != len(slots):
            raise ValueError(f"the batch has {obs_emb.shape[0]} rows but {len(slots)} slots were given")
        dev = obs_emb.device
        identity = list(order) == list(range(len(order)))      # the steady state of a control loop (all rows warm): nothing to reorder
        perm = None if identity else torch.as_tensor(order, device=dev, dtype=torch.long)
        emb = obs_emb if identity else obs_emb[perm].contiguous()
        lo, hi, mode = ag._action_bounds()
        table = self._table()
        kw = dict(seed=seed, sampler=self.sampler, planner_steps=self.n_steps, idm_steps=self.idm_steps, action_bounds=(lo, hi),
                  action_mode=mode)
        parts = []
        if n_warm:
            parts.append(self._warm_call(eng, emb[:n_warm], table, self._dev_slots([slots[i] for i in order[:n_warm]], torch.int32),
                                         list(order[:n_warm]), extras, kw))
            self.calls["warm"] += 1
        if n_warm < len(order):
            x, plan, act = self._cold_call(eng, emb[n_warm:], list(order[n_warm:]), n_warm, extras, kw)
            cold = [slots[i] for i in order[n_warm:]]
            if keep is None:
                table.index_copy_(0, self._dev_slots(cold, torch.long), x)
            elif any(keep):
                rows = [r for r, k in enumerate(keep) if k]
                table.index_copy_(0, self._dev_slots([cold[r] for r in rows], torch.long), x[self._dev_slots(rows, torch.long)])
            parts.append((x, plan, act))
            self.calls["cold"] += 1
        x, plan, act = parts[0] if len(parts) == 1 else (torch.cat([p[k] for p in parts]) for k in range(3))
        if not identity:                                   # back to the caller's row order
            inv = torch.empty_like(perm)
            inv[perm] = torch.arange(len(order), device=dev)
            x, plan, act = x[inv], plan[inv], act[inv]
        return [act, plan, x]

    def act(self, batch, eval_rng, slots, decode: bool = False):
        """-> (action (B, ah, A), metrics) like LDPAgent.sample_viz, plus metrics['x'] (B, T, D), in the caller's row order."""
        return self._act(batch, eval_rng, self._slots(slots), decode, None)

    def _act(self, batch, eval_rng, slots, decode, extras):
        """act() on validated slots; extras: what a subclass hands its group calls, the same in the first attempt, the retry and a late recompute."""
        from .agent import _seed_of
        ag = self.agent
        seed = _seed_of(eval_rng)
        order, n_warm = group_rows(self.valid, slots)

        straight = list(range(len(slots)))
        attempts = [0]

        def run():
            # the first attempt follows the grouping rule.  If the engine refuses one of its calls because of an earlier, unread fault,
            # the warm rows of this attempt may already have overwritten their slots: the retry runs every row cold
            attempts[0] += 1
            if attempts[0] == 1:
                return self._run(batch, seed, slots, order, n_warm, extras=extras)
            return self._run(batch, seed, slots, straight, 0, extras=extras)

        def recompute():
            # a fault invalidated this call AFTER its warm rows overwrote their slots: the previous states are gone, so the recompute
            # runs every row cold, in the caller's order (a valid plan; the handle has changed its launch mode by then anyway).  It runs
            # when the call's results are first read, possibly after later act() calls: only slots no later call has written are stored
            # (those later calls are suspect too -- a fault marks every call enqueued before its poll -- and recompute cold themselves).
            return self._run(batch, seed, slots, straight, 0, keep=[self.gen[s] == mine[s] for s in slots], extras=extras) + [None]
        res, rec = ag._call(run, recompute)
        for s in slots:
            self.valid[s] = True
            self.gen[s] += 1
        mine = {s: self.gen[s] for s in slots}
        return ag._plan_metrics(res, rec, ("x",), decode)


class Controller(Replanner):
    """A Replanner whose rows can also be steered (`LDPAgent.controller`): act() takes a guide and / or a constraint, and
    runs under any sampler, "dpmpp" included.  The grouping rule, the slot table, the fault retry and the recompute are Replanner's; its
    warm and cold group calls go through `agent_sample_composed`, which hands each group its rows of the guide and the constraint.  With
    neither, and under DDPM / DDIM, the results are Replanner's bit for bit.

    Whether such plans control well has been measured on a toy task only: there is no robot checkpoint and no robot simulator here."""

    def act(self, batch, eval_rng, slots, guide=None, decode: bool = False, **constraint_kw):
        """Replanner.act with `guide` (a guide.Guide for the B rows of this call, in the caller's row order; anchor=True: each row's own
        last observation embedding) and a constraint in constrain.build_constraint's keywords (target, mask, goal, t_goal, goal_dims)
        plus mode ('repaint' / 'clamp').  Every refusal is raised before any engine call."""
        from .constrain import MODES, build_constraint
        from .guide import Guide
        ag = self.agent
        slots = self._slots(slots)
        B = len(slots)
        mode = constraint_kw.pop("mode", "repaint")
        unknown = sorted(set(constraint_kw) - {"target", "mask", "goal", "t_goal", "goal_dims"})
        if unknown:
            raise TypeError(f"act() got unexpected keyword arguments {unknown}")
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
        extras = dict(guide=None, rho=None, target=None, mask=None, mode=mode)
        if guide is not None:
            if not isinstance(guide, Guide):
                raise ValueError(f"guide must be a guide.Guide (guide.build_guide / LDPAgent.build_guide), got {type(guide).__name__}")
            if guide.B != B:
                raise ValueError(f"the guide was built for B = {guide.B} plans, the call holds {B} rows")
            extras["guide"], extras["rho"] = guide, ag._guide_step_sizes(guide, self.sampler, self.n_steps)
        if any(v is not None for v in constraint_kw.values()):
            goal = constraint_kw.get("goal")
            kw = dict(constraint_kw, goal=None if goal is None else ag._goal_embedding(goal, B))
            if kw.get("target") is not None:
                kw["target"] = ag._t(kw["target"])
            tg, mk = build_constraint(ag.config, B, **kw)
            extras["target"], extras["mask"] = ag._t(tg), torch.as_tensor(mk)
        return self._act(batch, eval_rng, slots, decode, extras)

    def _parts(self, emb, rows, extras):
        """The rows of the guide and the constraint that belong to one group call, as agent_sample_composed's keywords."""
        from .guide import Guide
        kw = dict(mode=extras["mode"])
        gd = extras["guide"]
        if gd is not None:
            oh = self.agent.config["obs_horizon"]
            anchor = emb[:, oh - 1].contiguous() if gd.anchor is True else None if gd.anchor is None else self.agent._t(gd.anchor)[rows]
            kw["guide"] = Guide(gd.cfg, len(rows), gd.target[rows], gd.weight[rows], anchor, gd.lam, gd.beta, gd.lo, gd.hi, gd.scale,
                                gd.schedule, gd.engine, gd.wmax)
            kw["rho"] = extras["rho"]
        if extras["target"] is not None:
            kw["target"], kw["mask"] = extras["target"][rows], extras["mask"][rows]
        return kw

    def _warm_call(self, eng, emb, table, slot_t, rows, extras, kw):
        return eng.agent_sample_composed(emb, self.agent.config["obs_horizon"], x_store=table, slot=slot_t, shift=self.shift,
                                         step_begin=self.step_begin, row_offset=0, **self._parts(emb, rows, extras), **kw)

    def _cold_call(self, eng, emb, rows, row_offset, extras, kw):
        return eng.agent_sample_composed(emb, self.agent.config["obs_horizon"], row_offset=row_offset, **self._parts(emb, rows, extras), **kw)
