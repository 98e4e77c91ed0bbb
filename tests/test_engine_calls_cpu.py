"""What HipEngine's ten sampling methods hand to the C ABI, without a device: every method is called on an engine whose ctypes library
is a recording stub, once with every optional argument and once with none, and the recorded calls -- the symbol and, per argument, the
integer or the tensor's shape and dtype (None: a null pointer) -- are compared with tests/golden/engine_calls.json, which the same test
body wrote on the commit before the marshalling helpers (LDP_WRITE_ENGINE_CALLS=1 rewrites it).  The "all" case runs under sampler
"dpmpp", so the record also shows which methods register the solver's timestep table on first use and which leave that to the library."""
import ctypes as C
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from latent_diffusion_planning_amd.engine import HipEngine

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "engine_calls.json")
B, T, D, A, AH, N, H = 3, 8, 25, 7, 4, 10, 2


class _DeviceTensor(torch.Tensor):
    """A host tensor that says it lives on the device (x_store must: it is written in place)."""
    is_cuda = property(lambda self: True)


class _Recorder:
    """Stands in for the ctypes library: every symbol is a function that records its arguments and reports success."""

    def __init__(self, seen):
        self.calls, self._seen = [], seen

    def _value(self, v, ctype=None):
        if isinstance(v, C.Structure):
            return {name: self._value(getattr(v, name), ct) for name, ct in v._fields_}
        if hasattr(v, "_obj"):                               # C.byref(struct)
            return self._value(v._obj)
        pointer = ctype is C.c_void_p or isinstance(v, C.c_void_p)
        if hasattr(v, "value"):
            v = v.value
        if pointer:
            return None if v is None else self._seen.get(v, "host")
        return v if v is None else int(v)

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append({"symbol": name, "args": [self._value(a) for a in args]})
            return 0
        return fn


@pytest.fixture
def seen(monkeypatch):
    """address -> shape and dtype of every tensor whose address was taken"""
    seen, real = {}, torch.Tensor.data_ptr

    def data_ptr(t):
        p = real(t)
        seen[p] = {"shape": list(t.shape), "dtype": str(t.dtype).replace("torch.", "")}
        return p

    monkeypatch.setattr(torch.Tensor, "data_ptr", data_ptr)
    return seen


def _engine(seen):
    """A HipEngine without a handle or a device: the attributes the sampling methods read, around the recorder."""
    seen.clear()
    e = HipEngine.__new__(HipEngine)
    e.lib = _Recorder(seen)
    e.device = torch.device("cpu")
    e._h = C.c_void_p()                                  # (no handle: close() has nothing to destroy)
    e.D, e.A, e.G, e.T, e.ah = D, A, H * D, T, AH
    e.planner_train_steps = e.idm_train_steps = 100
    e.call_seq, e._bounds_cache, e.solver_tables = 0, {}, {}
    e._stream = lambda: C.c_void_p(0)
    return e


def _guide():
    z = lambda *s: torch.zeros(s)
    return SimpleNamespace(target=z(B, T, D), weight=z(B, T, D), anchor=z(B, D), lam=np.zeros(D, np.float32), beta=np.zeros(D, np.float32),
                           lo=-np.ones(D, np.float32), hi=np.ones(D, np.float32))


def _cases():
    """method -> {"all": (args, kwargs), "none": (args, kwargs)}"""
    z = lambda *s: torch.zeros(s)
    cond, obs = z(B, H * D), z(B, H, D)
    target, mask, rho = z(B, T, D), torch.zeros((B, T, D), dtype=torch.uint8), np.zeros(N, np.float32)
    store = lambda: torch.zeros((5, T, D)).as_subclass(_DeviceTensor)
    plan_all = dict(B=B, x_init=z(B, T, D), step_noise=z(N, B, T, D), seed=7, row_offset=2, sampler="dpmpp", n_steps=N, use_graph=False)
    agent_all = dict(x_noise=z(N, B, T, D), a_init=z(B * AH, A), a_noise=z(N, B * AH, A), seed=7, row_offset=2, sampler="dpmpp",
                     planner_steps=N, idm_steps=N, action_bounds=(-np.ones(A, np.float32), np.ones(A, np.float32)), action_mode=2,
                     use_graph=False)
    parts = dict(guide=_guide(), rho=rho, target=target, mask=mask, mode="clamp", x_store=store(), slot=[4, 0, 2], shift=1, step_begin=3)
    return {
        "plan_sample": {"all": ((cond,), plan_all), "none": ((cond,), {})},
        "plan_sample_range": {"all": ((cond, 2, 9), plan_all), "none": ((cond, 0, 100), {})},
        "plan_sample_constrained": {"all": ((cond, target, mask), dict(plan_all, mode="clamp", step_begin=2, step_end=9)),
                                    "none": ((cond, target, mask), {})},
        "plan_sample_guided": {"all": ((cond, _guide(), rho), dict(plan_all, step_begin=2, step_end=9)),
                               "none": ((cond, _guide(), np.zeros(100, np.float32)), {})},
        "plan_sample_composed": {"all": ((cond,), dict(plan_all, step_end=9, **parts)), "none": ((cond,), {})},
        "agent_sample": {"all": ((obs, H), dict(agent_all, x_init=z(B, T, D))), "none": ((obs, H), {})},
        "agent_resample": {"all": ((obs, H, store(), 3), dict(agent_all, slot=[4, 0, 2], shift=1)), "none": ((obs, H, store(), 0), {})},
        "agent_sample_constrained": {"all": ((obs, H, target, mask), dict(agent_all, x_init=z(B, T, D), mode="clamp")),
                                     "none": ((obs, H, target, mask), {})},
        "agent_sample_guided": {"all": ((obs, H, _guide(), rho), dict(agent_all, x_init=z(B, T, D))),
                                "none": ((obs, H, _guide(), np.zeros(100, np.float32)), {})},
        "agent_sample_composed": {"all": ((obs, H), dict(agent_all, x_init=z(B, T, D), **parts)), "none": ((obs, H), {})},
    }


def _record(seen):
    got = {}
    for method, cases in _cases().items():
        for case, (args, kwargs) in cases.items():
            e = _engine(seen)                      # a fresh engine: no timestep table registered yet
            out = getattr(e, method)(*args, **kwargs)
            outs = [out] if torch.is_tensor(out) else list(out)
            got[f"{method}/{case}"] = {"calls": e.lib.calls, "returns": [list(o.shape) for o in outs], "call_seq": e.call_seq}
    return got


def test_engine_calls_match_golden(seen):
    got = json.loads(json.dumps(_record(seen)))
    if os.environ.get("LDP_WRITE_ENGINE_CALLS") == "1":
        with open(GOLDEN, "w") as f:
            json.dump(got, f, indent=1, sort_keys=True)
            f.write("\n")
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key] == want[key], key


def test_shape_errors_keep_their_text(seen):
    z = lambda *s: torch.zeros(s)
    cond, obs = z(B, H * D), z(B, H, D)
    e = _engine(seen)
    with pytest.raises(ValueError, match=r"^x_init must have shape \(3, 8, 25\), got \(3, 8, 24\)$"):
        e.plan_sample(cond, x_init=z(B, T, D - 1))
    with pytest.raises(ValueError, match=r"^x_init must have shape \(3, 8, 25\), got \(2, 8, 25\)$"):
        e.agent_sample(obs, H, x_init=z(B - 1, T, D))
    with pytest.raises(ValueError, match=r"^a_noise must have shape \(10, 12, 7\), got \(10, 3, 4, 7\)$"):
        e.agent_sample(obs, H, a_noise=z(N, B, AH, A), idm_steps=N)
    with pytest.raises(ValueError, match=r"^action bounds must have length 1 or 7$"):
        e.agent_sample(obs, H, action_bounds=(-np.ones(3, np.float32), np.ones(3, np.float32)))
    with pytest.raises(ValueError, match=r"^action bounds must have length 1 or 7$"):
        e.agent_sample(obs, H, action_bounds=(-np.ones(A, np.float32), np.ones(1, np.float32)))
    assert e.lib.calls == [] and e.call_seq == 0             # refused before anything crossed the ABI
