"""A recording stand-in for HipEngine: the host logic of the training steps and of the weight hand-off runs on it without a GPU
(tests/test_vae_train_cpu.py, tests/test_update_host_cpu.py).  Every call appends a tuple to `calls`, its kind first; nothing is computed."""
import numpy as np
import torch


class TrainStub:
    TRAIN_PARAMS, TRAIN_GRADS, TRAIN_MU, TRAIN_NU, TRAIN_EMA = 0, 1, 2, 3, 4
    PLAN_LOSS, IDM_LOSS = 0.25, 0.5                       # what the two gradient calls return

    def __init__(self, grad_norm=3.0):
        self.loaded = {"planner": None, "idm": None, "vae": None}
        self.call_seq, self.fault_upto, self.last_fault_kinds = 0, -1, 0
        self.train_token, self.train_ema_token, self.ema_decay = {}, {}, {}
        self.calls = []
        self.grad_norm = grad_norm
        self.arenas = {}

    def kinds(self):
        return [c[0] for c in self.calls]

    def of(self, kind):
        return [c for c in self.calls if c[0] == kind]

    # ---- what every model class needs ----
    def normalize_bounds(self, x, lo, hi, normalize):
        lo, hi = (torch.as_tensor(np.asarray(v, np.float32)) for v in (lo, hi))
        if normalize == 2:                                # plain clip (utils/data_utils.py:61-65)
            return torch.maximum(torch.minimum(x, hi), lo)
        return (x - lo) / (hi - lo) * 2 - 1 if normalize else (x + 1) / 2 * (hi - lo) + lo

    def poll_fault_kinds(self):
        return 0

    def get_option(self, name):
        return 1 if name == "train_streams" else 0

    def aux_streams(self):
        return {}                                         # no side stream: the step must not touch a CUDA stream

    # ---- the sampling slots ----
    def load_params(self, planner=None, idm=None, vae=None, versions=None):
        trees = {k: v for k, v in (("planner", planner), ("idm", idm), ("vae", vae)) if v is not None}
        self.calls.append(("load_params", trees, dict(versions or {})))
        for k in trees:
            self.loaded[k] = (versions or {}).get(k, object())

    def train_publish(self, modules, versions=None):
        self.calls.append(("publish", list(modules), dict(versions or {})))
        for k in modules:
            self.loaded[k] = (versions or {}).get(k, object())

    def train_publish_ema(self, modules, versions=None):
        self.calls.append(("publish_ema", list(modules), dict(versions or {})))
        for k in modules:
            self.loaded[k] = (versions or {}).get(k, object())

    # ---- the training arenas ----
    def train_load(self, module, params, mu=None, nu=None, step=0, token=None):
        self.calls.append(("load", module, step, mu is None))
        self.loaded[module] = None
        self.train_token[module] = token

    def train_ema(self, module, decay):
        self.calls.append(("ema", module, decay))
        self.ema_decay[module] = decay

    def train_write(self, module, which, tree):
        self.calls.append(("write", module, which))

    def train_read(self, module, which, shapes):
        self.calls.append(("read", module, which))
        return {k: np.full((1,), which, np.float32) for k in shapes}

    def train_arena(self, module, which):
        self.calls.append(("arena", module, which))
        return self.arenas.setdefault((module, which), torch.ones(4))

    def train_apply(self, module, lr, b1=0.9, b2=0.999, eps=1e-8):
        self.calls.append(("apply", module, lr))

    def train_grad_norm(self, modules):
        self.calls.append(("grad_norm", list(modules)))
        return torch.tensor(self.grad_norm, dtype=torch.float32)

    # ---- one step's launches ----
    def reduce_stats(self, x):
        self.calls.append(("stats", x))
        return torch.stack([x.min(), x.max(), x.mean(), x.std(unbiased=False)]).float()

    def train_planner_grad(self, x0, noise, t, cond, alpha=1.0):
        self.calls.append(("planner_grad", x0, noise, np.asarray(t), cond, alpha))
        return torch.tensor(self.PLAN_LOSS)

    def train_idm_grad(self, s, a0, noise, t, alpha=1.0):
        self.calls.append(("idm_grad", s, a0, noise, np.asarray(t), alpha))
        return torch.tensor(self.IDM_LOSS)

    def train_vae_grad(self, img, use_kl, beta, seed=0, noise=None, row_offset=0):
        self.calls.append(("grad", tuple(img.shape), use_kl, beta, seed, row_offset))
        self.frames = img
        return torch.arange(11, dtype=torch.float32) + seed
