"""ORACLE (test infrastructure, NOT a product path) -- the camera of the reach task, `ldp_pix_render` of csrc/pix.hip (include/ldp_pix.h,
DESIGN.md 4.22), restated in NumPy float32: every operation rounded once, fused multiply-adds through toyenv_oracle.fma32 (exact, via
float64 rounded to odd).  The kernel must reproduce every byte of this file's frames.

`NumpyReach2DPixelEnv` has the interface of toyenv.Reach2DPixelEnv on host arrays: harness.run_device_eval runs on it without a GPU."""
from __future__ import annotations

import numpy as np

from tests import toyenv_oracle as O
from tests.toyenv_oracle import fma32

F32 = np.float32
SIZE = 64
K_POINT, K_DISC = F32(16.0), F32(11.111111)
ONE, HALF, B255 = F32(1), F32(0.5), F32(255)
CENTRES = ((2 * np.arange(SIZE) - (SIZE - 1)).astype(F32) * F32(2.0 ** -6)).astype(F32)         # c_k = (2k - 63) * 2^-6, exact


def blob(q, K):
    """q (M, 2) float32 centres -> (M, 64, 64) uint8: row i at y = c_i (row 0 is the bottom), column j at x = c_j."""
    q = np.asarray(q, F32).reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = (CENTRES[None, None, :] - q[:, 0, None, None]).astype(F32)                         # (M, 1, 64)
        dy = (CENTRES[None, :, None] - q[:, 1, None, None]).astype(F32)                         # (M, 64, 1)
        d2 = fma32(dx, dx, (dy * dy).astype(F32))                                               # (M, 64, 64)
        t = fma32(-d2, F32(K), ONE)
        s = np.where(t > 0, t, F32(0)).astype(F32)                                              # NaN -> 0
        v = (s * s).astype(F32)
        return np.trunc(fma32(B255, v, HALF)).astype(np.uint8)


def render(pos, goal):
    """pos, goal: (M, 2) views of any stride (two floats read per row) -> frames (M, 64, 64, 3) uint8: R the point, G the goal, B the disc."""
    pos, goal = np.asarray(pos, F32), np.asarray(goal, F32)
    assert pos.ndim == 2 and pos.shape[1] == 2 and pos.shape == goal.shape
    M = pos.shape[0]
    out = np.empty((M, SIZE, SIZE, 3), np.uint8)
    out[..., 0], out[..., 1] = blob(pos, K_POINT), blob(goal, K_POINT)
    out[..., 2] = blob(np.zeros((1, 2), F32), K_DISC)
    return out


def render_state(state):
    """The live state (N, 8): pos = state[:, 0:2], goal = state[:, 2:4] (strides 8)."""
    state = np.asarray(state, F32)
    return render(state[:, 0:2], state[:, 2:4])


class NumpyReach2DPixelEnv(O.NumpyReach2DEnv):
    """toyenv.Reach2DPixelEnv on the host: the goal is visible in the frame's G channel only."""

    def observe(self):
        return {"obs": {"pos": self.state[:, None, 0:2].copy(), "image": render_state(self.state)[:, None]}}

    def goal_observation(self):
        g = self.state[:, 2:4]
        return {"pos": g[:, None].copy(), "image": render(g, g)[:, None]}
