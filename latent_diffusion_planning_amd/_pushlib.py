"""ctypes binding of libldp_push.so (the C ABI in include/ldp_push.h): the device-resident pushing task of pushenv.py.

A library of its own beside libldp_hip.so, libldp_env.so and libldp_pix.so, built by the same csrc/Makefile.  As in _lib.py there is no
fallback: a missing library raises `LDPHipUnavailable` with the build command.  torch is imported first so that the library binds to the
libamdhip64 PyTorch-ROCm loaded.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Dict, List

from ._lib import LDPHipError, LDPHipUnavailable

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libldp_push.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ldp_push.h")

PHILOX_STREAM_PUSH = 14            # LDP_PHILOX_STREAM_PUSH: the reset and the scripted policies' noise
PUSH_STATE, PUSH_LATENT, PUSH_EPISODE_LEN = 12, 16, 48                # LDP_PUSH_*
PUSH_POLICIES = {"expert": 1, "straight": 2, "random": 3}             # LDP_PUSH_POLICY_* (0: given actions)

_FP = C.c_void_p       # device pointers passed as integers from tensor.data_ptr()

# name -> (restype, argtypes); must list every symbol include/ldp_push.h declares
SIGNATURES: Dict[str, tuple] = {
    "ldp_push_last_error": (C.c_char_p, []),
    "ldp_push_reset": (C.c_int, [_FP, C.c_int32, C.c_uint64, C.c_int64, C.c_void_p]),
    "ldp_push_observe": (C.c_int, [_FP, C.c_int32, _FP, _FP, _FP, C.c_void_p]),
    "ldp_push_step": (C.c_int, [_FP, C.c_int32, C.c_int32, _FP, C.c_int32, C.c_int32, C.c_float, C.c_uint64, C.c_int64, _FP, _FP, _FP, _FP,
                                C.c_void_p]),
}


def header_symbols(path: str = HEADER_PATH) -> List[str]:
    """Every function name declared in include/ldp_push.h."""
    with open(path) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ldp_push_[a-z0-9_]+)\s*\(", txt)))


_lib = None


def load() -> C.CDLL:
    """Load (once) and type the library.  Raises LDPHipUnavailable loudly when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LDPHipUnavailable(
            f"{LIB_PATH} is missing: the pushing task has no other implementation. "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'` (or `make -C latent_diffusion_planning_amd/csrc -j`).")
    try:
        import torch  # noqa: F401  (loads libamdhip64 / libhsa-runtime64 first)
    except Exception:  # pragma: no cover - torch is plumbing only
        pass
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:
        raise LDPHipUnavailable(f"could not load {LIB_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise LDPHipUnavailable(f"{LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(code: int) -> None:
    if code != 0:
        msg = load().ldp_push_last_error()
        raise LDPHipError(code, msg.decode() if msg else "?")
