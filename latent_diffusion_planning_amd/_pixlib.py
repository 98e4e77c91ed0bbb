"""ctypes binding of libldp_pix.so (the C ABI in include/ldp_pix.h): the camera of the reach task of toyenv.py.

A library of its own beside libldp_hip.so and libldp_env.so, built by the same csrc/Makefile.  As in _lib.py and _envlib.py there is no
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
LIB_PATH = os.path.join(_HERE, "libldp_pix.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ldp_pix.h")

PIX_SIZE = 64                                      # LDP_PIX_SIZE: a frame is (64, 64, 3) uint8
PIX_FRAME_BYTES = PIX_SIZE * PIX_SIZE * 3          # LDP_PIX_FRAME_BYTES
PIX_EINVAL = -1                                    # LDP_PIX_EINVAL

_FP = C.c_void_p       # device pointers passed as integers from tensor.data_ptr()

# name -> (restype, argtypes); must list every symbol include/ldp_pix.h declares
SIGNATURES: Dict[str, tuple] = {
    "ldp_pix_last_error": (C.c_char_p, []),
    "ldp_pix_render": (C.c_int, [_FP, C.c_int64, _FP, C.c_int64, C.c_int64, _FP, C.c_void_p]),
}


def header_symbols(path: str = HEADER_PATH) -> List[str]:
    """Every function name declared in include/ldp_pix.h."""
    with open(path) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ldp_pix_[a-z0-9_]+)\s*\(", txt)))


_lib = None


def load() -> C.CDLL:
    """Load (once) and type the library.  Raises LDPHipUnavailable loudly when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LDPHipUnavailable(
            f"{LIB_PATH} is missing: the task's camera has no other implementation. "
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
        msg = load().ldp_pix_last_error()
        raise LDPHipError(code, msg.decode() if msg else "?")
