"""Loader for the native library libmjx355.so (C ABI declared in include/mjx355.h).

The library is built in-tree (`mujoco-mjx-lab_amd/csrc/Makefile`, or `__graft_entry__.build()`).
There is no fallback: every entry point of the product path goes through this library, and a
missing library or GPU raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

from . import _srchash, abi
from ._header import HEADER, SCALARS

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MJX355_LIB", os.path.join(_HERE, "libmjx355.so"))  # override: A/B builds
CSRC = os.path.join(os.path.dirname(_HERE), "csrc")

# every symbol include/mjx355.h declares, in header order
EXPORTS = [name for _, name, _ in HEADER.protos]

# C type of the header -> ctypes: the structs and the handle outputs are typed, every other pointer
# (buffers, pointer tables, `void* stream`) is an address, scalars are SCALARS
_TYPED = {"mjlModelDesc*": C.POINTER(abi.ModelDesc), "mjlEnvConfig*": C.POINTER(abi.EnvConfigC),
          "mjlVisualDesc*": C.POINTER(abi.VisualDesc), "mjlModel**": C.POINTER(C.c_void_p),
          "mjlBatch**": C.POINTER(C.c_void_p), "mjlRenderer**": C.POINTER(C.c_void_p)}
_RETURNS = {"void": None, "char*": C.c_char_p}
_ERRORS = {v: k for k, v in HEADER.enums.items() if k.startswith("MJL_ERR_")}

_lib = None


def _ctype(t: str):
    return _TYPED.get(t) or (C.c_void_p if t.endswith("*") else SCALARS[t])


class MjlError(RuntimeError):
    pass


def source_hash() -> str:
    """sha256 prefix over the native sources (kernel + C ABI) of this tree (_srchash.py): the stamp a
    library built from them carries, and the key of recorded profiles."""
    return _srchash.source_hash(CSRC)


def stamped_hash(version: str) -> str:
    """The source hash a library stamped into its mjl_version() string ("... src=<hash>"), or ""."""
    return version.rsplit("src=", 1)[1].strip() if "src=" in version else ""


def build(force: bool = False):
    args = ["make", "-s", "-C", CSRC]
    if force:
        args.append("-B")
    subprocess.run(args, check=True)


def build_info() -> dict:
    """Which library this process runs and what it was built from (bench line, smoke)."""
    L = lib()
    v = L.mjl_version().decode()
    return {"lib": os.path.relpath(LIB_PATH, os.path.dirname(os.path.dirname(_HERE))), "version": v,
            "lib_src_hash": stamped_hash(v), "tree_src_hash": source_hash(),
            "override": "MJX355_LIB" in os.environ}


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MjlError(f"native library missing: {LIB_PATH} (run `make -C {CSRC}` or __graft_entry__.build())")
    L = C.CDLL(LIB_PATH)
    L.mjl_version.restype = C.c_char_p
    # provenance: the product library must have been built from this tree's sources. An explicit
    # MJX355_LIB (A/B and diagnostic builds) opts out of the check.
    if "MJX355_LIB" not in os.environ:
        built, tree = stamped_hash(L.mjl_version().decode()), source_hash()
        if built != tree:
            raise MjlError(f"stale native library {LIB_PATH}: built from sources {built or '(unstamped)'}, "
                           f"the tree's sources are {tree} (rebuild: make -C {CSRC})")
    for ret, name, args in HEADER.protos:
        fn = getattr(L, name)
        fn.restype = _RETURNS[ret] if ret in _RETURNS else _ctype(ret)
        fn.argtypes = [_ctype(a) for a in args]
    _lib = L
    return L


def check(rc: int):
    if rc != 0:
        raise MjlError(f"mjx355 error {rc} ({_ERRORS.get(rc, 'unknown code')}): {lib().mjl_last_error().decode()}")
