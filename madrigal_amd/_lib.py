"""ctypes binding of libmadrigal_hip.so (the C ABI declared in include/madrigal_hip.h).

The product path has NO fallback: if the shared object is missing or a call fails, an
exception is raised.  The public header types the binding: ``declared_prototypes()`` parses
every ``mdg_*`` prototype and ``lib()`` sets ``restype`` / ``argtypes`` on every function from
it, so callers pass plain Python values (ints, floats, ``data_ptr()`` addresses, ``None``)
and ctypes checks their number and kind and converts them at full width.
"""
from __future__ import annotations

import ctypes
import os
import re
from typing import Dict, List, Tuple

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libmadrigal_hip.so")
HEADER = os.path.join(os.path.dirname(HERE), "include", "madrigal_hip.h")

_lib = None

_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "uint64_t": ctypes.c_uint64,
            "float": ctypes.c_float, "double": ctypes.c_double}
_PROTOTYPE = re.compile(r"([A-Za-z_][\w\s*]*?)\b(mdg_[a-z0-9_]+)\s*\(([^()]*)\)\s*;")


class MadrigalHipError(RuntimeError):
    pass


def _header_text() -> str:
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def declared_symbols() -> List[str]:
    """Names of all functions declared in include/madrigal_hip.h."""
    return sorted(set(re.findall(r"\b(mdg_[a-z0-9_]+)\s*\(", _header_text())))


def _ctype(spelling: str, fn: str, returned: bool = False):
    words = spelling.replace("*", " * ").split()
    if not returned and len(words) > 1 and words[-1] != "*":
        words = words[:-1]                                    # the parameter's name
    if words and words[-1] == "*":
        if not returned:
            return ctypes.c_void_p
        if words == ["const", "char", "*"]:
            return ctypes.c_char_p
    elif words == ["void"] and returned:
        return None
    elif len(words) == 1 and words[0] in _SCALARS:
        return _SCALARS[words[0]]
    raise MadrigalHipError(f"{fn}: no ctypes mapping for the {'return' if returned else 'parameter'} type {spelling.strip()!r}")


def parse_prototypes(text: str) -> Dict[str, Tuple[object, list]]:
    """{name: (restype, [argtypes])} of every ``mdg_*`` prototype in comment-free C ``text``; an unknown type spelling raises."""
    out = {}
    for ret, name, params in _PROTOTYPE.findall(text):
        params = [] if params.strip() in ("", "void") else params.split(",")
        out[name] = (_ctype(ret, name, returned=True), [_ctype(p, name) for p in params])
    return out


def declared_prototypes() -> Dict[str, Tuple[object, list]]:
    """Return and parameter ctypes of all functions declared in include/madrigal_hip.h."""
    text = _header_text()
    protos = parse_prototypes(text)
    missed = sorted(set(re.findall(r"\b(mdg_[a-z0-9_]+)\s*\(", text)) - set(protos))
    if missed:
        raise MadrigalHipError(f"include/madrigal_hip.h: cannot parse the prototype of {', '.join(missed)}")
    return protos


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MadrigalHipError(
                f"{LIB_PATH} not found: build it with `python -m madrigal_amd.build` "
                "(there is no CPU or PyTorch fallback for the HIP path)")
        # torch first: its wheel bundles its own libamdhip64; loading ours afterwards makes the dynamic linker bind
        # libmadrigal_hip.so to that same, already initialised HIP runtime (two runtimes in one process do not
        # share devices, streams or allocations).
        import torch  # noqa: F401
        handle = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in declared_prototypes().items():
            fn = getattr(handle, name)          # AttributeError here = header/library mismatch
            fn.restype, fn.argtypes = restype, argtypes
        _lib = handle
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().mdg_last_error().decode(errors="replace")
        if rc == -1:
            raise ValueError(f"{what}: {msg}")
        raise MadrigalHipError(f"{what} failed (code {rc}): {msg}")


def call(name: str, *args, what: str = "") -> None:
    """Call the status-returning entry point ``name`` and raise on a non-zero status (``what``: the label of the error, default
    ``name``).  The function is looked up on the handle at every call (CDLL keeps it in the instance dictionary)."""
    check(getattr(lib(), name)(*args), what or name)
