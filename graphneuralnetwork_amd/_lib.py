"""ctypes binding of libgnn_mi355x.so (the C-ABI in include/gnn_mi355x.h).

This is the Python-side FFI the reference's modules call into: plain device
pointers (``tensor.data_ptr()``), sizes and the current HIP stream handle go
across; nothing else.  The library is loaded lazily and only after ``torch``
(so that it binds to the HIP runtime torch already loaded).  There is no CPU
fallback: if the library is missing every op raises.
"""
from __future__ import annotations

import ctypes
import re
import threading
from pathlib import Path

import torch  # noqa: F401  (must be imported before the HIP library is dlopen'ed)

from . import build as _build

_lock = threading.Lock()
_lib: ctypes.CDLL | None = None

_SCALARS = {
    "int": ctypes.c_int,  # the same object as c_int32 on this platform
    "int32_t": ctypes.c_int32,
    "int64_t": ctypes.c_int64,
    "uint32_t": ctypes.c_uint32,
    "uint64_t": ctypes.c_uint64,
    "float": ctypes.c_float,
}


def _ctype(entry: str, decl: str, is_return: bool = False):
    """The ctypes type of one C type of the header. The map is closed: a type outside it raises
    (a guessed width would hand a kernel a wrong address, not raise)."""
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    base = " ".join(w for w in words if w != "*")
    stars = words.count("*")
    if stars:
        return ctypes.c_char_p if base == "char" and stars == 1 else ctypes.c_void_p
    if base == "void" and is_return:
        return None
    if base not in _SCALARS:
        raise ValueError(f"{entry}: type {decl.strip()!r} is outside the binding's type map")
    return _SCALARS[base]


def parse_header(text: str) -> dict[str, tuple]:
    """name -> (restype, argtypes, parameter names) of every ``ret gnn_name(params);`` in the
    text of a C header (comments and preprocessor lines ignored; a prototype may span lines)."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", " ", text, flags=re.M)
    out = {}
    for stmt in text.split(";"):
        stmt = re.split(r"[{}]", stmt)[-1].strip()  # what follows `extern "C" {`
        m = re.fullmatch(r"([\w\s*]+?)\b(gnn_\w+)\s*\((.*)\)", stmt, flags=re.S)
        if m is None:
            continue
        ret, name, params = m.groups()
        if name in out:
            raise ValueError(f"{name}: declared twice")
        argtypes, names = [], []
        if params.strip() != "void":
            for p in params.split(","):
                pm = re.fullmatch(r"([\w\s*]*?)(\w+)", p.strip())
                if pm is None:
                    raise ValueError(f"{name}: parameter {p.strip()!r} is not `type name`")
                argtypes.append(_ctype(name, pm.group(1)))
                names.append(pm.group(2))
        out[name] = (_ctype(name, ret, is_return=True), argtypes, tuple(names))
    return out


# name -> (restype, argtypes) and name -> parameter names, read from include/gnn_mi355x.h: the
# header is the one description of the C ABI
_PROTOTYPES = parse_header(_build.HEADER.read_text())
SIGNATURES: dict[str, tuple] = {n: (res, args) for n, (res, args, _) in _PROTOTYPES.items()}
PARAMS: dict[str, tuple] = {n: names for n, (_, _, names) in _PROTOTYPES.items()}

EPI_RELU = 1
EPI_ELU = 2
EPI_ACCUMULATE = 4
EPI_SKIP_EMPTY = 8
E_ARG = -1
E_ALIGN = -2
E_UNSUPPORTED = -3


def library_path() -> Path:
    return _build.LIB_PATH


def load(build_if_missing: bool = False) -> ctypes.CDLL:
    """dlopen libgnn_mi355x.so and bind every C-ABI symbol (raises if absent)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        path = library_path()
        if not path.exists():
            if not build_if_missing:
                raise RuntimeError(
                    f"{path} is missing: build it with `python -m graphneuralnetwork_amd.build` "
                    "(the MI355X aggregation ops have no CPU fallback)")
            _build.build()
        lib = ctypes.CDLL(str(path), mode=ctypes.RTLD_GLOBAL)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        check_stamp(lib)
        _lib = lib
        return lib


def build_stamp(lib=None) -> str:
    """The source stamp embedded in the loaded library (``gnn_build_stamp()``)."""
    return (lib or load()).gnn_build_stamp().decode()


def check_stamp(lib) -> None:
    """Refuse a library not built from this tree's sources: a stale
    prebuilt .so would otherwise run silently under a newer tree's tests and bench."""
    built, tree = lib.gnn_build_stamp().decode(), _build.lib_source_stamp()
    if built != tree:
        raise RuntimeError(
            f"{library_path()} was built from sources with stamp {built}, but this tree's are "
            f"{tree}: rebuild with `python -m graphneuralnetwork_amd.build`")
    if lib.gnn_build_defines().decode():
        raise RuntimeError(f"{library_path()} is a tuning-variant build "
                           f"({lib.gnn_build_defines().decode()}), not the product library")


def use_variant(path) -> ctypes.CDLL:
    """Kernel-tuning hook (tools/*_ab.py): route every op through another build
    of the same C-ABI (``build.build_variant``); ``use_variant(None)`` restores."""
    global _lib
    if path is None:
        _lib = None
        return load()
    lib = ctypes.CDLL(str(path), mode=ctypes.RTLD_LOCAL)
    if not hasattr(lib, "gnn_build_stamp"):
        raise RuntimeError(f"{path}: no gnn_build_stamp (built before round 6); rebuild it")
    for name, (res, args) in SIGNATURES.items():
        try:  # an older build may lack entries added since (A/B of a previous tree)
            fn = getattr(lib, name)
        except AttributeError:
            continue
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def error_string(code: int) -> str:
    return load().gnn_error_string(int(code)).decode()


def check(code: int, what: str) -> None:
    if code != 0:
        raise RuntimeError(f"{what} failed with code {code}: {error_string(code)}")


def invoke(name: str, **kw) -> int:
    """Call entry ``name`` of the currently loaded library with its arguments given by the
    header's parameter names, each exactly once; returns the entry's return code."""
    names = PARAMS[name]
    if len(kw) != len(names) or not all(n in kw for n in names):
        missing = [n for n in names if n not in kw]
        unknown = [k for k in kw if k not in names]
        raise TypeError(f"{name}: missing arguments {missing}, unknown arguments {unknown}; "
                        f"the header declares {list(names)}")
    return getattr(load(), name)(*[kw[n] for n in names])


def run(name: str, **kw) -> None:
    """``invoke`` that raises on a nonzero return code."""
    check(invoke(name, **kw), name)


def ptr(t) -> int | None:
    """Device address of a tensor (None for an absent optional operand)."""
    return None if t is None else t.data_ptr()


def stream_handle(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream
