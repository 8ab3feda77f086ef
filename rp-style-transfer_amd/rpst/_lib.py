"""ctypes binding of librpst.so (the C ABI declared in include/rpst.h).

The header is the single statement of the ABI: every entry point's types and every RPST_*
code are parsed from it at import (parse_header), not written down here again.
The library is built in-tree (`make -C rp-style-transfer_amd/csrc`, or
`__graft_entry__.build()`) and loaded from there; RPST_LIB overrides the path.
There is no fallback: if the library is missing or a call fails, a RuntimeError is
raised with the library's own message (rpst_last_error()).
"""
from __future__ import annotations

import ctypes
import os
import re
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RPST_LIB", os.path.join(os.path.dirname(_HERE), "csrc", "librpst.so"))
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "rpst.h")

_P = ctypes.c_void_p
# scalar type in rpst.h -> ctypes; every pointer parameter is _P, whatever it points at
_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
            "double": ctypes.c_double, "size_t": ctypes.c_size_t, "rpst_stream_t": _P}


class RpstError(RuntimeError):
    pass


def parse_header(text: str):
    """The C ABI as rpst.h states it -> ({name: (restype, [argtypes])}, {"RPST_<NAME>": int}).

    A pure function of the header's text: `#define RPST_<NAME> <integer>` lines and prototypes
    `ret name(type name, ...);` of scalars and pointers inside the extern "C" frame. A statement
    that is no such prototype, or a type outside _SCALARS, raises RpstError: nothing is guessed."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = {m[1]: int(m[2]) for m in re.finditer(
        r"^[ \t]*#[ \t]*define[ \t]+(RPST_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, re.M)}
    text = re.sub(r'^[ \t]*#.*|extern\s+"C"\s*\{|\btypedef\b[^;]*;|\}', "", text, flags=re.M)

    def ctype(decl, name, named):
        words = [w for w in decl.replace("*", " * ").split() if w != "const"]
        if "*" in words:
            return _P if named or words != ["char", "*"] else ctypes.c_char_p
        kind = " ".join(words[:-1] if named and len(words) > 1 else words)
        if kind not in _SCALARS:
            raise RpstError(f"rpst.h: {name}: `{decl.strip()}` has type `{kind}`, which "
                            "rpst/_lib.py _SCALARS does not map")
        return _SCALARS[kind]

    signatures = {}
    for proto in filter(None, (" ".join(s.split()) for s in text.split(";"))):
        m = re.fullmatch(r"(.+?) ?\b(\w+) ?\(([^()\[\]]*)\)", proto)
        if not m:
            raise RpstError(f"rpst.h: `{proto}` is not a prototype the binding can read")
        ret, name, params = m.groups()
        params = [] if params.strip() in ("", "void") else params.split(",")
        signatures[name] = (ctype(ret, name, False), [ctype(p, name, True) for p in params])
    return signatures, constants


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            return parse_header(f.read())
    except OSError as e:
        raise RpstError(f"rpst: C ABI header not found at {HEADER_PATH} ({e})") from None


# name -> (restype, argtypes) and RPST_<NAME> -> value: what include/rpst.h declares. Mutable:
# a tool that loads an older library deletes the entries it lacks before load()
SIGNATURES, CONSTANTS = _read_header()


def constants(*names: str):
    """The header's RPST_<name> value for each name, in order (KeyError names a missing one)."""
    return tuple(CONSTANTS["RPST_" + n] for n in names)


_lib = None
_lock = threading.Lock()


def _bind(lib, signatures) -> None:
    """Give every declared entry point of lib its restype and argtypes."""
    for name, (res, args) in signatures.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise RpstError(f"rpst: {LIB_PATH} does not export {name}, which include/rpst.h "
                            "declares: the library is stale, rebuild it with "
                            "`make -C rp-style-transfer_amd/csrc`") from None
        fn.restype = res
        fn.argtypes = args


def load():
    """Load librpst.so once; raise RpstError if it is absent (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RpstError(
                f"rpst: HIP library not found at {LIB_PATH}; build it with "
                "`make -C rp-style-transfer_amd/csrc` or __graft_entry__.build()")
        lib = ctypes.CDLL(LIB_PATH)
        _bind(lib, SIGNATURES)
        _lib = lib
    return _lib


def check(status: int, what: str) -> None:
    if status != 0:
        msg = load().rpst_last_error().decode(errors="replace")
        raise RpstError(f"{what} failed (status {status}): {msg}")


def workspace_bytes(name: str, *dims) -> int:
    """rpst_<name>_workspace_size(*dims): the bytes the C call is told it has."""
    return getattr(load(), f"rpst_{name}_workspace_size")(*dims)


def scratch(nbytes: int, like):
    """The one workspace allocation, on like's device (16 bytes at least: never null)."""
    return torch.empty(max(nbytes, 16), device=like.device, dtype=torch.uint8)


def workspace(name: str, like, *dims):
    """Size and allocate the workspace of one launch -> (uint8 tensor, nbytes)."""
    nbytes = workspace_bytes(name, *dims)
    return scratch(nbytes, like), nbytes


def call(name: str, *args):
    """Call an rpst_* entry point that returns a status code; raise on failure."""
    st = getattr(load(), name)(*args)
    check(st, name)
