"""The C ABI as include/semicrf_hip.h states it.  The header is the contract; this module reads its text (no compiler, no
library) so that the ctypes prototypes and the SEMICRF_* integer constants of _lib.py cannot differ from it.  The type map is
closed: a declaration it does not cover raises, it is never guessed."""
from __future__ import annotations

import ctypes
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "semicrf_hip.h")


class SemiCRFLibraryError(RuntimeError):
    pass


_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
            "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double, "semicrf_stream_t": ctypes.c_void_p}
_INT_EXPR = re.compile(r"(?:(?:0[xX][0-9a-fA-F]+|[1-9][0-9]*|0)\b|<<|[-+|()]|\s)+")


def header_text(path: str = HEADER) -> str:
    with open(path) as f:
        return f.read()


def _code(text: str) -> str:
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def constants(text: str) -> dict:
    """{NAME: value} of every `#define SEMICRF_<NAME> <expr>` whose expression is made of integer literals, parentheses and
    << - + | only; any other #define is skipped."""
    out = {}
    for name, expr in re.findall(r"^[ \t]*#[ \t]*define[ \t]+SEMICRF_(\w+)[ \t]+(\S.*)$", _code(text), flags=re.M):
        if _INT_EXPR.fullmatch(expr):
            out[name] = int(eval(expr, {"__builtins__": {}}))
    return out


def _ctype(decl: str, fn: str, by_value: dict, result: bool = False):
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    if "*" in words:
        return ctypes.c_char_p if result and words == ["char", "*"] else ctypes.c_void_p
    if not result and words:
        words.pop()                             # the parameter's name
    kind = " ".join(words)
    if result and kind == "void":
        return None
    if kind in by_value:
        return by_value[kind]
    if kind not in _SCALARS:
        raise SemiCRFLibraryError(f"semicrf_hip.h: {fn}: no ctypes mapping for the type `{kind}` in `{decl.strip()}`")
    return _SCALARS[kind]


def prototypes(text: str, by_value: dict) -> dict:
    """{function: (restype, [argtypes])} of every prototype, in the header's order.  by_value: {struct typedef: ctypes class} of
    the structures that are passed by value."""
    text = re.sub(r"^[ \t]*#.*$", "", _code(text), flags=re.M)
    text = re.sub(r"typedef\s+struct\s+\w*\s*\{.*?\}\s*\w+\s*;", "", text, flags=re.S)
    text = re.sub(r"typedef\b[^;{]*;", "", text)
    text = re.sub(r'extern\s+"C"\s*\{|\}', "", text)
    out = {}
    for stmt in text.split(";"):
        if not stmt.strip():
            continue
        m = re.fullmatch(r"\s*([\w\s*]+?)\b(\w+)\s*\(([^()]*)\)\s*", stmt)
        if m is None:
            raise SemiCRFLibraryError(f"semicrf_hip.h: not a function prototype: `{' '.join(stmt.split())}`")
        res, fn, params = m.groups()
        params = [] if params.strip() in ("", "void") else params.split(",")
        out[fn] = (_ctype(res, fn, by_value, result=True), [_ctype(p, fn, by_value) for p in params])
    return out
