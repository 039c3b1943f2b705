"""ctypes loader of libazhip.so -- the only way the Python host code reaches the
HIP kernels.  There is NO fallback: if the library is missing or a call fails,
a RuntimeError is raised (the product path never routes through oracle/ or a
CPU restatement)."""
import ctypes
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AZ_LIB_PATH") or os.path.join(HERE, "lib", "libazhip.so")  # AZ_LIB_PATH: kernel A/B experiments
HEADER = os.path.join(HERE, "..", "include", "azhip.h")

_lib = None

_C = ctypes
_PTR, _INT = _C.c_void_p, _C.c_int
_SCALARS = {"int": _INT, "long long": _C.c_longlong, "float": _C.c_float, "double": _C.c_double, "size_t": _C.c_size_t}
_FIELDS = {"int": "i4", "long long": "i8"}  # members of the descriptor structs; a pointer is "u8"
_DIRECTIVES = re.compile(r"#\s*(ifndef AZHIP_H|ifdef __cplusplus|endif|include\s*<\w+\.h>|define AZHIP_H)\s*")
_CALL = re.compile(r"\baz_[a-z0-9_]+\s*\(")
_PROTO = re.compile(r"([\w\s*]*?)\b(az_[a-z0-9_]+)\s*\(([^()]*)\)\s*;")
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;")


def _ctype(decl, where):
    """ctypes type of `type [name]`: any pointer is a void pointer, except `const char *`"""
    decl = " ".join(decl.split())
    if "*" in decl:
        return _C.c_char_p if decl.split("*")[0].strip() == "const char" else _PTR
    m = re.fullmatch(r"(?:const )?(int|long long|float|double|size_t)(?: \w+)?", decl)
    if m is None:
        raise RuntimeError(f"azhip.h: {where}: unknown type in '{decl}'")
    return _SCALARS[m.group(1)]


def _struct_dtype(name, body):
    """numpy structured dtype of a descriptor struct, laid out as the C compiler lays it out"""
    names, formats = [], []
    for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
        ptr = re.fullmatch(r"(?:const )?\w+ \*(\w+)", decl)
        val = re.fullmatch(r"(int|long long) (\w+(?:, \w+)*)", decl)
        if ptr is None and val is None:
            raise RuntimeError(f"azhip.h: struct {name}: unknown member '{decl}'")
        members = [ptr.group(1)] if ptr else val.group(2).split(", ")
        names += members
        formats += ["u8" if ptr else _FIELDS[val.group(1)]] * len(members)
    return np.dtype({"names": names, "formats": formats}, align=True)


def _constant(name, expr, known):
    """value of an integer #define: a literal, a parenthesised negative, or a product of literals and earlier constants"""
    expr = expr.strip()
    if expr.startswith("(") and expr.endswith(")"):
        expr = expr[1:-1]
    value = 1
    for term in (t.strip() for t in expr.split("*")):
        if re.fullmatch(r"-?\d+", term):
            value *= int(term)
        elif term in known:
            value *= known[term]
        else:
            raise RuntimeError(f"azhip.h: #define {name}: '{term}' is neither an integer nor an earlier AZ_* constant")
    return value


def parse_header(text):
    """(argtypes, non-int restypes, constants, struct dtypes) of the header `text`; RuntimeError for anything in it that
    is not a comment, a known directive, an integer `#define AZ_*`, a struct of pointers / int / long long, or a prototype
    `type az_name(args);` -- nothing is skipped"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    const, lines = {}, []
    for line in text.split("\n"):
        m = re.fullmatch(r"\s*#\s*define\s+(AZ_\w+)\s+(.*)", line)
        if m is not None:
            const[m.group(1)] = _constant(m.group(1), m.group(2), const)
        elif not line.lstrip().startswith("#"):
            lines.append(line)
        elif _DIRECTIVES.fullmatch(line.strip()) is None:  # (a conditional could hide a declaration from the compiler)
            raise RuntimeError(f"azhip.h: directive '{line.strip()}' is not understood")
    text = "\n".join(lines)
    structs = {}
    for m in _STRUCT.finditer(text):
        if m.group(1) != m.group(3):
            raise RuntimeError(f"azhip.h: struct {m.group(1)} is typedef'd as {m.group(3)}")
        structs[m.group(1)] = _struct_dtype(m.group(1), m.group(2))
    text = _STRUCT.sub(" ", text)
    sigs, restype = {}, {}
    for ret, name, args in _PROTO.findall(text):
        if name in sigs:
            raise RuntimeError(f"azhip.h: {name} is declared twice")
        args = [] if args.strip() in ("", "void") else args.split(",")
        sigs[name] = [_ctype(a, name) for a in args]
        res = _ctype(ret, f"return type of {name}")
        if res is not _INT:
            restype[name] = res
    calls = len(_CALL.findall(text))
    rest = _PROTO.sub(" ", text).replace('extern "C" {', " ").replace("}", " ").strip()
    if calls != len(sigs) or rest:
        raise RuntimeError(f"azhip.h: {calls} az_*( occurrences but {len(sigs)} prototypes parsed; not understood: '{rest[:200]}'")
    return sigs, restype, const, structs


# include/azhip.h is the only statement of the ABI: argtypes per function (return type is int unless listed in
# _RESTYPE), the integer AZ_* constants, and the descriptor structs as numpy dtypes, all read from it once, here
with open(HEADER) as _f:
    _SIGS, _RESTYPE, CONST, _STRUCTS = parse_header(_f.read())
PACK_DESC, UNPACK_DESC, ABSMAX_DESC = _STRUCTS["AzPackDesc"], _STRUCTS["AzUnpackDesc"], _STRUCTS["AzAbsmaxDesc"]
ADAM_DESC = _STRUCTS["AzAdamDesc"]
MS_LOSS_DESC = _STRUCTS["AzMsLossDesc"]


def declared_symbols():
    """Every function name include/azhip.h declares."""
    return sorted(_SIGS)


def expected_abi_version():
    """AZ_ABI_VERSION of include/azhip.h: the signatures _SIGS holds"""
    return CONST["AZ_ABI_VERSION"]


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python -m activezero_amd.build` "
                "(there is no non-HIP fallback)")
        handle = _C.CDLL(LIB_PATH)
        # a stale build (or a stale variant picked up through AZ_LIB_PATH) would read shifted arguments: refuse it
        handle.az_abi_version.argtypes, handle.az_abi_version.restype = [], _INT
        have, want = handle.az_abi_version(), expected_abi_version()
        if have != want:
            raise RuntimeError(f"{LIB_PATH} has ABI version {have}, include/azhip.h declares {want}: rebuild it "
                               "(`python -m activezero_amd.build --force`)")
        for name, args in _SIGS.items():
            fn = getattr(handle, name)
            fn.argtypes = args
            fn.restype = _RESTYPE.get(name, _INT)
        _lib = handle
    return _lib


def check(code, what):
    if code != 0:
        raise RuntimeError(f"{what} failed: {lib().az_strerror(code).decode()} ({code})")
