"""CPU: include/azhip.h is the only statement of the C ABI, and activezero_amd/_lib.py reads it.  A C++ compiler's view of
the header (prototypes through decltype, struct layouts, macro values) must equal the parser's; the descriptor tables that
packing.py and overlap.py fill by field name must hold the bytes of the structs; and the parser must refuse what it does
not understand instead of skipping it."""
import ctypes
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from activezero_amd import _lib, overlap, packing

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = {ctypes.c_int: "i", ctypes.c_longlong: "q", ctypes.c_float: "f", ctypes.c_double: "d", ctypes.c_size_t: "z",
         ctypes.c_char_p: "s", ctypes.c_void_p: "p"}
STRUCTS = {"AzPackDesc": _lib.PACK_DESC, "AzUnpackDesc": _lib.UNPACK_DESC, "AzAbsmaxDesc": _lib.ABSMAX_DESC}

PROGRAM_HEAD = r"""
#include <cstddef>
#include <cstdio>
#include <type_traits>
#include "azhip.h"
template <class T> constexpr char code() {
    if constexpr (std::is_same_v<T, int>) return 'i';
    else if constexpr (std::is_same_v<T, long long>) return 'q';
    else if constexpr (std::is_same_v<T, float>) return 'f';
    else if constexpr (std::is_same_v<T, double>) return 'd';
    else if constexpr (std::is_same_v<T, size_t>) return 'z';
    else if constexpr (std::is_same_v<T, const char *>) return 's';
    else {
        static_assert(std::is_pointer_v<T>, "azhip.h uses a type this test has no letter for");
        return 'p';
    }
}
template <class R, class... A> void sig(const char *name, R (*)(A...)) {
    const char args[] = {code<A>()..., 0};
    std::printf("fn %s %c(%s)\n", name, code<R>(), args);
}
int main() {
"""


@pytest.fixture(scope="module")
def compiler_view(tmp_path_factory):
    """what g++ makes of the header: {line kind: {name: value}}; only decltype / sizeof / offsetof, so nothing is linked"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the image is expected to have it")
    lines = [f'    sig("{n}", static_cast<decltype(&{n})>(nullptr));' for n in _lib.declared_symbols()]
    for sname, dtype in STRUCTS.items():
        lines.append(f'    std::printf("sizeof {sname} %zu\\n", sizeof({sname}));')
        for f in dtype.names:
            lines.append(f'    std::printf("field {sname}.{f} %zu+%zu\\n", offsetof({sname}, {f}), sizeof((({sname} *)0)->{f}));')
    macros = re.findall(r"#\s*define\s+(AZ_\w+)", open(_lib.HEADER).read())  # (found without the parser)
    lines += [f'    std::printf("const {m} %lld\\n", (long long)({m}));' for m in macros]
    tmp = tmp_path_factory.mktemp("cabi")
    src, exe = tmp / "abi_view.cpp", tmp / "abi_view"
    src.write_text(PROGRAM_HEAD + "\n".join(lines) + "\n    return 0;\n}\n")
    build = subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr[-2000:]
    view = {"fn": {}, "sizeof": {}, "field": {}, "const": {}}
    for line in run.stdout.splitlines():
        kind, name, value = line.split(" ")
        view[kind][name] = value
    return view


def test_prototypes_are_what_the_compiler_deduces(compiler_view):
    mine = {name: CODES[_lib._RESTYPE.get(name, ctypes.c_int)] + "(" + "".join(CODES[t] for t in args) + ")"
            for name, args in _lib._SIGS.items()}
    assert len(mine) >= 114
    assert set(_lib._RESTYPE) <= set(_lib._SIGS) and ctypes.c_int not in _lib._RESTYPE.values()
    assert compiler_view["fn"] == mine


def test_struct_layouts_and_constants_are_what_the_compiler_sees(compiler_view):
    assert _lib.PACK_DESC.itemsize == 72 and _lib.UNPACK_DESC.itemsize == 40  # what the Python side used to hard-code
    for sname, dtype in STRUCTS.items():
        assert int(compiler_view["sizeof"][sname]) == dtype.itemsize
        end = 0
        for f in dtype.names:
            sub, offset = dtype.fields[f][:2]
            assert compiler_view["field"][f"{sname}.{f}"] == f"{offset}+{sub.itemsize}", f
            assert offset == end, f"{sname}: a member the parser does not know lies before {f}"
            end = offset + sub.itemsize
        assert end == dtype.itemsize
    assert {k: int(v) for k, v in compiler_view["const"].items()} == _lib.CONST
    assert _lib.CONST["AZ_ABI_VERSION"] == 6 and _lib.CONST["AZ_AMAX_FLOATS"] == 1024
    assert [_lib.CONST[k] for k in ("AZ_OK", "AZ_EINVAL", "AZ_ENULL", "AZ_ELAUNCH", "AZ_EUNSUPPORTED", "AZ_EWORKSPACE")] == \
        [0, -1, -2, -3, -4, -5]


def test_modules_take_their_constants_from_the_header():
    from activezero_amd import amax
    assert amax.AMAX_SLOTS == _lib.CONST["AZ_AMAX_FLOATS"] == _lib.CONST["AZ_AMAX_SLOTS"] * _lib.CONST["AZ_AMAX_STRIDE"]
    assert (packing.PACK_2D_SAME, packing.PACK_2D_ROLL, packing.PACK_3D_GATHER, packing.PACK_3D_ROLL,
            packing.PACK_3D_ROLL2) == (0, 1, 2, 3, 4)


def _block_tables(work):
    """block_desc, first_block, nblocks by the loop the table builders used before they shared launch_tables"""
    block_desc, first, nblocks = [], [], 0
    for i, n in enumerate(work):
        nb = (n + 255) // 256
        first.append(nblocks)
        block_desc += [i] * nb
        nblocks += nb
    return block_desc, first, nblocks


def test_pack_table_bytes_are_the_struct_in_header_order():
    fields = ("dst", "src", "amax", "s_co", "s_ci", "kind", "cin", "cout", "ci_real", "co_real", "taps", "flip")
    rows = [(0x7F0000001000, 0x7F0000002040, 0x7F0000003080, 64 * 27, 27, 3, 64, 32, 61, 29, 27, 1),
            (0xFFFF000011110000, 0x7E0000005000, 0x7E0000006000, -5, 1 << 40, 0, 48, 96, 40, 12, 1, 0),
            (0x10, 0x20, 0x30, 9, 64 * 9, 1, 32, 64, 31, 63, 9, True)]
    descs, block_desc, first, nblocks = packing.pack_tables([dict(zip(fields, r)) for r in rows])
    assert descs.view(np.uint8).tobytes() == b"".join(struct.pack("<QQQqq8i", *r, 0) for r in rows)
    want = _block_tables([2 * r[10] * r[6] * r[7] for r in rows])  # two fp16 parts of taps * cin * cout weights
    assert (block_desc.tolist(), first.tolist(), nblocks) == want
    assert block_desc.dtype == first.dtype == np.int32 and nblocks == 432 + 36 + 144
    with pytest.raises(KeyError):  # a row that lacks a field of the struct is an error, not a zero
        packing.pack_tables([dict(zip(fields[:-1], rows[0]))])


def test_unpack_table_bytes_are_the_struct_in_header_order():
    fields = ("dst", "ws", "cm", "cn", "cm_real", "cn_real", "taps")
    rows = [(0x7F0000001000, 0xFFFF000022220000, 64, 32, 61, 29, 27), (0x40, 0x80, 96, 48, 3, 5, 9)]
    descs, block_desc, first, nblocks = overlap.unpack_tables([dict(zip(fields, r)) for r in rows])
    assert descs.view(np.uint8).tobytes() == b"".join(struct.pack("<QQ6i", *r, 0) for r in rows)
    want = _block_tables([r[4] * r[5] * r[6] for r in rows])  # one element per real weight
    assert (block_desc.tolist(), first.tolist(), nblocks) == want and nblocks == 187 + 1
    # Sink._flush_pending uploads the three tables as one int32 array and offsets into it by ints per descriptor
    assert descs.view(np.int32).size == len(rows) * (_lib.UNPACK_DESC.itemsize // 4) == len(rows) * 10
    assert np.concatenate([descs.view(np.int32), block_desc, first]).dtype == np.int32


MINI = "#define AZ_OK 0\n#define AZ_EINVAL (-1)\n#define AZ_N 4\n#define AZ_NN (AZ_N * AZ_N * 2)\nint az_a(int x, long long y);\n"


def test_parser_reads_a_prototype_split_over_three_lines():
    sigs, restype, const, structs = _lib.parse_header(
        MINI + "long long az_b(const float *p, /* a comment, with a comma */\n        const char *name,\n"
               "        size_t n);\ntypedef struct S {\n    void *p;\n    long long a, b;\n    int k;\n} S;\n")
    assert sigs == {"az_a": [ctypes.c_int, ctypes.c_longlong], "az_b": [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]}
    assert restype == {"az_b": ctypes.c_longlong}
    assert const == {"AZ_OK": 0, "AZ_EINVAL": -1, "AZ_N": 4, "AZ_NN": 32}
    assert structs["S"].itemsize == 32 and structs["S"].fields["k"][1] == 24  # (padded to the pointer's alignment)


@pytest.mark.parametrize("extra, names", [
    ("int az_b(unsigned n);\n", "az_b.*unsigned n"),                            # a parameter type with no ctypes mapping
    ("short az_b(int n);\n", "az_b.*short"),                                    # ... and a return type
    ("#if AZ_N > 2\nint az_b(int n);\n#endif\n", "#if AZ_N > 2"),               # a declaration the compiler may not see
    ("AZ_EXPORT(int) az_b(int n);\n", "az_b"),                                  # a declaration behind a macro
    ("static inline int az_b(int n) { return n; }\n", "az_b"),                  # a definition
    ("int az_b(int (*callback)(int));\n", "az_b"),                              # a shape of parameter list it cannot split
    ("#define AZ_HALF 0.5\n", "AZ_HALF"),                                       # a constant that is no integer
    ("typedef struct S {\n    float x;\n} S;\n", "struct S.*float x"),          # a struct member with no dtype mapping
    ("int az_a(int x, long long y);\n", "az_a.*twice"),
])
def test_parser_refuses_what_it_does_not_understand(extra, names):
    with pytest.raises(RuntimeError, match=names):
        _lib.parse_header(MINI + extra)


def test_a_prototype_that_lost_its_semicolon_trips_the_count():
    text = open(_lib.HEADER).read()
    assert _lib.parse_header(text)[0] == _lib._SIGS
    broken = text.replace("int az_option(const char *name);", "int az_option(const char *name)")
    assert broken != text
    with pytest.raises(RuntimeError, match=r"\d+ az_\*\( occurrences but \d+ prototypes") as err:
        _lib.parse_header(broken)
    occurrences, parsed = map(int, re.findall(r"\d+", str(err.value))[:2])
    assert occurrences == len(_lib._SIGS) and parsed < occurrences
