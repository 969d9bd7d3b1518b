"""CPU: the C-ABI shared library loads and exports every symbol include/vneti.h declares."""
import ctypes
import os
import shutil
import subprocess

import pytest

from view_neti_amd import lib


@pytest.mark.parametrize("precision,code", [("fp16", 0), ("bf16", 1)])
def test_header_symbols_exported(precision, code):
    """both builds of the library (fp16: libvneti_hip.so, bf16: libvneti_hip_bf16.so, the same sources with -DVN_BF16)"""
    path = lib.so_path(precision)
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    so = ctypes.CDLL(path)
    names = lib.declared_symbols()
    assert len(names) >= 15
    missing = [n for n in names if not hasattr(so, n)]
    assert not missing, f"declared in vneti.h but not exported: {missing}"
    assert so.vneti_version() == 1 and so.vneti_precision() == code


def test_one_precision_per_process():
    lib.load()
    with pytest.raises(RuntimeError):
        lib.set_precision("bf16" if lib.precision() == "fp16" else "fp16")
    lib.set_precision(lib.precision())  # re-stating the loaded one is fine


def test_error_convention_no_gpu():
    """argument validation happens before any HIP call, so it is testable without a GPU."""
    l = lib.load()
    d = lib.GemmDesc()
    rc = l.vneti_gemm_f16(ctypes.byref(d), None)
    assert rc < 0
    assert "null" in lib.last_error().lower()
    with pytest.raises(RuntimeError):
        lib.check(rc, "gemm")


def test_signatures_cover_header():
    """every function the header declares is bound after load(): argtypes and restype derived from its prototype"""
    so = lib.load()
    names = lib.declared_symbols()
    assert set(names) == {"vneti_" + k for k in lib.SIGNATURES}
    for n in names:
        fn = getattr(so, n)
        assert fn.argtypes is not None and list(fn.argtypes) == lib.SIGNATURES[n[len("vneti_"):]], n
        assert fn.restype in (ctypes.c_int, ctypes.c_longlong), n
    for k in lib.VALUE_FUNCS:
        assert k in lib.SIGNATURES
    assert so.vneti_groupnorm_ws_floats.restype is ctypes.c_longlong and so.vneti_gemm_f16.restype is ctypes.c_int
    assert so.vneti_gemm_f16.argtypes[0] is ctypes.POINTER(lib.GemmDesc)
    assert so.vneti_transpose_f16_multi.argtypes[0] is ctypes.POINTER(lib.TransposeDesc)
    with pytest.raises(KeyError):
        lib.query("gemm_f16")  # a status-returning entry goes through call(), which checks it


def test_struct_layout_matches_compiler(tmp_path):
    """sizeof / offsetof of every field of every struct of the header, as the C++ compiler lays them out, against the
    generated ctypes classes; the program's field list comes from the parsed header, so a new field is covered as is"""
    structs, _ = lib.parse_header(open(lib.HEADER_PATH).read())
    assert structs["vneti_gemm_desc"]._fields_ == lib.GemmDesc._fields_ and len(lib.GemmDesc._fields_) >= 50
    assert structs["vneti_transpose_desc"]._fields_ == lib.TransposeDesc._fields_
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "vneti.h"', "int main() {"]
    for name, cls in structs.items():
        lines.append(f'  std::printf("{name} sizeof %zu\\n", sizeof({name}));')
        for f, _ in cls._fields_:
            lines.append(f'  std::printf("{name} {f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    cxx = next((c for c in ("c++", "g++", "clang++", "hipcc") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler (c++, g++, clang++ or hipcc) on PATH"
    subprocess.run([cxx, "-I", os.path.dirname(lib.HEADER_PATH), str(src), "-o", str(exe)], check=True)  # host only
    want = {}
    for name, cls in structs.items():
        want[(name, "sizeof")] = (ctypes.sizeof(cls),)
        for f, _ in cls._fields_:
            want[(name, f)] = (getattr(cls, f).offset, getattr(cls, f).size)
    got = {}
    for row in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n"):
        if row:
            name, f, *nums = row.split()
            got[(name, f)] = tuple(int(x) for x in nums)
    assert got == want


_MINI = """
/* a comment with int vneti_not_a_function(int x); inside */
#define VNETI_SOMETHING 1
typedef struct vneti_mini_desc {
  const void* p;   /* pointer */
  long long ld, stride;
  int rows, cols;
  float alpha;
} vneti_mini_desc;
int vneti_mini(const vneti_mini_desc* d, const float* x, unsigned* mask, void** out, char* buf, size_t n,
               uint32_t seed, unsigned int id, void* stream);
long long vneti_mini_floats(int rows, int cols);
int vneti_none(void);
"""


def test_parser_type_rule_and_negatives():
    c = ctypes
    structs, protos = lib.parse_header(_MINI)
    d = structs["vneti_mini_desc"]
    assert d._fields_ == [("p", c.c_void_p), ("ld", c.c_longlong), ("stride", c.c_longlong), ("rows", c.c_int),
                          ("cols", c.c_int), ("alpha", c.c_float)]
    assert protos == {
        "vneti_mini": (c.c_int, [c.POINTER(d), c.c_void_p, c.c_void_p, c.c_void_p, c.c_char_p, c.c_size_t, c.c_uint,
                                 c.c_uint, c.c_void_p]),
        "vneti_mini_floats": (c.c_longlong, [c.c_int, c.c_int]),
        "vneti_none": (c.c_int, [])}
    # a parameter added to a prototype changes the derived arity
    _, more = lib.parse_header(_MINI.replace("(int rows, int cols)", "(int rows, int cols, long long ld)"))
    assert more["vneti_mini_floats"] == (c.c_longlong, [c.c_int, c.c_int, c.c_longlong])
    # unknown types raise and name the line, by value and behind a pointer, in a prototype and in a struct
    for bad in (_MINI.replace("uint32_t seed", "uint16_t seed"), _MINI.replace("unsigned* mask", "half* mask"),
                _MINI.replace("float alpha;", "double alpha;")):
        line = 1 + next(i for i, (a, b) in enumerate(zip(_MINI.split("\n"), bad.split("\n"))) if a != b)
        with pytest.raises(ValueError, match=rf"line {line}\b"):
            lib.parse_header(bad)
    # what is not a struct or an `int|long long vneti_*(...)` prototype raises as well: no statement is skipped
    for bad in (_MINI + "float vneti_ratio(int a);\n", _MINI + "int other_name(int a);\n",
                _MINI.replace("int rows, cols;", "int rows, *cols;"), _MINI.replace("int rows, cols;", "int rows, in;"),
                _MINI.replace("int rows, int cols", "int rows, int")):
        with pytest.raises(ValueError, match="line"):
            lib.parse_header(bad)
