"""ctypes binding of libvneti_hip.so, derived from the C ABI declared in include/vneti.h: the header is parsed once at
import into the argument structs and the signature of every entry point; nothing here restates it by hand.

The product path has NO fallback: if the shared library is missing or a call fails, a
RuntimeError is raised.  `load()` never builds implicitly on a machine without hipcc; use
`__graft_entry__.build()` / `python view_neti_amd/csrc/build.py` to compile.
"""
from __future__ import annotations

import ctypes as C
import keyword
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "vneti.h")

# One precision per process: "fp16" (libvneti_hip.so) or "bf16" (libvneti_hip_bf16.so, the same sources built with
# -DVN_BF16) — the reference's optim.mixed_precision branches fp16 / bf16 (training/coach.py:792-802).  Chosen before the
# first call into the library (set_precision, or VNETI_PRECISION in the environment); every 16-bit buffer of the engines
# is allocated as act_dtype().
_PRECISIONS = {"fp16": ("libvneti_hip.so", 0), "bf16": ("libvneti_hip_bf16.so", 1)}
_precision = os.environ.get("VNETI_PRECISION", "fp16")
if _precision not in _PRECISIONS:
    raise RuntimeError(f"VNETI_PRECISION={_precision!r}: expected one of {sorted(_PRECISIONS)}")

_lib = None


def so_path(precision: str = None) -> str:
    # VNETI_LIB_PATH: kernel-development aid (A/B a lab build of the same ABI); the product path is the in-tree library
    return os.environ.get("VNETI_LIB_PATH") or os.path.join(_HERE, "csrc", _PRECISIONS[precision or _precision][0])


SO_PATH = so_path()


def precision() -> str:
    return _precision


def set_precision(p: str) -> None:
    """select the library build; only before the first call into it (a process computes in ONE 16-bit format)"""
    global _precision, SO_PATH
    if p not in _PRECISIONS:
        raise ValueError(f"precision {p!r}: expected one of {sorted(_PRECISIONS)}")
    if _lib is not None and p != _precision:
        raise RuntimeError(f"libvneti is already loaded in {_precision}; {p} needs its own process")
    _precision = p
    SO_PATH = so_path()


def act_dtype():
    """torch dtype of the 16-bit activations / packed weights the loaded library computes in"""
    import torch
    return torch.bfloat16 if _precision == "bf16" else torch.float16


_SCALARS = {"int": C.c_int, "long long": C.c_longlong, "float": C.c_float, "unsigned": C.c_uint, "unsigned int": C.c_uint,
            "uint32_t": C.c_uint, "size_t": C.c_size_t}


def _ctype(ctype: str, structs: dict, where: str):
    """THE type rule of the binding: a scalar by _SCALARS, `char*` -> c_char_p, a pointer to a struct of the header ->
    POINTER(its Structure), every other pointer (void*, const float*, unsigned*, void**, ...) -> c_void_p, which takes
    data_ptr() ints, None, ctypes arrays and byref(...).  Anything else raises: there is no default."""
    words = [w for w in ctype.replace("*", " * ").split() if w != "const"]
    stars, base = words.count("*"), " ".join(w for w in words if w != "*")
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars == 1 and base == "char":
        return C.c_char_p
    if stars == 1 and base in structs:
        return C.POINTER(structs[base])
    if stars and (base in _SCALARS or base in ("void", "char")):
        return C.c_void_p
    raise ValueError(f"vneti.h {where}: no ctypes rule for the type {ctype.strip()!r}")


def _declarator(decl: str, where: str):
    """'const void* A' -> ('const void*', 'A')"""
    m = re.fullmatch(r"(.*[\s*])(\w+)", decl.strip(), re.S)
    if not m:
        raise ValueError(f"vneti.h {where}: cannot read the declaration {' '.join(decl.split())!r}")
    return m.group(1), m.group(2)


def parse_header(text: str):
    """The C ABI in header text -> (structs: C name -> generated ctypes.Structure, prototypes: C name -> (restype, argtypes)).
    Reads `typedef struct ... { ... } name;` and `int|long long vneti_*(...);`; any other statement raises with its line."""
    blank = lambda m: "\n" * m.group().count("\n")  # what is cut out keeps its line breaks, so positions still name lines
    text = re.sub(r"/\*.*?\*/|//[^\n]*", blank, text, flags=re.S)
    text = re.sub(r'^[ \t]*#.*$|extern\s+"C"\s*\{|^\}[ \t]*$', "", text, flags=re.M)
    at = lambda src, pos: f"line {src.count(chr(10), 0, pos) + 1}"
    structs, protos = {}, {}
    typedef = r"typedef\s+struct\s+\w*\s*\{(.*?)\}\s*(\w+)\s*;"
    for m in re.finditer(typedef, text, flags=re.S):
        fields = []
        for d in re.finditer(r"[^;\s][^;]*", m.group(1)):  # `int Hi, Wi, Ci;` declares one field per name
            where = at(text, m.start(1) + d.start())
            first, *more = d.group().split(",")
            ctype, name = _declarator(first, where)
            for n in [name] + [x.strip() for x in more]:
                if not n.isidentifier() or keyword.iskeyword(n):  # `*b`, `a[4]`, or a name python cannot spell as d.<name>
                    raise ValueError(f"vneti.h {where}: cannot bind the field {n!r}")
                fields.append((n, _ctype(ctype, structs, where)))
        structs[m.group(2)] = type(m.group(2), (C.Structure,), {"_fields_": fields})
    rest = re.sub(typedef, blank, text, flags=re.S)
    for m in re.finditer(r"[^;\s][^;]*", rest):
        p = re.fullmatch(r"(int|long long)\s+(vneti_\w+)\s*\((.*)\)\s*", m.group(), re.S)
        if not p:
            raise ValueError(f"vneti.h {at(rest, m.start())}: cannot read {' '.join(m.group().split())!r} as a prototype")
        argtypes = []
        for x in re.finditer(r"[^,\s][^,]*", "" if p.group(3).strip() == "void" else p.group(3)):
            where = at(rest, m.start() + p.start(3) + x.start())
            argtypes.append(_ctype(_declarator(x.group(), where)[0], structs, where))
        protos[p.group(2)] = (_SCALARS[p.group(1)], argtypes)
    return structs, protos


with open(HEADER_PATH) as _f:
    _STRUCTS, _PROTOS = parse_header(_f.read())
GemmDesc, TransposeDesc = _STRUCTS["vneti_gemm_desc"], _STRUCTS["vneti_transpose_desc"]
# short name -> argtypes of every declared function
SIGNATURES = {n[len("vneti_"):]: argtypes for n, (_, argtypes) in _PROTOS.items()}
# the functions whose return value is a number to use (`query`); every other one returns a status (`call`)
VALUE_FUNCS = frozenset({
    "version", "precision", "last_error", "gemm_select_tile", "gemm_select_split", "attn_dkv_qsplit", "img_resample_ksize",
    "groupnorm_ws_floats", "lpips_ws_floats", "mse_loss_per_sample_ws_floats", "mapper_num_params", "mapper_save_floats",
    "mapper_rowgrad_floats", "mapper_legacy_input_params", "grad_sumsq_ws_doubles", "cfg_rescale_ws_doubles",
    "loss_weights_from_mask_ws_ints"})
_stray = ({n[len("vneti_"):] for n, (res, _) in _PROTOS.items() if res is C.c_longlong} - VALUE_FUNCS) | (VALUE_FUNCS - set(SIGNATURES))
if _stray:
    raise RuntimeError(f"lib.VALUE_FUNCS is out of step with include/vneti.h: {sorted(_stray)}")


def declared_symbols() -> list[str]:
    """Every function name declared in include/vneti.h (used by the CPU test suite)."""
    src = open(HEADER_PATH).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(vneti_[a-z0-9_]+)\s*\(", src)))


def load():
    """Load the library once and bind every declared function (argtypes and restype from the header); raise loudly when
    the library or one of its symbols is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise RuntimeError(
            f"{os.path.basename(SO_PATH)} not found at {SO_PATH}: build it with "
            "`python view_neti_amd/csrc/build.py` (hipcc, gfx950). There is no fallback path.")
    lib = C.CDLL(SO_PATH)
    for name, (restype, argtypes) in _PROTOS.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise RuntimeError(f"{SO_PATH} does not export {name}, which include/vneti.h declares: rebuild it")
        fn.restype, fn.argtypes = restype, argtypes
    if lib.vneti_precision() != _PRECISIONS[_precision][1]:
        raise RuntimeError(f"{SO_PATH} computes in precision {lib.vneti_precision()}, the process asked for {_precision}")
    _lib = lib
    return lib


def last_error() -> str:
    lib = load()
    buf = C.create_string_buffer(512)
    lib.vneti_last_error(buf, 512)
    return buf.value.decode(errors="replace")


def check(rc: int, what: str = ""):
    if rc != 0:
        raise RuntimeError(f"vneti call failed ({what}) rc={rc}: {last_error()}")


def call(name: str, *args):
    """Call the status-returning `vneti_<name>`: pointers are data_ptr() ints / None / ctypes arrays / byref(...), scalars
    python numbers; a non-zero status raises with the library's message."""
    check(getattr(load(), "vneti_" + name)(*args), name)


def query(name: str, *args) -> int:
    """Call one of VALUE_FUNCS and return its number (a size query answers negative for an unsupported shape)."""
    if name not in VALUE_FUNCS:
        raise KeyError(f"vneti_{name} returns a status: use call()")
    return int(getattr(load(), "vneti_" + name)(*args))
