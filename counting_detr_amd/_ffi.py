"""ctypes binding of libcdetr_hip.so, DERIVED from include/cdetr_hip.h at import: the header is the one statement of the ABI.  No torch types
cross the boundary: raw device pointers (tensor.data_ptr()), sizes and the current hipStream_t.

What the reader below understands -- the subset of C the header is written in:
  - `#define CDETR_<NAME> <integer literal | CDETR_<OTHER>>`            -> DEFINES["<NAME>"] (anything else, the include guard too, is skipped);
  - `typedef struct { ... } cdetr_x_y;`                                 -> a ctypes.Structure `XY`, a module attribute, in header order;
  - `int | const char* cdetr_name(<parameters> | void);`                -> EXPORTS, and restype / argtypes in lib();
  - fields and parameters: `[const] T name`, `[const] T* name`, several names after one T; T one of _SCALARS or, by value, an earlier struct;
    every pointer, struct pointers included, is a c_void_p (C.byref(desc) is passed); `static inline` helpers are not part of the ABI.
No arrays, unions, bit-fields, enums or function pointers: a declaration outside the subset raises at import, naming itself -- whoever needs
one extends this reader and the compiler-checked layout test (tests/test_abi.py) together.

The product path has NO fallback: if the library is missing or a call fails, a RuntimeError is raised.
"""
import ctypes as C
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CDETR_LIB") or os.path.join(_HERE, "lib", "libcdetr_hip.so")      # CDETR_LIB: experiment builds (tools/)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "cdetr_hip.h")

_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint8_t": C.c_uint8, "float": C.c_float, "double": C.c_double}
_DECL = re.compile(r"(?:const\s+)?(\w+)\b\s*(.*)", re.S)      # base type, then the declarators `* a`, `a, b`
DEFINES, EXPORTS, _STRUCTS, _PROTOS = {}, [], {}, []          # _PROTOS: (name, restype, argtypes) per prototype


def _ctypes_of(decl, where):
    """`const float* A` / `int32_t Ha, Wa` / `cdetr_conv_geom g` -> [(name, ctype)]."""
    base, rest = _DECL.fullmatch(decl.strip()).groups()
    out = []
    for d in rest.split(","):
        m = re.fullmatch(r"\s*(\*?)\s*(\w+)\s*", d)
        if m is None or (not m.group(1) and base not in _SCALARS and base not in _STRUCTS):
            raise RuntimeError(f"{HEADER_PATH}: `{decl.strip()}` in {where} is outside the subset counting_detr_amd/_ffi.py reads")
        out.append((m.group(2), C.c_void_p if m.group(1) else _SCALARS.get(base) or _STRUCTS[base]))
    return out


def _read_header():
    if not os.path.exists(HEADER_PATH):
        raise RuntimeError(f"{HEADER_PATH} is missing: the binding of libcdetr_hip.so is derived from it")
    src = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(HEADER_PATH).read(), flags=re.S)
    raw = dict(re.findall(r"^[ \t]*#define[ \t]+CDETR_(\w+)[ \t]+(\w+)[ \t]*$", src, flags=re.M))
    for name, v in raw.items():
        for _ in raw:                                       # a define may name another
            v = raw.get(v[len("CDETR_"):], v) if v.startswith("CDETR_") else v
        if re.fullmatch(r"\d+|0[xX][0-9a-fA-F]+", v):
            DEFINES[name] = int(v, 0)
    for body, name in re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", src, flags=re.S):
        fields = [f for decl in body.split(";") if decl.strip() for f in _ctypes_of(decl, name)]
        camel = "".join(w.capitalize() for w in name[len("cdetr_"):].split("_"))
        _STRUCTS[name] = globals()[camel] = type(camel, (C.Structure,), {"_fields_": fields})
    for ret, name, params in re.findall(r"^[ \t]*([\w \t\*]+?)[ \t]*\b(cdetr_\w+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        ret = re.sub(r"\s+", "", ret)
        if ret not in ("int", "constchar*"):
            raise RuntimeError(f"{HEADER_PATH}: return type of {name} is outside the subset counting_detr_amd/_ffi.py reads")
        args = [] if params.strip() in ("", "void") else [_ctypes_of(p, name)[0][1] for p in params.split(",")]
        EXPORTS.append(name)
        _PROTOS.append((name, C.c_int if ret == "int" else C.c_char_p, args))
    declared = re.findall(r"^(?!\s*static\b)[^\n(]*\b(cdetr_\w+)\s*\(", src, flags=re.M)
    if declared != EXPORTS:
        raise RuntimeError(f"{HEADER_PATH}: the declaration of {sorted(set(declared) ^ set(EXPORTS))} is outside the subset counting_detr_amd/_ffi.py reads")


_read_header()
ROWS_DENSE, ROWS_CONV_FWD, ROWS_CONV_DGRAD = DEFINES["ROWS_DENSE"], DEFINES["ROWS_CONV_FWD"], DEFINES["ROWS_CONV_DGRAD"]
_lib = None


def lib():
    """Load (once) and return the library; raises if it is missing -- there is no CPU/eager fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -m counting_detr_amd.build` "
                               "(the Counting-DETR MI355X path has no fallback implementation)")
        L = C.CDLL(LIB_PATH)
        for name, restype, argtypes in _PROTOS:
            fn = getattr(L, name, None)
            if fn is None:
                raise RuntimeError(f"{LIB_PATH} does not export {name}, which include/cdetr_hip.h declares: rebuild it with "
                                   "`python -m counting_detr_amd.build`")
            fn.restype, fn.argtypes = restype, argtypes
        if L.cdetr_abi_version() != DEFINES["ABI_VERSION"]:
            raise RuntimeError("libcdetr_hip.so ABI version mismatch")
        _lib = L
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().cdetr_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed (rc={rc}): {msg}")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_ptr():
    """hipStream_t of torch's current stream on the current device.  The raw accessor costs ~0.3 us; torch.cuda.current_stream()
    builds a Stream object and resolves the device index in Python (~9 us, i.e. ~6 ms of host time over the ~700 launches of a step)."""
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device pointer of a tensor (None -> NULL).  The product path only ever runs on the GPU."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("counting_detr_amd kernels need device tensors (no CPU fallback exists)")
    return t.data_ptr()
