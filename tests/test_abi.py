"""CPU-side checks of the drop-in boundary: libcdetr_hip.so builds for gfx950, loads, and exports every function that
include/cdetr_hip.h declares; the binding _ffi derives from the header is held to the header as the tests' own reader (abi_header) and
the C compiler see it: field names, struct layouts, every signature; no compute is launched."""
import ctypes
import os
import re
import subprocess

import pytest

import abi_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def libpath():
    from counting_detr_amd.build import build_lib
    return build_lib(verbose=False)


# how the tests spell a C type of the header as a ctypes type: written out here, not taken from _ffi
CTYPE = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint8_t": ctypes.c_uint8, "float": ctypes.c_float,
         "double": ctypes.c_double}
RESTYPE = {"int": ctypes.c_int, "const char*": ctypes.c_char_p}


def twins(_ffi):
    return [c for c in vars(_ffi).values() if isinstance(c, type) and issubclass(c, ctypes.Structure) and c is not ctypes.Structure]


def test_exports_every_declared_symbol(libpath):
    L = ctypes.CDLL(libpath)
    names = abi_header.function_names()
    assert len(names) >= 10, names
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/cdetr_hip.h but not exported"
    L.cdetr_abi_version.restype = ctypes.c_int
    assert L.cdetr_abi_version() == 2


def test_ffi_export_list_matches_header(libpath):
    from counting_detr_amd import _ffi
    assert sorted(_ffi.EXPORTS) == abi_header.function_names()


def test_struct_fields_match_header():
    """One ctypes.Structure of _ffi per `typedef struct` of the header, each naming the fields of its header struct in the header's order,
    each field of the header's type (a pointer is a c_void_p, a struct by value its twin)."""
    from counting_detr_amd import _ffi
    tw = twins(_ffi)
    names = abi_header.struct_names()
    assert len(names) == len(set(names)) >= 10 and sorted(abi_header.header_name(c) for c in tw) == sorted(names)
    assert _ffi.ConvGeom in tw and _ffi.EmitPseudoLabelsDesc in tw and _ffi.NmsSuppressDesc in tw
    by_name = {abi_header.header_name(c): c for c in tw}
    assert abi_header.header_name(_ffi.RcdaFwdDesc) == "cdetr_rcda_fwd_desc" and abi_header.header_name(_ffi.MirrorItem) == "cdetr_mirror_item"
    for cls in tw:
        assert abi_header.field_names(abi_header.header_name(cls)) == [f[0] for f in cls._fields_], cls.__name__
        for (name, base, pointer), (_, ctype) in zip(abi_header.struct_fields(abi_header.header_name(cls)), cls._fields_):
            assert ctype is (ctypes.c_void_p if pointer else CTYPE.get(base) or by_name[base]), (cls.__name__, name)


def test_struct_layouts_match_the_compiler(tmp_path):
    """sizeof of every struct and offsetof of every field, as gcc lays out the real header, against ctypes.sizeof and the field offsets of
    the twin: a field bound with the wrong width, or a missed padding rule, moves a number."""
    from counting_detr_amd import _ffi
    structs = [(s, abi_header.field_names(s)) for s in abi_header.struct_names()]
    lines = ['#include <stdio.h>', '#include "cdetr_hip.h"', 'int main(void) {']
    for s, fields in structs:
        lines.append(f'    printf("{s} %zu\\n", sizeof({s}));')
        lines += [f'    printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for f in fields]
    (tmp_path / "layout.c").write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")])
    got = dict(line.split() for line in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())
    by_name = {abi_header.header_name(c): c for c in twins(_ffi)}
    want = {}
    for s, fields in structs:
        want[s] = str(ctypes.sizeof(by_name[s]))
        want.update({f"{s}.{f}": str(getattr(by_name[s], f).offset) for f in fields})
    assert len(want) == sum(1 + len(f) for _, f in structs) and got == want


def test_signatures_match_header(libpath):
    """restype and argtypes of every bound function against the prototype as abi_header reads it: pointers are c_void_p, scalars their
    fixed-width ctypes; the bound names are the header's, once each."""
    from counting_detr_amd import _ffi
    L = _ffi.lib()
    protos = abi_header.prototypes()
    assert len(protos) >= 10 and len(_ffi.EXPORTS) == len(set(_ffi.EXPORTS)) == len(protos) and set(_ffi.EXPORTS) == {p[0] for p in protos}
    for name, ret, args in protos:
        fn = getattr(L, name)
        assert fn.restype is RESTYPE[ret], name
        assert list(fn.argtypes) == [ctypes.c_void_p if pointer else CTYPE[base] for base, pointer in args], name


def test_error_reporting_without_gpu(libpath):
    """Argument validation happens before any launch: a bad descriptor returns <0 and sets cdetr_last_error()."""
    from counting_detr_amd import _ffi
    L = _ffi.lib()
    d = _ffi.GemmDesc()
    rc = L.cdetr_gemm(ctypes.byref(d), None)
    assert rc < 0 and b"cdetr_gemm" in L.cdetr_last_error()


def test_product_path_refuses_cpu_tensors(libpath):
    import torch
    from counting_detr_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.linear_fwd(torch.zeros(4, 8), torch.zeros(2, 8))


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "counting_detr_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            assert not re.search(r"^\s*(from|import)\s+oracle", open(os.path.join(pkg, fn)).read(), flags=re.M), fn


def test_zero_arena_host_logic():
    """ops.ZeroArena (the backward's zeroed accumulators as slices of one engine-owned buffer): a measuring pass serves torch.zeros and
    records the high-water mark of one backward; the serving pass hands out aligned, disjoint slices in the same order and refuses to
    alias when a backward asks for more than was measured."""
    import torch
    from counting_detr_amd import ops
    a = ops.ZeroArena()
    with ops.scope(ZERO_ARENA=a):
        for _ in range(2):                       # two backwards of the same shape: the need is a maximum, not a sum
            a.reset()
            t1, t2 = ops.zeros_flat(100, "cpu"), ops.zeros_flat(7, "cpu")
            assert t1.numel() == 100 and t2.numel() == 7 and float(t1.abs().sum() + t2.abs().sum()) == 0.0
    assert a.need == 128 + 64 and ops.ZERO_ARENA is None
    a.buf = torch.zeros(a.need)
    with ops.scope(ZERO_ARENA=a):
        a.reset()
        s1, s2 = ops.zeros_flat(100, "cpu"), ops.zeros_flat(7, "cpu")
        assert s1.data_ptr() == a.buf.data_ptr() and s2.data_ptr() == a.buf.data_ptr() + 128 * 4
        s1.fill_(1.0)
        assert float(s2.sum()) == 0.0            # disjoint
        with pytest.raises(RuntimeError):
            ops.zeros_flat(1, "cpu")
    assert ops.zeros_flat(5, "cpu").numel() == 5   # outside any engine: a plain fill
