"""CPU-side checks of the drop-in boundary: libcdetr_hip.so builds for gfx950, loads, and exports every function that
include/cdetr_hip.h declares; the ctypes structs mirror the header's field order; no compute is launched."""
import ctypes
import os
import re

import pytest

import abi_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def libpath():
    from counting_detr_amd.build import build_lib
    return build_lib(verbose=False)


def header_functions():
    src = open(os.path.join(ROOT, "include", "cdetr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"^\s*(?:int|size_t|const char\*)\s+(cdetr_\w+)\s*\(", src, flags=re.M)
    return sorted(set(names))


def test_exports_every_declared_symbol(libpath):
    L = ctypes.CDLL(libpath)
    names = header_functions()
    assert len(names) >= 10, names
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/cdetr_hip.h but not exported"
    L.cdetr_abi_version.restype = ctypes.c_int
    assert L.cdetr_abi_version() == 2


def test_ffi_export_list_matches_header(libpath):
    from counting_detr_amd import _ffi
    assert sorted(_ffi.EXPORTS) == header_functions()


def test_struct_fields_match_header():
    """Every ctypes.Structure of _ffi names the fields of its header struct, in the header's order."""
    from counting_detr_amd import _ffi
    twins = [c for c in vars(_ffi).values() if isinstance(c, type) and issubclass(c, ctypes.Structure) and c is not ctypes.Structure]
    assert len(twins) == 13 and _ffi.ConvGeom in twins and _ffi.EmitPseudoLabelsDesc in twins
    assert abi_header.header_name(_ffi.RcdaFwdDesc) == "cdetr_rcda_fwd_desc" and abi_header.header_name(_ffi.MirrorItem) == "cdetr_mirror_item"
    for cls in twins:
        assert abi_header.field_names(abi_header.header_name(cls)) == [f[0] for f in cls._fields_], cls.__name__


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
