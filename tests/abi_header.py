"""include/cdetr_hip.h as the ABI tests read it: the fields of a descriptor struct in declaration order, the prototypes, and the header name of a
ctypes twin of counting_detr_amd/_ffi.py.  The tests' OWN reader: _ffi derives its binding from the same header, so nothing here may come from
the package.  Not a test module; imported by tests/test_abi.py and the per-feature CPU tests."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def source():
    return open(os.path.join(ROOT, "include", "cdetr_hip.h")).read()


def struct_body(struct_name):
    """The text between the braces of `typedef struct { ... } struct_name;`, comments included."""
    return re.search(r"typedef struct \{([^}]*)\}\s*" + struct_name + r"\s*;", source(), flags=re.S).group(1)


def struct_fields(struct_name):
    """[(field name, C base type without const, is a pointer)] in declaration order."""
    body = re.sub(r"/\*.*?\*/", "", struct_body(struct_name), flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        base = re.match(r"(?:const\s+)?(\w+)", decl).group(1)
        for i, nm in enumerate(decl.split(",")):
            out.append((re.findall(r"(\w+)\s*$", nm.strip())[0], base, "*" in (decl.split(",")[0] if i == 0 else nm)))
    return out


def struct_names():
    """Every `typedef struct { ... } name;` of the header, in declaration order."""
    return re.findall(r"typedef struct \{[^}]*\}\s*(\w+)\s*;", re.sub(r"/\*.*?\*/", "", source(), flags=re.S))


def prototypes():
    """[(function name, return type, [(C base type without const, is a pointer), ...])] in declaration order; `static inline` helpers are
    no part of the ABI and are left out."""
    src = re.sub(r"/\*.*?\*/", "", source(), flags=re.S)
    out = []
    for ret, name, params in re.findall(r"^\s*(int|size_t|const char\*)\s+(cdetr_\w+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        args = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            base, star = re.fullmatch(r"\s*(?:const\s+)?(\w+)\s*(\*?)\s*\w+\s*", p).groups()
            args.append((base, star == "*"))
        out.append((name, ret, args))
    return out


def function_names():
    """Every declared function, sorted: read more loosely than prototypes(), so a prototype that one cannot parse is still counted."""
    src = re.sub(r"/\*.*?\*/", "", source(), flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(cdetr_\w+)\s*\(", src, flags=re.M)))


def field_names(struct_name):
    return [f[0] for f in struct_fields(struct_name)]


def header_name(cls):
    """_ffi.EmitDetectionsDesc -> "cdetr_emit_detections_desc"."""
    return "cdetr_" + re.sub(r"(?<!^)(?=[A-Z])", "_", cls.__name__).lower()
