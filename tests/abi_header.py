"""include/cdetr_hip.h as the ABI tests read it: the fields of a descriptor struct in declaration order, and the header name of a ctypes twin
of counting_detr_amd/_ffi.py.  Not a test module; imported by tests/test_abi.py and the per-feature CPU tests."""
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


def field_names(struct_name):
    return [f[0] for f in struct_fields(struct_name)]


def header_name(cls):
    """_ffi.EmitDetectionsDesc -> "cdetr_emit_detections_desc"."""
    return "cdetr_" + re.sub(r"(?<!^)(?=[A-Z])", "_", cls.__name__).lower()
