"""What the C-ABI tests (tests/test_*abi*.py) share: the loaded library, and the headers under include/ read as the binding has
to mirror them (helper module, not collected by pytest)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# C argument type -> what iterative_learning_nmpc_amd._lib.SIGNATURES binds it as: pointers to device memory, to host structures
# and the stream are void pointers; `long long *` is written through on the host
C_TYPES = {"void *": ctypes.c_void_p, "const float *": ctypes.c_void_p, "float *": ctypes.c_void_p, "const double *": ctypes.c_void_p,
           "const int *": ctypes.c_void_p, "int *": ctypes.c_void_p, "int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double,
           "long long": ctypes.c_longlong, "long long *": ctypes.POINTER(ctypes.c_longlong),
           "const nmpc_contact_cfg *": ctypes.c_void_p, "const nmpc_policy_rollout_cfg *": ctypes.c_void_p}
SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "long long": ctypes.c_longlong}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from iterative_learning_nmpc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def header(header_file):
    """include/<header_file>, comments aside"""
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", header_file)).read(), flags=re.S)


def declaration(header_file, name):
    """(argument names, ctypes argument list) of the header's declaration `int name(...)`"""
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header(header_file))
    assert m, f"{name} is not declared in include/{header_file}"
    names, types = [], []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        assert re.match(r"^(const )?(long long|\w+) \*?\w+$", a), a        # anything else is a declaration this parser does not read
        names.append(re.search(r"\w+$", a).group(0))
        types.append(C_TYPES[re.sub(r"\s*\w+$", "", a).strip()])
    return names, types


def struct_fields(header_file, typedef_name):
    """[(field name, ctypes type)] of `typedef struct { ... } typedef_name;` in declaration order: scalars by their C type,
    pointers as void pointers"""
    body = re.search(r"typedef struct \{([^}]*)\} " + typedef_name + r";", header(header_file)).group(1)
    fields = []
    for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
        m = re.match(r"^(const )?(long long|int|float|double) (.+)$", decl)
        assert m, decl
        for n in m.group(3).split(","):
            n = n.strip()
            assert re.match(r"^\*? ?\w+$", n), decl
            fields.append((n.lstrip("* "), ctypes.c_void_p if n.startswith("*") else SCALARS[m.group(2)]))
    return fields
