"""include/acr_hip.h as the stage tests read it: their own regular expressions over the header's text, not acr_wsss_amd._abi --
a check against the parser's output would compare the parser with itself."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "include", "acr_hip.h")) as _f:
    HEADER = _f.read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
PROTOTYPES = {m.group(2): (" ".join(m.group(1).split()), [" ".join(p.split()) for p in m.group(3).split(",")])
              for m in re.finditer(r"^((?:const\s+)?\w+\s*\*?)\s*(acr_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", CODE, flags=re.M)}
SCALARS = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
           "float": ctypes.c_float, "double": ctypes.c_double}


def declared(name):
    """(return type, [parameter strings]) of the prototype of ``name``; a ``(void)`` list is [].  KeyError: not declared."""
    ret, params = PROTOTYPES[name]
    return ret, [] if params == ["void"] else params


def defined(name):
    """The literal of ``#define name literal`` as the header spells it."""
    return re.search(r"^#define\s+%s\s+(\S+)\s*$" % name, CODE, flags=re.M).group(1)


def ctype_of(c_type, structs=(), ret=False):
    """The ctypes type a C type of the header is bound as (``structs``: {C name: ctypes.Structure} for typed struct pointers)."""
    t = re.sub(r"\bconst\b", "", c_type).replace(" ", "")
    if t in SCALARS:
        return SCALARS[t]
    if ret and t == "char*":
        return ctypes.c_char_p
    if t == "void**":
        return ctypes.POINTER(ctypes.c_void_p)
    if t.endswith("*") and t[:-1] in structs:
        return ctypes.POINTER(dict(structs)[t[:-1]])
    assert t.endswith("*") and (t[:-1] in SCALARS or t[:-1] in ("void", "uint8_t")), c_type
    return ctypes.c_void_p


def check_bound(names, signatures):
    """Every name is declared and bound with one ctypes type per declared parameter, and an int64_t return is bound as c_int64."""
    for name in names:
        ret, params = declared(name)
        assert name in signatures and len(params) == len(signatures[name][1]), name
        assert (ret == "int64_t") == (signatures[name][0] is ctypes.c_int64), name
