"""The C ABI as Python reads it: include/acr_hip.h parsed once at import (no torch: evaluation.py's numpy half imports this).

``prototypes``: name -> (restype, [argtypes]); ``constants``: every enumerator and ``#define NAME literal``; ``structs``: name -> a
ctypes.Structure with the header's fields in order (ctypes applies the C layout rules); ``record_dtype(name)``: its numpy dtype.
The parser accepts exactly the declarations the header uses and raises on anything else, naming the line: a
prototype it skipped would be called with ctypes' default int arguments.
"""
import ctypes
import os
import re

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "acr_hip.h")

SCALARS = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
           "uint8_t": ctypes.c_uint8, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double}
_TYPE = r"((?:const\s+)?\w+\s*\**)"
_NUMBER = r"[-+]?(?:0[xX][0-9a-fA-F]+|\d+|(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?)"


class HeaderError(ValueError):
    pass


def _ctype(spelling, structs, where, ret=False):
    """ctypes type of a C type spelling such as ``const float*`` (None for a ``void`` return)."""
    const, base, stars = re.fullmatch(r"(const\s+)?(\w+)\s*(\**)", spelling.strip()).groups()
    if not stars and base in SCALARS:
        return SCALARS[base]
    if ret and not stars and base == "void":
        return None
    if ret and const and (base, stars) == ("char", "*"):
        return ctypes.c_char_p
    if stars == "*" and base in structs:
        return ctypes.POINTER(structs[base])
    if (base, stars) == ("void", "**"):
        return ctypes.POINTER(ctypes.c_void_p)
    if stars == "*" and (base in SCALARS or base == "void"):
        return ctypes.c_void_p
    raise HeaderError("unknown type '%s' in %s" % (spelling.strip(), where))


def _statements(text):
    """(line number, text) of every preprocessor line and of every declaration up to its top-level ';'."""
    text = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), text, flags=re.S)
    pending, start, depth, cplusplus = "", 0, 0, False
    for no, line in enumerate(text.split("\n"), 1):
        line = line.strip()
        if line.startswith("#"):
            if pending.strip():
                raise HeaderError("line %d: '%s' splits the declaration '%s'" % (no, line, pending.strip()))
            cplusplus = line == "#ifdef __cplusplus"       # only the extern "C" braces may stand between it and the #endif
            yield no, line
        elif cplusplus:
            if line not in ("", 'extern "C" {', "}"):
                raise HeaderError("line %d: '%s' inside #ifdef __cplusplus" % (no, line))
        else:
            for ch in line + " ":
                if ch == ";" and depth == 0:
                    yield start, pending.strip()
                    pending = ""
                    continue
                start = start if pending.strip() else no
                pending += ch
                depth += (ch == "{") - (ch == "}")
    if pending.strip():
        raise HeaderError("line %d: unterminated declaration '%s'" % (start, pending.strip()))


def parse(text):
    """(prototypes, constants, structs) of a header's text."""
    prototypes, constants, structs, guard = {}, {}, {}, None
    for no, st in _statements(text):
        where = "line %d: '%s'" % (no, st)
        if st.startswith("#"):
            m = re.fullmatch(r"#define\s+(\w+)\s+(%s)" % _NUMBER, st)
            if m and m.group(1) not in constants:
                lit = m.group(2)
                constants[m.group(1)] = float(lit) if re.search(r"[.eE]", lit) and "x" not in lit.lower() else int(lit, 0)
            elif re.fullmatch(r"#ifndef\s+\w+", st) and guard is None:
                guard = st.split()[1]
            elif st != "#define %s" % guard and not re.fullmatch(r"#include\s*<\w+\.h>|#ifdef __cplusplus|#endif", st):
                raise HeaderError("unsupported preprocessor %s" % where)
            continue
        m = re.fullmatch(r"typedef\s+(enum|struct)\s+(\w+)\s*\{(.*)\}\s*(\w+)", st)
        if m and m.group(2) == m.group(4) and m.group(1) == "enum":
            for item in filter(None, (s.strip() for s in m.group(3).split(","))):
                e = re.fullmatch(r"(\w+)\s*=\s*(-?\d+)", item)
                if not e or e.group(1) in constants:
                    raise HeaderError("enumerator '%s' without an explicit value or defined twice in %s" % (item, where))
                constants[e.group(1)] = int(e.group(2))
        elif m and m.group(2) == m.group(4):
            fields = []
            for member in filter(None, (s.strip() for s in m.group(3).split(";"))):
                d = re.fullmatch(_TYPE + r"\s*(\w+(?:\s*,\s*\w+)*)", member)
                if not d or ("*" in d.group(1) and "," in d.group(2)):
                    raise HeaderError("member '%s' of %s" % (member, where))
                fields += [(name.strip(), _ctype(d.group(1), structs, where)) for name in d.group(2).split(",")]
            if m.group(2) in structs:
                raise HeaderError("struct defined twice in %s" % where)
            structs[m.group(2)] = type(m.group(2), (ctypes.Structure,), {"_fields_": fields})
        else:
            m = re.fullmatch(_TYPE + r"\s*(\w+)\s*\(([^()]*)\)", st)
            if not m or m.group(2) in prototypes:
                raise HeaderError("unsupported declaration %s" % where)
            args = []
            for p in ([] if m.group(3).strip() == "void" else m.group(3).split(",")):
                d = re.fullmatch(_TYPE + r"\s*(\w+)", p.strip())
                if not d:
                    raise HeaderError("parameter '%s' of %s" % (p.strip(), where))
                args.append(_ctype(d.group(1), structs, where))
            prototypes[m.group(2)] = (_ctype(m.group(1), structs, where, ret=True), args)
    return prototypes, constants, structs


with open(HEADER) as _f:
    prototypes, constants, structs = parse(_f.read())


def record_dtype(name):
    """numpy dtype of a device-table record: the header struct's fields at the offsets the C compiler gives them."""
    return np.dtype(structs[name])
