"""What include/mtmp.h declares, read by the tests on their own: a scanner that shares nothing with the parser of
medical_tri_modal_pilot_amd/_lib.py, so that holding the two against each other (tests/test_abi_table_cpu.py) says something.

    declaration(name) -> (return type, [argument declarations]) as written, white space normalised
    ctypes_of(name)   -> (restype, [argtypes]) as ctypes must see that declaration
"""
import ctypes
import functools
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mtmp.h")

BY_VALUE = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "unsigned": ctypes.c_uint, "long long": ctypes.c_longlong,
            "float": ctypes.c_float}


def header_text():
    with open(HEADER) as f:
        return f.read()


def _code(text):
    """the text without block comments and preprocessor lines"""
    kept, at = [], 0
    while (start := text.find("/*", at)) >= 0:
        kept.append(text[at:start])
        at = text.index("*/", start) + 2
    kept.append(text[at:])
    return "\n".join(line for line in " ".join(kept).split("\n") if not line.lstrip().startswith("#"))


@functools.lru_cache(maxsize=None)
def declarations():
    """name -> (return type, [argument declarations]) of every entry point, in the header's order"""
    code, found = _code(header_text()), {}
    for m in re.finditer(r"\b(mtmp_[a-z0-9_]+)\s*\(", code):
        name, close = m.group(1), code.index(")", m.end())
        inside = code[m.end():close]
        assert "(" not in inside and code[close + 1:].lstrip().startswith(";"), f"{name}: not a plain declaration"
        assert name not in found, f"{name} is declared twice"
        begin = max(code.rfind(c, 0, m.start()) for c in ";{}") + 1
        args = [" ".join(a.split()) for a in inside.split(",")]
        found[name] = (" ".join(code[begin:m.start()].split()), [] if args == ["void"] else args)
    return found


def declaration(name):
    assert name in declarations(), f"{name} is not declared in include/mtmp.h"
    return declarations()[name]


def _by_value(spelling, where):
    assert spelling in BY_VALUE, f"{where}: no ctypes type for '{spelling}'"
    return BY_VALUE[spelling]


def ctypes_of(name):
    ret, args = declaration(name)
    if "*" in ret:
        assert ret == "const char*", f"{name}: returns '{ret}'"
    restype = ctypes.c_char_p if "*" in ret else _by_value(ret, name)
    # by value an argument is "<type> <name>"; every pointer travels as a void pointer
    return restype, [ctypes.c_void_p if "*" in a else _by_value(a.rpartition(" ")[0], f"{name}({a})") for a in args]
