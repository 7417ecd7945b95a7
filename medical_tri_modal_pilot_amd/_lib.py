"""ctypes binding of libmtmp_hip.so.

include/mtmp.h is the single source of the C ABI: the library's sources are compiled against it, and the restype / argtypes of
every entry point are read from its declarations here (SIGNATURES).  An entry point is added by declaring it there, defining it
and calling it; there is no table to edit.

The product path has NO fallback: if the shared library is missing or a symbol is
absent this module raises at import of the first op, and every non-zero status
from the library becomes a RuntimeError carrying mtmp_last_error().
"""
import ctypes
import os
import re
from ctypes import c_char_p, c_float, c_int, c_longlong, c_uint, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MTMP_LIB", os.path.join(_HERE, "libmtmp_hip.so"))   # MTMP_LIB: diagnostic builds only
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mtmp.h")

F32, BF16 = 0, 1

# Every scalar spelling the header passes or returns by value.  Anything else (double, size_t, a struct, ...) is refused by name:
# a type read wrongly here would hand a kernel garbage sizes without any error.
_SCALARS = {"int": c_int, "unsigned": c_uint, "long long": c_longlong, "float": c_float}
_DECLARATION = re.compile(r"(const char\*|[\w ]+?) ?\b(mtmp_[a-z0-9_]+) ?\(([^()]*)\)")


def _argtype(arg: str, decl: str):
    if "*" in arg:
        return c_void_p                                # every pointer, whatever it points to
    spelling, _, name = arg.rpartition(" ")            # by value: "<spelling> <name>"
    if spelling not in _SCALARS or not name.isidentifier():
        raise RuntimeError(f"include/mtmp.h: cannot read the parameter '{arg}' of '{decl}': by value the binding knows "
                           f"{sorted(_SCALARS)} followed by a name, nothing else")
    return _SCALARS[spelling]


def parse_header(text: str) -> dict:
    """name -> (restype, argtypes) of every function the text of a header like include/mtmp.h declares.  Comments and
    preprocessor lines are dropped; everything else has to be a declaration this reads completely, or it raises."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    text = text.replace('extern "C" {', ";").replace("}", ";")
    table = {}
    for decl in (" ".join(d.split()) for d in text.split(";")):
        if not decl:
            continue
        m = _DECLARATION.fullmatch(decl.replace(" *", "*"))
        if m is None:
            raise RuntimeError(f"include/mtmp.h: cannot read '{decl}' as the declaration of an entry point")
        ret, name, args = m.groups()
        if ret != "const char*" and ret not in _SCALARS:
            raise RuntimeError(f"include/mtmp.h: cannot read the return type '{ret}' of '{decl}'")
        if name in table:
            raise RuntimeError(f"include/mtmp.h: {name} is declared twice")
        argtypes = [] if args.strip() == "void" else [_argtype(a.strip(), decl) for a in args.split(",")]
        table[name] = (c_char_p if ret == "const char*" else _SCALARS[ret], argtypes)
    return table


def _read_header() -> dict:
    if not os.path.exists(HEADER_PATH):
        raise RuntimeError(f"{HEADER_PATH} not found: the binding reads every entry point's argument types from the public header, "
                           "which belongs to the source tree next to the package.  There is no built-in table to fall back to.")
    with open(HEADER_PATH) as f:
        return parse_header(f.read())


# name -> (restype, argtypes), read once at import
SIGNATURES = _read_header()

_lib = None


def lib():
    """The loaded library (loads on first use; raises if it was not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; "
                "g.build()'` (or `make -C medical_tri_modal_pilot_amd/csrc`). There is no CPU fallback.")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError if the symbol is missing
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().mtmp_last_error()
        raise RuntimeError(f"libmtmp_hip {what} failed (status {rc}): {msg.decode() if msg else '?'}")


def call(name: str, *args):
    check(getattr(lib(), name)(*args), name)
