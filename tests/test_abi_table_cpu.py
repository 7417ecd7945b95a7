"""CPU-only: include/mtmp.h is the one place the C ABI is written down.  The binding's table is read from it
(_lib.parse_header) and is held here, entry by entry and type by type, against the tests' own reading of the header
(tests/abi.py); the parser is strict on synthetic headers; and a definition that disagrees with its declaration does not
compile, which is what the library's sources rely on now that they include the header."""
import os
import re
import subprocess
from ctypes import c_char_p, c_float, c_int, c_longlong, c_uint, c_void_p

import pytest

from medical_tri_modal_pilot_amd import _lib
from tests import abi
from tests.test_mtmp_header_cpu import _compiler

ROOT = abi.ROOT
CSRC = os.path.join(ROOT, "medical_tri_modal_pilot_amd", "csrc")


def test_every_declared_entry_is_bound_with_its_declared_types():
    declared = abi.declarations()
    assert set(_lib.SIGNATURES) == set(declared) and len(declared) >= 129
    for name in declared:
        restype, argtypes = abi.ctypes_of(name)
        got_res, got_args = _lib.SIGNATURES[name]
        assert got_res is restype, (name, got_res, restype)
        assert len(got_args) == len(argtypes) == len(abi.declaration(name)[1]), name
        for i, (got, want) in enumerate(zip(got_args, argtypes)):
            assert got is want, (name, i, abi.declaration(name)[1][i], got, want)
    kinds = {t for _, args in _lib.SIGNATURES.values() for t in args}
    assert kinds == {c_int, c_uint, c_longlong, c_float, c_void_p}              # every kind the map knows is exercised
    assert _lib.SIGNATURES["mtmp_last_error"] == (c_char_p, []) and _lib.SIGNATURES["mtmp_abi_version"] == (c_int, [])


SYNTHETIC = """/* a header in the shape of mtmp.h.
 * int mtmp_hidden(int a, double b);  <- inside a comment, with ( , and ; around it: f(x, y); g(); */
#ifndef SYNTHETIC_H
#define SYNTHETIC_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define MTMP_ABI_VERSION 6

int mtmp_version(void);
const char* mtmp_text(void);
/* sizes (in floats); see mtmp_hidden(int a, double b); */
long long mtmp_floats(long long rows, int H);
int mtmp_launch(int dtype, const void* const* q, float *lse, const int32_t* const* kv_len,
                unsigned seed, const unsigned* seed_dev,
                long long n, float scale,
                unsigned long long* slot, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SYNTHETIC_H */
"""


def test_parser_reads_every_supported_spelling():
    assert _lib.parse_header(SYNTHETIC) == {
        "mtmp_version": (c_int, []),
        "mtmp_text": (c_char_p, []),
        "mtmp_floats": (c_longlong, [c_longlong, c_int]),
        "mtmp_launch": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_uint, c_void_p, c_longlong, c_float, c_void_p, c_void_p]),
    }
    assert _lib.parse_header("") == {} and _lib.parse_header("/* int mtmp_hidden(int a); */\n#define X 1\n") == {}


@pytest.mark.parametrize("decl", [
    "int mtmp_x(double x);", "int mtmp_x(int n, size_t bytes);", "int mtmp_x(struct pt);", "int mtmp_x(struct pt p);",
    "int mtmp_x(int (*cb)(int), void* stream);", "int mtmp_x(int);", "int mtmp_x();", "int mtmp_x(unsigned int n);",
    "int mtmp_x(int32_t n);", "int mtmp_x(const int n);", "int mtmp_x(int n, ...);", "double mtmp_x(void);", "void* mtmp_x(void);",
    "size_t mtmp_x(int n);", "void mtmp_x(int n);", "int mtmp_x(int n)", "int mtmp_x(int n) { return n; }"])
def test_parser_refuses_what_it_does_not_know_and_names_the_declaration(decl):
    with pytest.raises(RuntimeError, match="mtmp_x"):
        _lib.parse_header("int mtmp_before(void);\n" + decl + "\nint mtmp_after(void);\n")


@pytest.mark.parametrize("text,said", [("typedef int mtmp_t;", "typedef"), ("int other_entry(int n);", "other_entry"),
                                       ("struct pt { int x; };", "struct pt"),
                                       ("int mtmp_x(void);\nint mtmp_x(void);", "mtmp_x is declared twice")])
def test_parser_refuses_anything_that_is_not_one_declaration_per_entry(text, said):
    with pytest.raises(RuntimeError, match=said):
        _lib.parse_header(text)


def test_a_missing_header_is_an_error_that_says_where_it_should_be(monkeypatch, tmp_path):
    assert os.path.samefile(_lib.HEADER_PATH, abi.HEADER)            # the binding and the tests read the same file
    monkeypatch.setattr(_lib, "HEADER_PATH", str(tmp_path / "include" / "mtmp.h"))
    with pytest.raises(RuntimeError, match="mtmp.h not found"):
        _lib._read_header()


@pytest.mark.parametrize("params,compiles", [("void", True), ("int", False)])
def test_a_definition_that_differs_from_its_declaration_does_not_compile(tmp_path, params, compiles):
    cxx = _compiler(("c++", "g++", "clang++"))
    assert cxx is not None, "no host C++ compiler: the guard the library's build relies on cannot be checked"
    src = tmp_path / "define_entry.cpp"
    src.write_text('#include "mtmp.h"\nextern "C" int mtmp_abi_version(%s) { return MTMP_ABI_VERSION; }\n' % params)
    r = subprocess.run([cxx, "-x", "c++", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert (r.returncode == 0) == compiles, r.stdout
    assert compiles or "mtmp_abi_version" in r.stdout


def test_the_library_sources_are_compiled_against_the_header():
    """every .hip includes common.hip.h (directly or through head_common.hip.h), which includes the header, as error.cpp does;
    every object depends on it in the Makefile; no source declares an entry point for itself, on one line or several"""
    include = '#include "../../include/mtmp.h"'
    names = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".cpp")))
    assert {"gemm.hip", "attention.hip", "error.cpp", "common.hip.h", "head_common.hip.h"} <= set(names)
    for name in names:
        text = open(os.path.join(CSRC, name)).read()
        if name in ("error.cpp", "common.hip.h"):
            assert include in text, name
        else:
            assert '#include "common.hip.h"' in text or '#include "head_common.hip.h"' in text, name
        local = re.findall(r'^[ \t]*extern "C"[^{;]*;', text, re.M)  # a declaration: it reaches its ';' before any '{'
        assert not local, (name, local)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^ABI\s*:=\s*\.\./\.\./include/mtmp\.h\s*$", mk, re.M)
    compile_rules = [line for line in mk.split("\n") if ".o:" in line and any(w.endswith((".hip", ".cpp")) for w in line.split())]
    assert len(compile_rules) >= 4 and all("$(ABI)" in line for line in compile_rules), compile_rules
    assert "return MTMP_ABI_VERSION;" in open(os.path.join(CSRC, "error.cpp")).read()
    assert "#define MTMP_ABI_VERSION 6\n" in abi.header_text()
