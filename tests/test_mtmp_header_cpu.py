"""include/mtmp.h is the public C interface: it must compile on its own for a C and a C++ consumer (the library's sources
include it behind the HIP runtime's headers and as C++ only, and the binding and the ABI tests read it as text -- so only this
notices a type that needs another header, or something a C compiler refuses)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler(names):
    for n in names:
        path = shutil.which(n)
        if path:
            return path
    for path in ("/opt/rocm/lib/llvm/bin/clang", "/opt/rocm/llvm/bin/clang"):
        if os.path.exists(path):
            return path
    return None


@pytest.mark.parametrize("lang,names", [("c", ("cc", "gcc", "clang")), ("c++", ("c++", "g++", "clang++"))])
def test_public_header_compiles_on_its_own(tmp_path, lang, names):
    cc = _compiler(names)
    if cc is None:
        pytest.skip("no host compiler")
    src = tmp_path / ("use_mtmp." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "mtmp.h"\n#include "mtmp.h"\nint use_mtmp(void) { return mtmp_abi_version(); }\n')
    r = subprocess.run([cc, "-x", lang, "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    text = open(os.path.join(ROOT, "include", "mtmp.h")).read()
    assert text.count("#ifndef MTMP_H") == 1 and text.rstrip().endswith("#endif /* MTMP_H */")
