"""CPU-only: what mtmp_ffn_block and mtmp_ffn_block_grouped REFUSE, in the manner of tests/test_abi_refusals_cpu.py: every case is a
call that must come back with MTMP_ERR_ARG and a message that names the entry, before anything touches a GPU.  The pointers are
made-up addresses that a launched kernel would dereference, so NO case may pass the checks; the host arrays of the grouped entry,
which the checks themselves index, are real arrays."""
import ctypes
import os

import pytest

MTMP_ERR_ARG = 1
P, P2 = 0x100000, 0x900000                 # "device pointers" far enough apart that x and out do not overlap


def _ptrs(v):
    return (ctypes.c_void_p * 3)(v, v, v)


def _ints(v):
    return (ctypes.c_int * 3)(v, v, v)


PA, PO, PA0 = _ptrs(P), _ptrs(P2), _ptrs(None)
# dtype, x, ldx, gamma, beta, w1, c1, w2, c2, out, ldo, M, eps, stream
SINGLE = [1, P, 256, P, P, P, P, P, P, P2, 256, 300, 1e-6, None]
# dtype, n, x, ldx, gamma, beta, w1, c1, w2, c2, out, ldo, M, eps, rows_live, stream
GROUPED = [1, 1, PA, _ints(256), PA, PA, PA, PA, PA, PA, PO, _ints(256), _ints(300), 1e-6, None, None]

CASES = {
    "mtmp_ffn_block": (SINGLE, [("null_x", {1: None}), ("null_gamma", {3: None}), ("null_beta", {4: None}), ("null_w1", {5: None}),
                                ("null_c1", {6: None}), ("null_w2", {7: None}), ("null_c2", {8: None}), ("null_out", {9: None}),
                                ("M0", {11: 0}), ("Mneg", {11: -5}), ("ldx_small", {2: 248}), ("ldx_odd", {2: 260}),
                                ("ldo_small", {10: 248}), ("ldo_odd", {10: 260}), ("in_place", {9: P}),
                                ("overlap", {9: P + 512}), ("dtype7", {0: 7})]),
    "mtmp_ffn_block_grouped": (GROUPED, [("null_x", {2: PA0}), ("null_out", {10: PA0}), ("null_w2", {8: PA0}), ("null_array", {4: None}),
                                         ("M0", {12: _ints(0)}), ("ldx_small", {3: _ints(248)}), ("ldx_odd", {3: _ints(260)}),
                                         ("ldo_odd", {11: _ints(260)}), ("in_place", {10: PA}), ("fp32", {0: 0}), ("dtype7", {0: 7}),
                                         ("n0", {1: 0}), ("n4", {1: 4})]),
}


def _cases():
    for entry, (good, cases) in CASES.items():
        for label, change in cases:
            args = list(good)
            for i, v in change.items():
                args[i] = v
            yield pytest.param(entry, args, id=f"{entry}-{label}")


@pytest.fixture(scope="module")
def lib():
    from medical_tri_modal_pilot_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


@pytest.mark.parametrize("entry,args", _cases())
def test_refused_before_any_launch(lib, entry, args):
    rc = getattr(lib, entry)(*args)
    msg = (lib.mtmp_last_error() or b"").decode()
    assert rc == MTMP_ERR_ARG, (entry, rc, msg)
    assert msg.startswith(entry + ":"), (entry, msg)


def test_signatures_match_the_header(lib):
    from medical_tri_modal_pilot_amd import _lib
    from tests import abi
    for name in CASES:
        ret, args = abi.declaration(name)
        assert ret == "int" and len(_lib.SIGNATURES[name][1]) == len(args) == len(CASES[name][0]), name
    assert lib.mtmp_abi_version() == 6
