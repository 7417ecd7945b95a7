"""CPU-only: the C-ABI surface of the padded-window attention entries (mtmp_swin_window_attn_pad / _pad_bwd): declared in
include/mtmp.h, listed in _lib.py's table with the same argument count, exported by the library the project's own build makes,
and reachable through ops and ShiftedWindowAttention.  No kernel is launched here."""
import ctypes
import inspect
import os

import pytest

from tests import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "medical_tri_modal_pilot_amd", "libmtmp_hip.so")
ENTRIES = {"mtmp_swin_window_attn_pad": 14, "mtmp_swin_window_attn_pad_bwd": 16}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_padded_window_entries_declared_listed_and_exported(name):
    if not os.path.exists(LIB):
        import __graft_entry__ as ge
        ge.build()
    ret, args = abi.declaration(name)
    assert ret == "int" and len(args) == ENTRIES[name], args
    assert args[0] == "int dtype" and args[2] == "const float* qkv_bias" and args[-1] == "void* stream"
    from medical_tri_modal_pilot_amd import _lib
    assert name in _lib.SIGNATURES, f"{name} missing from _lib.SIGNATURES"
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is ctypes.c_int and len(argtypes) == len(args)
    assert (restype, argtypes) == abi.ctypes_of(name)          # position by position
    lib = ctypes.CDLL(LIB)                       # loads without a GPU: HIP initialises lazily
    assert hasattr(lib, name), f"{name} declared in include/mtmp.h but not exported"


def test_existing_window_entries_keep_their_signatures():
    assert len(abi.declaration("mtmp_swin_window_attn")[1]) == 12
    assert len(abi.declaration("mtmp_swin_window_attn_live")[1]) == 13
    assert len(abi.declaration("mtmp_swin_window_attn_bwd")[1]) == 14


def test_host_side_reaches_the_padded_entries():
    from medical_tri_modal_pilot_amd import ops
    from medical_tri_modal_pilot_amd.builder.models.src.swin_transformer import ShiftedWindowAttention
    assert list(inspect.signature(ops.swin_window_attn_pad).parameters) == ["qkv", "bias", "table", "heads", "shift"]
    assert list(inspect.signature(ops.swin_window_attn_pad_bwd).parameters) == ["qkv", "bias", "table", "dout", "heads", "shift"]
    assert issubclass(ops.WindowAttnPadFn, __import__("torch").autograd.Function)
    src = inspect.getsource(ShiftedWindowAttention)
    assert "WindowAttnPadFn" in src and "swin_window_attn_pad" in src
    assert "224" not in inspect.getsource(ShiftedWindowAttention.forward_train)      # training is no longer tied to 224 / 448 pixels
