"""CPU-only: the C-ABI surface of the one-launch attention half on maps of any size (mtmp_swin_attn_block_pad): declared in
include/mtmp.h with the signature of mtmp_swin_attn_block, listed in _lib.py's table, exported by the library the project's own
build makes, reachable through ops and SwinTransformerBlock -- and the ABI version stays 6.  No kernel is launched here."""
import ctypes
import inspect
import os

from tests import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "medical_tri_modal_pilot_amd", "libmtmp_hip.so")
NAME = "mtmp_swin_attn_block_pad"


def _library():
    if not os.path.exists(LIB):
        import __graft_entry__ as ge
        ge.build()
    return ctypes.CDLL(LIB)                          # loads without a GPU: HIP initialises lazily


def test_block_pad_entry_declared_listed_and_exported():
    lib = _library()
    ret, args = abi.declaration(NAME)
    assert (ret, args) == abi.declaration("mtmp_swin_attn_block"), args     # the signature of the window-multiple entry
    assert ret == "int" and len(args) == 21
    assert args[0] == "int dtype" and args[-2] == "const int32_t* rows_live" and args[-1] == "void* stream"
    from medical_tri_modal_pilot_amd import _lib
    assert NAME in _lib.SIGNATURES, f"{NAME} missing from _lib.SIGNATURES"
    restype, argtypes = _lib.SIGNATURES[NAME]
    assert restype is ctypes.c_int and len(argtypes) == len(args)
    assert (restype, argtypes) == abi.ctypes_of(NAME)                       # position by position
    assert (restype, argtypes) == _lib.SIGNATURES["mtmp_swin_attn_block"]
    assert hasattr(lib, NAME), f"{NAME} declared in include/mtmp.h but not exported"
    assert hasattr(lib, "mtmp_swin_attn_block")


def test_abi_version_stays_6():
    lib = _library()
    lib.mtmp_abi_version.restype = ctypes.c_int
    assert lib.mtmp_abi_version() == 6


def test_host_side_reaches_the_block_pad_entry():
    from medical_tri_modal_pilot_amd import ops
    from medical_tri_modal_pilot_amd.builder.models.src.swin_transformer import SwinTransformerBlock
    assert list(inspect.signature(ops.swin_attn_block_pad).parameters) == list(inspect.signature(ops.swin_attn_block).parameters)
    src = inspect.getsource(SwinTransformerBlock.forward)
    assert "ops.swin_attn_block_pad" in src and "ops.swin_attn_block " in src
    assert "swin_attn_block" not in inspect.getsource(SwinTransformerBlock.forward_train)      # the trained encoder is not touched
