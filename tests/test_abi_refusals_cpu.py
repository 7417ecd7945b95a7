"""CPU-only: what the C entry points of the GEMM / elementwise / Swin / stem / attention files REFUSE, and how they say it.

Arguments that MTMP_CHECK_ARG refuses never reach HIP, so the library is called here without a GPU: every row of the table below
is a call that must come back with MTMP_ERR_ARG and a message that names the entry.  Per entry: a null required pointer, a bad
shape or leading dimension, a dtype the entry does not take (7 where it dispatches on dtype, fp32 where it is bf16-only) and, for
the grouped entries, n = 0 and n = 4; products with a single and a grouped form get the same bad shape through both.

The rows are spelled as one good call per entry plus the single argument each case changes.  NO case may pass the checks: the
pointers are made-up addresses that a launched kernel would dereference.  A refused call never reads them -- the HOST arrays of
the grouped entries, which the checks themselves index, are real arrays.

The name in a message is the entry's own or that of the family it forwards to (mtmp_gemm_nt_live says "mtmp_gemm_nt:",
mtmp_attn_fwd_grouped says "mtmp_attn_fwd:"), hence the prefix rule in _names_entry."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MTMP_ERR_ARG = 1
P, P2 = 0x1000, 0x2000                     # "device pointers": never read by a refused call


def _ptrs(*v):
    return (ctypes.c_void_p * 3)(*(v + (P,) * (3 - len(v))))


def _ints(*v):
    return (ctypes.c_int * 3)(*(v + (v[-1],) * (3 - len(v))))


PA, PA0 = _ptrs(P), _ptrs(None)            # host pointer arrays of a grouped entry: all set / first entry NULL
F1, U0 = (ctypes.c_float * 3)(0.1, 0.1, 0.1), (ctypes.c_uint * 3)(0, 0, 0)
I = _ints

# entry -> (the arguments of a call that would be accepted, [(case, {argument index: refused value})])
CALLS = {
    # ---- gemm.hip: single forms
    "mtmp_ln_gemm": ([1, P, P, P, P, None, P, None, None, 300, 1024, 256, 1024, 1e-5, 1, 0.1, 0, None, None],
                     [("null", {1: None}), ("ldx", {11: 250}), ("dtype7", {0: 7}), ("dropout", {15: 1.0})]),
    "mtmp_ln_gemm_qkv": ([1, P, P, P, P, None, P, None, None, P, 300, 256, 1e-5, None],
                         [("null", {9: None}), ("ldx", {11: 250}), ("dtype7", {0: 7})]),
    "mtmp_ln_gemm_signs": ([1, P, P, P, P, None, P, None, None, 300, 1024, 256, 1024, 1e-5, 0.1, 0, None, P, None],
                           [("null", {17: None}), ("N", {10: 1000}), ("N96", {10: 96, 12: 96}), ("fp32", {0: 0}), ("ldx", {11: 250})]),
    "mtmp_gemm_nt_signs": ([1, P, P, P, 300, 1024, 256, 1024, P, 1.0, None],
                           [("null", {8: None}), ("lda", {6: 250}), ("fp32", {0: 0})]),
    "mtmp_gemm_nt_signs_drop": ([1, P, P, P, 300, 1024, 256, 1024, P, 1.0, 0.1, 0, None, None, None],
                                [("null", {1: None}), ("lda", {6: 250}), ("M2p24", {4: 1 << 24}), ("fp32", {0: 0})]),
    "mtmp_gemm_nt": ([1, P, P, None, None, P, 300, 256, 1024, 1024, 256, 0, 0, 0.1, 0, None, None, 1.0, None, 1, None],
                     [("null", {5: None}), ("ldy", {10: 200}), ("dtype7", {0: 7}), ("act", {12: 3})]),
    "mtmp_gemm_nt_live": ([1, P, P, None, None, P, 300, 256, 1024, 1024, 256, 0, 0, 0.1, 0, None, None, 1.0, None, 1, None, None],
                          [("null", {1: None}), ("ldy", {10: 200}), ("dtype7", {0: 7})]),
    "mtmp_gemm_lnbwd": ([1, P, P, P, 256, P, P, None, 0, P, P, P, 300, 1024, 1024, 1e-5, None],
                        [("null", {11: None}), ("ldz", {4: 250}), ("dtype7", {0: 7})]),
    "mtmp_gemm_tn": ([1, P, P, P, None, P, 300, 1024, 256, 1024, 256, None],
                     [("null", {5: None}), ("ldy", {9: 1000}), ("dtype7", {0: 7}), ("db_without_dw", {3: None, 4: P})]),
    "mtmp_gemm_tn_live": ([1, P, P, P, None, P, 300, 1024, 256, 1024, 256, None, None],
                          [("null", {1: None}), ("ldy", {9: 1000}), ("dtype7", {0: 7})]),
    "mtmp_dropout_bwd": ([1, P, P, 1024, 0, None, 0.1, None], [("null", {1: None}), ("n", {3: 1023}), ("dtype7", {0: 7})]),
    # ---- gemm.hip: grouped forms (bf16 only, 1..3 streams); the bad shapes are those of the single forms above
    "mtmp_ln_gemm_qkv_grouped": ([1, 1, PA, PA, PA, PA, None, PA, None, None, PA, I(300), I(256), 1e-5, None, None],
                                 [("null", {10: PA0}), ("ldx", {12: I(250)}), ("fp32", {0: 0}), ("n0", {1: 0}), ("n4", {1: 4})]),
    "mtmp_ln_gemm_signs_grouped": ([1, 1, PA, PA, PA, PA, None, PA, None, None, PA, I(300), 1024, I(256), 1e-5, 0.1, None, None, None, None],
                                   [("null", {10: PA0}), ("N", {12: 1000}), ("N96", {12: 96}), ("ldx", {13: I(250)}), ("fp32", {0: 0}),
                                    ("n0", {1: 0}), ("n4", {1: 4})]),
    "mtmp_gemm_nt_signs_drop_grouped": ([1, 1, PA, PA, PA, I(300), 1024, I(256), PA, 1.0, 0.1, None, None, None, None, None],
                                        [("null", {2: PA0}), ("lda", {7: I(250)}), ("M2p24", {5: I(1 << 24)}), ("fp32", {0: 0}),
                                         ("n0", {1: 0}), ("n4", {1: 4})]),
    "mtmp_gemm_nt_grouped": ([1, 1, PA, PA, None, None, PA, I(300), 256, 1024, I(1024), I(256), None, 0, 0.1, None, None, None, None],
                             [("null", {6: PA0}), ("ldy", {11: I(200)}), ("act", {13: 3}), ("fp32", {0: 0}), ("n0", {1: 0}), ("n4", {1: 4})]),
    "mtmp_gemm_lnbwd_grouped": ([1, 1, PA, PA, PA, I(256), PA, PA, None, None, PA, PA, I(300), 1024, I(1024), 1e-5, None, None],
                                [("null", {11: PA0}), ("ldz", {5: I(250)}), ("fp32", {0: 0}), ("n0", {1: 0}), ("n4", {1: 4})]),
    "mtmp_gemm_tn_grouped": ([1, 1, PA, PA, PA, I(300), 1024, 256, I(1024), I(256), I(1), None, None],
                             [("null", {4: PA0}), ("ldy", {8: I(1000)}), ("K200", {7: 200}), ("splits0", {10: I(0)}), ("fp32", {0: 0}),
                              ("n0", {1: 0}), ("n4", {1: 4})]),
    # ---- elementwise.hip
    "mtmp_ln_bwd": ([1, P, 256, P, P, P, None, 0, P, P, P, 300, 1e-5, None], [("null", {1: None}), ("ldz", {2: 250}), ("dtype7", {0: 7})]),
    "mtmp_tie_embed_fwd": ([1, P, P, P, P, 100, None], [("null", {1: None}), ("n", {5: 0}), ("dtype7", {0: 7})]),
    "mtmp_time_embed_fwd": ([1, P, P, P, P, 100, None], [("null", {4: None}), ("n", {5: 0}), ("dtype7", {0: 7})]),
    "mtmp_tie_embed_bwd": ([1, P, P, P, P, P, 100, None], [("null", {5: None}), ("n", {6: 0}), ("dtype7", {0: 7})]),
    "mtmp_time_embed_bwd": ([1, P, P, P, P, P, 100, None], [("null", {3: None}), ("n", {6: 0}), ("dtype7", {0: 7})]),
    "mtmp_tie_embed_packed_fwd": ([1, P, P, 4, 32, P, P, P, None], [("null", {2: None}), ("t_pad", {4: 0}), ("dtype7", {0: 7})]),
    "mtmp_tie_embed_packed_bwd": ([1, P, P, 4, 32, P, P, P, P, None], [("null", {8: None}), ("B", {3: 0}), ("dtype7", {0: 7})]),
    "mtmp_tie_time_embed_bwd_partials": ([1, P, 100, P, 10, 5, P, P, P, P, P, None],
                                         [("null", {3: None}), ("n_time_a", {5: 11}), ("dtype7", {0: 7})]),
    "mtmp_hourly_embed_fwd": ([1, P, P, P, P, 100, 18, None], [("null", {2: None}), ("F", {6: 19}), ("dtype7", {0: 7})]),
    "mtmp_hourly_embed_bwd": ([1, P, P, P, P, P, P, 100, 18, None], [("null", {6: None}), ("F", {8: 0}), ("dtype7", {0: 7})]),
    "mtmp_stream_input_fwd": ([1, P, P, P, P, None, P, P, P, 4, 32, 4, 1e-5, 0.1, 0, None, None, None, None],
                              [("null", {7: None}), ("nb", {11: 5}), ("packed_without_kv_len", {16: P}), ("dtype7", {0: 7})]),
    "mtmp_stream_input_fwd_add": ([1, P, P, P, P, None, P, P, P, 4, 32, 4, 1e-5, 0.1, 0, None, None, None, P, 8, None],
                                  [("null", {7: None}), ("nb", {11: 5}), ("add_L", {19: 0}), ("add_L_divides", {19: 5}), ("dtype7", {0: 7})]),
    "mtmp_stream_input_bwd": ([1, P, P, P, P, P, P, P, P, 4, 32, 4, 0.1, 0, None, None, None, None],
                              [("null", {7: None}), ("N", {10: 0}), ("dtype7", {0: 7})]),
    "mtmp_stream_input_bwd_partials": ([1, P, P, P, P, P, P, P, 4, 32, 4, 0.1, 0, None, None, None, None],
                                       [("null", {7: None}), ("p", {11: 1.0}), ("dtype7", {0: 7})]),
    "mtmp_stream_input_bwd_grouped": ([1, 1, PA, PA, PA, PA, PA, PA, P, I(4), I(32), I(4), F1, U0, None, None, None, None, None, None],
                                      [("null", {2: PA0}), ("N", {10: I(0)}), ("dtype7", {0: 7}), ("n0", {1: 0}), ("n4", {1: 4})]),
    "mtmp_token_sums": ([1, 1, PA, PA, I(4), I(8), None], [("null", {2: PA0}), ("L", {5: I(0)}), ("dtype7", {0: 7}), ("n0", {1: 0}), ("n3", {1: 3})]),
    "mtmp_bottleneck_exchange_fwd": ([1, P, P, P, 4, 10, 10, 10, P, 0, None, None, None, None],
                                     [("null", {8: None}), ("n_v", {5: 3}), ("dtype7", {0: 7})]),
    "mtmp_bottleneck_exchange_bwd": ([1, P, P, P, 4, 10, 10, 10, P, 0, None, None, None, None],
                                     [("null", {1: None}), ("n_i", {6: 3}), ("dtype7", {0: 7})]),
    # ---- stem.hip, swin.hip
    "mtmp_swin_stem_fwd": ([1, P, P, P, P, P, P, 2, 32, 32, None], [("null", {6: None}), ("H", {8: 30}), ("dtype7", {0: 7})]),
    "mtmp_swin_stem_fwd_live": ([1, P, P, P, P, P, P, 2, 32, 32, None, None, None], [("null", {1: None}), ("W", {9: 30}), ("dtype7", {0: 7})]),
    "mtmp_layernorm_rows": ([1, P, P, P, P, 100, 96, 1e-5, 0, 0, 0, None], [("null", {4: None}), ("C", {6: 100}), ("dtype7", {0: 7})]),
    "mtmp_layernorm_rows_live": ([1, P, P, P, P, 100, 96, 1e-5, 0, 0, 0, None, None], [("rows", {5: 0}), ("merge", {8: 1, 9: 3, 10: 4}), ("dtype7", {0: 7})]),
    "mtmp_swin_window_attn": ([1, P, P, P, 2, 14, 14, 96, 3, 0, 0.17, None], [("null", {2: None}), ("H", {5: 15}), ("dtype7", {0: 7}),
                               ("one_window_shifted", {5: 7, 6: 7, 9: 3}), ("one_window_side_shifted", {5: 7, 9: 3})]),
    "mtmp_swin_window_attn_live": ([1, P, P, P, 2, 14, 14, 96, 3, 0, 0.17, None, None], [("null", {3: None}), ("shift", {9: 7}), ("dtype7", {0: 7}),
                                    ("one_window_shifted", {5: 7, 6: 7, 9: 3}), ("one_window_side_shifted", {6: 7, 9: 3})]),
    "mtmp_swin_window_attn_pad": ([1, P, P, P, P, 2, 16, 16, 96, 3, 0, 0.17, None, None],
                                  [("null", {2: None}), ("C", {8: 100}), ("one_window_shifted", {6: 5, 7: 5, 10: 1}), ("dtype7", {0: 7})]),
    "mtmp_swin_mlp": ([1, P, P, P, P, P, P, P, None, 1, P2, 100, 96, 1e-5, None],
                      [("null", {4: None}), ("aliased", {10: P}), ("C", {12: 128}), ("fp32", {0: 0})]),
    "mtmp_swin_mlp_live": ([1, P, P, P, P, P, P, P, None, 1, P2, 100, 96, 1e-5, None, None], [("null", {1: None}), ("M", {11: 0}), ("fp32", {0: 0})]),
    "mtmp_swin_ln_linear": ([1, P, P, P, P, None, P, 100, 96, 288, 1e-5, None], [("null", {6: None}), ("N", {9: 100}), ("fp32", {0: 0})]),
    "mtmp_swin_ln_linear_live": ([1, P, P, P, P, None, P, 100, 96, 288, 1e-5, None, None], [("null", {4: None}), ("C", {8: 128}), ("fp32", {0: 0})]),
    "mtmp_swin_attn_block": ([1, P, P, P, 1e-5, P, P, P, P, P, None, P2, 2, 14, 14, 96, 3, 0, 0.17, None, None],
                             [("null", {7: None}), ("in_place", {11: P}), ("H", {13: 15}), ("fp32", {0: 0}),
                              ("one_window_shifted", {13: 7, 14: 7, 17: 3}), ("one_window_side_shifted", {13: 7, 17: 3})]),
    "mtmp_swin_attn_block_pad": ([1, P, P, P, 1e-5, P, P, P, P, P, None, P2, 2, 16, 16, 96, 3, 0, 0.17, None, None],
                                 [("null", {7: None}), ("heads", {16: 4}), ("one_side_single_window", {14: 5}),
                                  ("one_window_shifted", {13: 5, 14: 5, 17: 1}), ("fp32", {0: 0})]),
    # ---- swin_bwd.hip
    "mtmp_layernorm_rows_bwd": ([1, P, P, P, P, P, 100, 96, 1e-5, None], [("null", {5: None}), ("C", {7: 100}), ("dtype7", {0: 7})]),
    "mtmp_gelu_fwd": ([1, P, P, 1024, None], [("null", {2: None}), ("n", {3: 1001}), ("dtype7", {0: 7})]),
    "mtmp_gelu_bwd": ([1, P, P, P, 1024, None], [("null", {2: None}), ("n", {4: 1001}), ("dtype7", {0: 7})]),
    "mtmp_swin_window_attn_bwd": ([1, P, P, P, P, P, 2, 14, 14, 96, 3, 0, 0.17, None], [("null", {5: None}), ("W", {8: 15}), ("dtype7", {0: 7}),
                                   ("one_window_shifted", {7: 7, 8: 7, 11: 3}), ("one_window_side_shifted", {7: 7, 11: 3})]),
    "mtmp_swin_window_attn_pad_bwd": ([1, P, P, P, P, P, P, P, 2, 16, 16, 96, 3, 0, 0.17, None],
                                      [("null", {7: None}), ("heads", {12: 4}), ("one_window_shifted", {9: 5, 10: 5, 13: 1}), ("dtype7", {0: 7})]),
    # ---- attention.hip
    "mtmp_attn_fwd": ([1, P, P, P, P, None, None, P, None, None, 2, 100, 4, 768, 256, 0.125, None],
                      [("null", {7: None}), ("H", {12: 5}), ("res_without_o_res", {5: P}), ("dtype7", {0: 7})]),
    "mtmp_attn_fwd_grouped": ([1, 1, PA, PA, PA, PA, None, None, PA, None, None, None, I(100), I(768), I(256), 2, 4, 0.125, None],
                              [("null", {4: PA0}), ("ld_qkv", {13: I(250)}), ("dtype7", {0: 7}), ("n0", {1: 0}), ("n4", {1: 4})]),
    "mtmp_attn_bwd": ([1, P, P, P, P, P, P, None, P, P, P, P, 2, 100, 4, 768, 256, 256, 768, 0.125, None],
                      [("null", {11: None}), ("ld_dqkv", {18: 100}), ("dtype7", {0: 7})]),
    "mtmp_attn_bwd_grouped": ([1, 1, PA, PA, PA, PA, PA, PA, None, None, PA, PA, PA, PA, I(100), I(768), I(256), I(256), I(768), 2, 4, 0.125, None],
                              [("null", {13: PA0}), ("N", {14: I(0)}), ("dtype7", {0: 7}), ("n0", {1: 0}), ("n4", {1: 4})]),
    "mtmp_attn_cls_fwd": ([1, P, P, P, 768, P, 256, P, P, P, None, None, 2, 100, 4, 0, 0.125, None],
                          [("null", {5: None}), ("cls_tok", {15: 100}), ("dtype7", {0: 7})]),
    "mtmp_attn_cls_bwd": ([1, P, P, P, 768, P, P, P, None, None, P, P, P, 768, 2, 100, 4, 0, 0.125, None],
                          [("null", {10: None}), ("ld_dqkv", {13: 100}), ("dtype7", {0: 7})]),
    "mtmp_key_norms": ([1, P, P, 100, 4, 768, None], [("null", {2: None}), ("ld", {5: 100}), ("dtype7", {0: 7})]),
}

# the same bad shape through the single and the grouped form of every product that has both: (single, grouped, case)
PAIRS = [("mtmp_ln_gemm_qkv", "mtmp_ln_gemm_qkv_grouped", "ldx"), ("mtmp_ln_gemm_signs", "mtmp_ln_gemm_signs_grouped", "N"),
         ("mtmp_ln_gemm_signs", "mtmp_ln_gemm_signs_grouped", "N96"), ("mtmp_gemm_nt_signs_drop", "mtmp_gemm_nt_signs_drop_grouped", "lda"),
         ("mtmp_gemm_nt_signs_drop", "mtmp_gemm_nt_signs_drop_grouped", "M2p24"), ("mtmp_gemm_nt", "mtmp_gemm_nt_grouped", "ldy"),
         ("mtmp_gemm_lnbwd", "mtmp_gemm_lnbwd_grouped", "ldz"), ("mtmp_gemm_tn", "mtmp_gemm_tn_grouped", "ldy"),
         ("mtmp_attn_fwd", "mtmp_attn_fwd_grouped", None), ("mtmp_attn_bwd", "mtmp_attn_bwd_grouped", None)]


def _cases():
    for entry, (good, cases) in CALLS.items():
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


def _names_entry(msg, entry):
    said = msg.split(":")[0].split(" ")[0]
    return said.startswith("mtmp_") and (entry == said or entry.startswith(said + "_"))


@pytest.mark.parametrize("entry,args", _cases())
def test_refused_before_any_launch(lib, entry, args):
    rc = getattr(lib, entry)(*args)
    msg = (lib.mtmp_last_error() or b"").decode()
    assert rc == MTMP_ERR_ARG, (entry, rc, msg)
    assert _names_entry(msg, entry), (entry, msg)


def test_table_covers_what_it_promises():
    for entry, (good, cases) in CALLS.items():
        labels = [c for c, _ in cases]
        assert "null" in labels or entry.endswith("_live"), entry
        assert any(c in labels for c in ("dtype7", "fp32")), entry
        assert len(labels) >= 3 and len(set(labels)) == len(labels), entry
        if entry.endswith("_grouped") or entry == "mtmp_token_sums":
            assert "n0" in labels and ("n4" in labels or "n3" in labels), entry
    for single, grouped, case in PAIRS:
        assert single in CALLS and grouped in CALLS
        if case:
            assert case in [c for c, _ in CALLS[single][1]] and case in [c for c, _ in CALLS[grouped][1]], (single, case)
