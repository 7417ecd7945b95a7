"""The token-id report store on the CPU (builder/data/report_store.TokenReportStore): the host plan against the reference
``__getitem__`` goldens of ``--berttype bert`` (tests/golden/token_report_cases.npz), the models of the loader's rule and of the
kernel's closed form (tests/token_store_model.py) against their digests, the refusals, and the new entry points' declarations
and argument errors (the library loads without a GPU)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from medical_tri_modal_pilot_amd.builder.data import TokenReportBatch, TokenReportStore
from tests import token_store_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_store_of_the_golden_reports():
    g, st = M.golden(), M.golden_store()
    assert tuple(g["report_len"].tolist()) == M.GOLDEN_LENGTHS and len(g["case_file"]) == 40
    assert st.n_reports == 7 and st.n_tokens == sum(M.GOLDEN_LENGTHS) and st.nbytes == 4 * st.n_tokens
    assert st.tok_ptr.dtype == np.int64 and st.tok_ptr.tolist() == np.concatenate([[0], np.cumsum(g["report_len"])]).tolist()
    assert st.ids.dtype == torch.int32 and tuple(st.ids.shape) == (st.n_tokens,) and st.ids.is_contiguous()
    assert (st.vocab, st.max_length, st.device.type) == (30000, 128, "cpu") and st.to("cpu") is st
    for k, f in enumerate(g["report_file"]):
        assert st.index_of(int(f), 0) == st.index_of(np.int64(f), 0.0) == k
    assert st.index_of(12345, 0) == st.index_of(int(g["report_file"][0]), 1) == -1
    assert set(st.ids.tolist()) >= set(M.SPECIAL)
    assert sorted(set(g["text_length"].tolist())) == [0, 1, 5, 37, 125, 126, 127, 200]


def test_plan_on_the_golden_cases():
    g, st = M.golden(), M.golden_store()
    idx = M.golden_report_idx(st)
    assert (idx >= 0).sum() == 28 and (idx < 0).sum() == 12          # seven txt1 files, three txt0 files, four combinations each
    b = st.plan(idx, g["case_comb"])
    assert isinstance(b, TokenReportBatch) and b.batch_size == 40 and b.store is st and b.max_length == 128
    assert b.txt_lengths.dtype == torch.int64 and b.txt_lengths.tolist() == g["text_length"].tolist()      # UNTRIMMED: 200 stays 200
    assert b.missing.dtype == torch.float32 and b.missing.tolist() == g["missing"][:, 2].tolist()
    assert b.n_tokens.tolist() == g["text_length"].tolist() and (b.first_token[b.n_tokens == 0] == 0).all()
    d = b.descriptor()
    assert d.dtype == torch.int64 and tuple(d.shape) == (40, 2) and d.is_contiguous()
    for lo in range(0, 40, 10):                                      # the batches of ten the GPU test gathers
        bb = st.plan(idx[lo:lo + 10], g["case_comb"][lo:lo + 10])
        assert bb.txt_lengths.tolist() == g["text_length"][lo:lo + 10].tolist()
    one = st.plan(idx[:8], 3)                                        # one combination for the whole batch
    assert one.txt_lengths.tolist() == [0] * 8 and one.missing.tolist() == [1.0] * 8


def test_key_lengths():
    """min(textLength, L - 2): the model's key count textLength + 2 never names more rows than the stream's L"""
    g, st = M.golden(), M.golden_store()
    b = st.plan(M.golden_report_idx(st), g["case_comb"])
    assert b.key_lengths.dtype == torch.int64
    assert b.key_lengths.tolist() == [min(int(n), 126) for n in g["text_length"]]
    assert set(b.key_lengths.tolist()) == {0, 1, 5, 37, 125, 126} and int((b.key_lengths + 2).max()) == 128
    small = TokenReportStore.from_mapping({(0, 0): [5, 6, 7, 8], (1, 0): [9], (2, 0): []}, vocab=10, max_length=5)
    sb = small.plan(np.asarray([0, 1, 2, -1]))
    assert sb.txt_lengths.tolist() == [4, 1, 0, 0] and sb.key_lengths.tolist() == [3, 1, 0, 0] and sb.missing.tolist() == [0, 0, 1, 1]


def test_models_reproduce_the_golden_digests():
    """the loader's rule restated branch by branch AND the kernel's closed form, on the 40 cases"""
    g, st = M.golden(), M.golden_store()
    b = st.plan(M.golden_report_idx(st), g["case_comb"])
    tok = M.plan_ids(b, st.ids.numpy())
    assert tok.dtype == torch.float32 and tuple(tok.shape) == (40, 128)
    assert [M.digest(t) for t in tok] == g["sha256"].tolist()
    closed = M.closed_form_ids(b.first_token, b.n_tokens, st.ids.numpy(), 128)
    assert closed.dtype == np.int32 and [M.digest(r.astype(np.float32)) for r in closed] == g["sha256"].tolist()
    assert len(set(g["sha256"].tolist())) == 8                       # seven reports and the zeros
    assert not (tok == 1).any() and (tok[:, 0][b.n_tokens > 0] == 2).all()


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 9, 124, 125, 126, 127, 128, 200])
@pytest.mark.parametrize("L", [3, 5, 128])
def test_closed_form_equals_the_two_branches(n, L):
    ids = M.golden_ids(77, n)
    want = M.reference_ids(ids, L).numpy()
    got = M.closed_form_ids([0], [n], ids, L)[0]
    assert want.shape == (L,) and np.array_equal(got.astype(np.float32), want)


@pytest.mark.parametrize("seq,word", [
    ([4, 30000, 5], r"report \(7, 2\) holds the id 30000, outside \[0, 30000\)"),
    ([4, -1], r"report \(7, 2\) holds the id -1, outside"),
    ([4, 2.5], r"report \(7, 2\) holds a non-integer value"),
    ([4.0, 2.0], r"report \(7, 2\) holds a non-integer value"),
    (["12"], r"report \(7, 2\) holds a non-integer value"),
    ([[1, 2], [3, 4]], r"report \(7, 2\) has shape \(2, 2\)"),
])
def test_store_refuses_at_build_time_by_name(seq, word):
    with pytest.raises(ValueError, match=word):
        TokenReportStore.from_mapping({(1, 1): [1, 2, 3], (7, 2): seq})
    assert TokenReportStore.from_mapping({(1, 1): [1, 2, 3]}).n_tokens == 3


def test_store_refuses_other_bad_input():
    with pytest.raises(ValueError, match="max_length 2 < 3"):
        TokenReportStore.from_mapping({(1, 1): [1]}, max_length=2)
    assert TokenReportStore.from_mapping({(1, 1): [1]}, max_length=3).max_length == 3
    with pytest.raises(ValueError, match=r"holds the id 7, outside \[0, 7\)"):
        TokenReportStore.from_mapping({(1, 1): [7]}, vocab=7)
    with pytest.raises(ValueError, match=r"share the key \(1, 1\)"):
        TokenReportStore.from_mapping({(1, 1): [1], ("1", "1"): [2]})
    st = TokenReportStore.from_mapping({(1, 1): [1, 2]})
    with pytest.raises(ValueError, match=r"sample 1 names report 1, the store holds 0\.\.0"):
        st.plan(np.asarray([0, 1]))
    with pytest.raises(ValueError, match="integer"):
        st.plan(np.asarray([0.0]))


def test_from_mapping_copies_and_leaves_the_callers_lists_alone():
    """the reference's own read grows the list inside txtDict by a BOS and an EOS; the store reads a copy"""
    lists = {(3, 1): [5, 1, 7], (4, 1): [], (5, 1): np.asarray([9, 8], np.int16)}
    before = {k: list(v) for k, v in lists.items()}
    st = TokenReportStore.from_mapping(lists)
    lists[(3, 1)].append(11)                                          # a later change of the caller's list is not the store's
    assert st.ids.tolist() == [5, 1, 7, 9, 8] and st.tok_ptr.tolist() == [0, 3, 3, 5]
    lists[(3, 1)].pop()
    assert {k: list(v) for k, v in lists.items()} == before
    b = st.plan(np.asarray([0, 0, 1, 2]))
    first, second = M.plan_ids(b, st.ids.numpy()), M.plan_ids(b, st.ids.numpy())
    assert torch.equal(first, second) and first[0].tolist()[:6] == [2, 5, 0, 7, 3, 0]      # a second read equals the first


def test_synthetic_token_store():
    from medical_tri_modal_pilot_amd.synthetic import make_token_report_store
    st = make_token_report_store(11, n_reports=300)
    n = np.diff(st.tok_ptr)
    assert st.n_reports == 300 and n.min() == 0 and 126 < n.max() <= 160 and (n <= 125).any()
    assert st.index_of(17, 0) == 17 and int(st.ids.min()) >= 0 and int(st.ids.max()) < 30000
    assert torch.equal(make_token_report_store(11, n_reports=300).ids, st.ids)


NAMES = ("mtmp_report_ids_gather", "mtmp_token_embed_fwd", "mtmp_token_embed_bwd_workspace", "mtmp_token_embed_bwd_chunk",
         "mtmp_token_embed_bwd")


def test_new_entry_points_declared_listed_and_exported():
    from medical_tri_modal_pilot_amd import _lib
    from tests import abi
    for name in NAMES:
        ret, args = abi.declaration(name)
        restype, argtypes = _lib.SIGNATURES[name]
        assert ret in ("int", "long long")
        assert restype is (ctypes.c_int if ret == "int" else ctypes.c_longlong) and len(args) == len(argtypes)
        assert (restype, argtypes) == abi.ctypes_of(name)
    L = _lib.lib()
    assert all(getattr(L, n) for n in NAMES) and L.mtmp_abi_version() == 6
    mk = open(os.path.join(ROOT, "medical_tri_modal_pilot_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC\s*:=.*\btoken_embed\.hip\b", mk, re.M)


def test_workspace_and_chunk_queries():
    from medical_tri_modal_pilot_amd import _lib, ops
    L = _lib.lib()
    C = ops.token_embed_chunk()
    assert C == L.mtmp_token_embed_bwd_chunk() and C >= 2
    for T in (1, C, C + 1, 8192, 8193):
        nc = -(-T // C)
        want = -(-(4 * T + nc) // 4) * 16 + 2 * nc * 256 * 4         # four int32 [T], the counters, 16-byte pad, two partials a chunk
        assert L.mtmp_token_embed_bwd_workspace(T, 30000) == want
    assert L.mtmp_token_embed_bwd_workspace(0, 30000) == 0 and L.mtmp_token_embed_bwd_workspace(8192, 30000) < (1 << 20)


def test_entry_point_argument_errors():
    """every refusal returns before anything touches a GPU; the message is the thread's last error"""
    from medical_tri_modal_pilot_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    base = (ctypes.addressof(buf) + 15) & ~15
    p, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 8)

    def run(fn, defaults, over):
        a = dict(defaults)
        a.update(over)
        return getattr(L, fn)(*a.values()), L.mtmp_last_error().decode()
    gather = dict(ids=p, total=10, desc=p, out=p, B=2, L=128, stream=None)
    fwd = dict(ids=p, T=8, table=p, table_dtype=0, out=p, out_dtype=1, V=30000, D=256, stream=None)
    bwd = dict(ids=p, T=8, dy=p, dy_dtype=1, dw=p, workspace=p, V=30000, D=256, stream=None)
    cases = [("mtmp_report_ids_gather", gather, o, w) for o, w in (
                (dict(ids=None), "null pointer"), (dict(desc=None), "null pointer"), (dict(out=None), "null pointer"),
                (dict(L=2), "L >= 3"), (dict(B=0), "bad argument"), (dict(total=-1), "bad argument"), (dict(out=odd), "16-byte aligned"))]
    cases += [("mtmp_token_embed_fwd", fwd, o, w) for o, w in (
                (dict(ids=None), "null pointer"), (dict(table=None), "null pointer"), (dict(D=128), "D = 128"), (dict(D=768), "D = 768"),
                (dict(table_dtype=2), "dtype codes 2 -> 1"), (dict(T=0), "bad argument"), (dict(V=0), "bad argument"),
                (dict(out=odd), "16-byte aligned"))]
    cases += [("mtmp_token_embed_bwd", bwd, o, w) for o, w in (
                (dict(dw=None), "null pointer"), (dict(workspace=None), "null pointer"), (dict(D=255), "D = 255"),
                (dict(dy_dtype=3), "dtype code 3"), (dict(T=(1 << 24) + 1), "bad argument"), (dict(V=-1), "bad argument"),
                (dict(dw=odd), "16-byte aligned"))]
    for fn, defaults, over, word in cases:
        rc, msg = run(fn, defaults, over)
        assert rc != 0 and fn in msg and word in msg, (fn, over, rc, msg)


def test_ops_raise_without_a_device():
    from medical_tri_modal_pilot_amd import ops
    st = M.golden_store()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.report_token_ids(st.plan(np.asarray([0, 1])), "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.TokenEmbedFn.apply(torch.zeros(2, 3, dtype=torch.int32), torch.zeros(7, 256), torch.float32)
