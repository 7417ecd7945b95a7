"""The device-resident report store on the CPU (builder/data/report_store.py): the gate and the host plan against the reference
``__getitem__`` goldens (tests/golden/report_cases.npz), the model of the gather (tests/report_store_model.py) against their
digests, the refusals, the bfloat16 bits, and the new entry point's declaration and argument errors (the library loads without
a GPU)."""
import ctypes
import itertools
import os
import re
import types

import numpy as np
import pytest
import torch

from medical_tri_modal_pilot_amd.builder.data import ReportBatch, ReportStore, report_wanted
from tests import report_store_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_report_wanted_truth_table():
    """every combination of the flag values the gate reads, against the reference's expression spelled out term by term"""
    n = 0
    for it, fd, mi, fn in itertools.product(("vslt", "vslt_txt", "vslt_img", "vslt_img_txt"), ("txt1_img1", "txt1", "img1"),
                                            ("train-full_test-full", "train-missing_test-missing", "train-full_test-missing",
                                             "train-missing_test-full"),
                                            ("1_2_txt1_img0.pkl", "1_2_txt0_img1.pkl", "1_2_txt1_img1.pkl", "1_2_txt0_img0.pkl")):
        has_txt, def_txt = it in ("vslt_txt", "vslt_img_txt"), fd in ("txt1_img1", "txt1")
        test_full, test_missing = mi.endswith("test-full"), mi.endswith("test-missing")
        want = ((has_txt and def_txt and test_full) or (test_missing and has_txt)) and fn.split("_")[2] == "txt1"
        got = report_wanted(types.SimpleNamespace(input_types=it, fullmodal_definition=fd, modality_inclusion=mi), fn)
        assert got is want, (it, fd, mi, fn)
        n += 1
    assert n == 192
    a = types.SimpleNamespace(input_types="vslt_img_txt", fullmodal_definition="img1", modality_inclusion="train-full_test-full")
    assert report_wanted(a, "x_txt1.pkl") is False               # test-full needs txt1 in the definition ...
    a.modality_inclusion = "train-full_test-missing"
    assert report_wanted(a, "x_txt1.pkl") is True                # ... test-missing does not


def test_store_of_the_golden_reports():
    g, st = M.golden(), M.golden_store()
    assert st.n_reports == 7 and st.n_tokens == sum(M.GOLDEN_LENGTHS) == int(g["report_len"].sum())
    assert st.tok_ptr.dtype == np.int64 and st.tok_ptr.tolist() == np.concatenate([[0], np.cumsum(g["report_len"])]).tolist()
    assert st.emb.dtype == torch.float32 and tuple(st.emb.shape) == (st.n_tokens, 768) and st.nbytes == st.n_tokens * 3072
    assert (st.width, st.max_tokens, st.device.type) == (768, 128, "cpu") and st.to("cpu") is st
    for k, f in enumerate(g["report_file"]):
        assert st.index_of(str(int(f))) == st.index_of(f"  {int(f)}\n") == k
    assert st.index_of("") == st.index_of("   ") == st.index_of("no such report") == -1
    assert sorted(set(g["text_length"].tolist())) == [0, 1, 2, 5, 37, 64, 127, 128] and len(g["case_file"]) == 40


def test_plan_on_the_golden_cases():
    g, st = M.golden(), M.golden_store()
    idx = M.golden_report_idx(st)
    assert (idx >= 0).sum() == 28 and (idx < 0).sum() == 12          # seven txt1 files, three txt0 files, four combinations each
    b = st.plan(idx, g["case_comb"])
    assert isinstance(b, ReportBatch) and b.batch_size == 40 and b.store is st and (b.max_tokens, b.width) == (128, 768)
    assert b.txt_lengths.dtype == torch.int64 and b.txt_lengths.tolist() == g["text_length"].tolist()
    assert b.missing.dtype == torch.float32 and b.missing.tolist() == g["missing"][:, 2].tolist()
    assert b.n_tokens.tolist() == g["text_length"].tolist() and (b.first_token[b.n_tokens == 0] == 0).all()
    d = b.descriptor()
    assert d.dtype == torch.int64 and tuple(d.shape) == (40, 2) and d.is_contiguous()
    for lo in range(0, 40, 10):                                      # the batches of ten the GPU test gathers
        bb = st.plan(idx[lo:lo + 10], g["case_comb"][lo:lo + 10])
        assert bb.txt_lengths.tolist() == g["text_length"][lo:lo + 10].tolist()
    one = st.plan(idx[:8], 3)                                        # one combination for the whole batch
    assert one.txt_lengths.tolist() == [0] * 8 and one.missing.tolist() == [1.0] * 8
    assert st.plan(idx[:8]).txt_lengths.tolist() == [int(st.tok_ptr[i + 1] - st.tok_ptr[i]) if i >= 0 else 0 for i in idx[:8]]


def test_model_reproduces_the_golden_digests():
    g, st = M.golden(), M.golden_store()
    b = st.plan(M.golden_report_idx(st), g["case_comb"])
    tok = M.plan_tokens(b, st.emb)
    assert tok.dtype == torch.float32 and tuple(tok.shape) == (40, 128, 768)
    assert [M.digest(t) for t in tok] == g["sha256"].tolist()
    assert len(set(g["sha256"].tolist())) == 8                       # seven reports and the zeros


def test_a_report_without_tokens_is_missing():
    st = ReportStore.from_mapping(M.synthetic_mapping())
    assert st.index_of("note 0") == 0 and st.index_of(" note 3 ") == 3 and int(st.tok_ptr[1]) == 0
    b = st.plan(np.asarray([0, 1, 2, 3, -1]))
    assert b.txt_lengths.tolist() == [0, 1, 37, 128, 0] and b.missing.tolist() == [1.0, 0.0, 0.0, 0.0, 1.0]
    b = st.plan(np.asarray([1, 1, 1, 1]), np.asarray([0, 1, 2, 3]))
    assert b.txt_lengths.tolist() == [1, 0, 1, 0] and b.missing.tolist() == [0.0, 1.0, 0.0, 1.0]


@pytest.mark.parametrize("entry,exc,word", [
    (np.zeros((129, 768)), ValueError, r"report 1 \('long'\) has 129 tokens, more than max_tokens 128"),
    (np.zeros(768), NotImplementedError, r"report 1 \('long'\) is a 1-D CLS vector of 768 values"),
    (np.zeros((4, 760)), ValueError, r"report 1 \('long'\) has shape \(4, 760\), want \[tokens, 768\]"),
    (np.zeros((2, 3, 768)), ValueError, r"has shape \(2, 3, 768\)"),
    (np.full((4, 768), np.nan), ValueError, r"report 1 \('long'\) holds a non-finite value"),
    (np.full((4, 768), np.inf), ValueError, "non-finite"),
    (np.full((4, 768), 1e39), ValueError, "non-finite"),              # finite in float64, inf once rounded to float32
])
def test_store_refuses_at_build_time_by_name(entry, exc, word):
    good = {"embedding": np.ones((3, 768))}
    with pytest.raises(exc, match=word):
        ReportStore.from_mapping({"fine": good, "long": {"embedding": entry}})
    assert ReportStore.from_mapping({"fine": good}).n_tokens == 3


def test_store_refuses_other_bad_input():
    good = {"embedding": np.ones((3, 40))}
    with pytest.raises(ValueError, match="width 44 is not a positive multiple of 8"):
        ReportStore.from_mapping({"a": good}, width=44)
    with pytest.raises(ValueError, match="share the key 'a'"):
        ReportStore.from_mapping({"a": good, " a ": good}, width=40)
    st = ReportStore.from_mapping({"a": good, "  ": good}, width=40, max_tokens=3)       # an unreachable key is left out
    assert st.n_reports == 1 and (st.width, st.max_tokens) == (40, 3)
    with pytest.raises(ValueError, match=r"sample 1 names report 1, the store holds 0\.\.0"):
        st.plan(np.asarray([0, 1]))
    with pytest.raises(ValueError, match="integer"):
        st.plan(np.asarray([0.0]))
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        st.to("cpu", torch.float16)


def test_values_are_rounded_to_float32_once_and_bfloat16_by_torch():
    x64 = np.concatenate([M.rounding_values().astype(np.float64), [1.0 + 2.0 ** -30, 1.0 / 3.0, 1e-45, 3.0e38]])
    x64 = np.resize(x64, (3, 48))
    st = ReportStore.from_mapping({"r": {"embedding": x64}}, width=48)
    want32 = torch.Tensor(x64)                                       # the reference's rounding
    assert st.emb.numpy().tobytes() == want32.numpy().tobytes()
    st2 = st.to("cpu", torch.bfloat16)
    assert st2 is st and st.dtype == torch.bfloat16 and st.nbytes == 3 * 48 * 2
    assert st.emb.view(torch.int16).numpy().tobytes() == want32.to(torch.bfloat16).view(torch.int16).numpy().tobytes()
    with pytest.raises(RuntimeError, match="keeps no float32 host copy"):
        st.to("cpu", torch.float32)
    # the integer rule the kernel applies is torch's conversion, on the values the GPU rounding test stores
    r = M.rounding_values()
    assert M.bf16_bits_rne(r).tobytes() == torch.from_numpy(r.copy()).to(torch.bfloat16).view(torch.int16).numpy().tobytes()
    assert np.isinf(torch.from_numpy(r.copy()).to(torch.bfloat16).float().numpy()).sum() == 4      # +-max and +-0x7F7F8000
    full = M.golden_store()
    per_token = full.nbytes // full.n_tokens
    assert per_token == 3072 and full.to("cpu", torch.bfloat16).nbytes // full.n_tokens == 1536


def test_synthetic_report_store():
    from medical_tri_modal_pilot_amd.synthetic import make_report_store
    st = make_report_store(11, n_reports=40)
    n = np.diff(st.tok_ptr)
    assert st.n_reports == 40 and n[0] == 1 and n[1] == 128 and n[2:].min() >= 1 and n[2:].max() <= 126
    assert st.index_of("report 17") == 17 and st.emb.dtype == torch.float32 and torch.isfinite(st.emb).all()
    assert torch.equal(make_report_store(11, n_reports=40).emb, st.emb)


def test_new_entry_point_declared_listed_and_exported():
    from medical_tri_modal_pilot_amd import _lib
    from medical_tri_modal_pilot_amd.builder.data import report_store as RS
    from tests import abi
    hdr = abi.header_text()
    ret, args = abi.declaration("mtmp_report_gather")
    restype, argtypes = _lib.SIGNATURES["mtmp_report_gather"]
    assert ret == "int" and restype is ctypes.c_int and len(args) == len(argtypes) == 10
    assert (restype, argtypes) == abi.ctypes_of("mtmp_report_gather")
    L = _lib.lib()
    assert L.mtmp_report_gather and L.mtmp_abi_version() == 6
    assert "int64 [B][2]" in hdr and RS.DESC_WORDS == 2
    mk = open(os.path.join(ROOT, "medical_tri_modal_pilot_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC\s*:=.*\breport_store\.hip\b", mk, re.M)


def test_entry_point_argument_errors():
    """every refusal returns before anything touches a GPU; the message is the thread's last error"""
    from medical_tri_modal_pilot_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    base = (ctypes.addressof(buf) + 15) & ~15
    p = ctypes.c_void_p(base)

    def call(**over):
        a = dict(emb=p, emb_dtype=0, total_tokens=10, desc=p, out=p, out_dtype=1, B=2, L=128, W=768, stream=None)
        a.update(over)
        rc = L.mtmp_report_gather(*a.values())
        return rc, L.mtmp_last_error().decode()
    for over, word in ((dict(emb=None), "null pointer"), (dict(desc=None), "null pointer"), (dict(out=None), "null pointer"),
                       (dict(W=772), "width 772 is not a positive multiple of 8"), (dict(W=0), "width 0"), (dict(W=-8), "width -8"),
                       (dict(emb_dtype=2), "dtype codes 2 -> 1"), (dict(out_dtype=-1), "dtype codes 0 -> -1"),
                       (dict(B=0), "bad argument"), (dict(B=-3), "bad argument"), (dict(L=0), "bad argument"),
                       (dict(L=1 << 17), "bad argument"), (dict(total_tokens=-1), "bad argument"),
                       (dict(B=1 << 20, L=1 << 16, W=1 << 20), "workgroups of 256 lanes are more than a grid holds"),
                       (dict(out=ctypes.c_void_p(base + 8)), "16-byte aligned"), (dict(emb=ctypes.c_void_p(base + 4)), "16-byte aligned")):
        rc, msg = call(**over)
        assert rc != 0 and "mtmp_report_gather" in msg and word in msg, (over, rc, msg)


def test_report_tokens_raises_without_a_device():
    from medical_tri_modal_pilot_amd import ops
    st = M.golden_store()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.report_tokens(st.plan(np.asarray([0, 1])), "cpu", torch.float32)
