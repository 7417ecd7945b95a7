"""The device-resident event store on the CPU (builder/data/tie_store.py): the store and its host plan against the reference
``__getitem__`` goldens (tests/golden/tie_windows.npz), the NumPy model of the gather kernel (tests/tie_store_model.py) bit for
bit against ``seq_cat`` and, on synthetic patients that cover what the fixture is thin in, against ``tie_window``; the window
draws; the refusals; the new entry point's declaration and argument errors (the library loads without a GPU)."""
import collections
import ctypes
import os
import pickle
import random
import re

import numpy as np
import pytest
import torch

from medical_tri_modal_pilot_amd.builder.data import (SampleTieDataset, StoreWindowDataset, TieEventStore, TieWindowBatch,
                                                       collate_windows)
from tests import tie_store_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_store_of_the_golden_patients():
    g, st = M.golden(), M.golden_store()
    P = len(g["files"])
    lens = [g[f"p{i}.dit_len"] for i in range(P)]
    assert st.n_patients == P and st.hour_ptr.tolist() == np.concatenate([[0], np.cumsum([len(x) for x in lens])]).tolist()
    assert st.hour_ptr.dtype == st.ev_ptr.dtype == np.int64 and st.ev_time.dtype == torch.float64
    assert (np.diff(st.hour_ptr) > 0).all() and (np.diff(st.ev_ptr) >= 0).all() and st.ev_ptr[0] == 0
    assert st.ev_ptr.shape == (st.n_hours + 1,) and st.n_events == sum(int(x[x > 0].sum()) for x in lens) == st.ev_time.numel()
    assert np.array_equal(st.present, np.concatenate(lens) >= 0)
    assert np.array_equal(np.diff(st.ev_ptr), np.maximum(np.concatenate(lens), 0))
    assert st.static.shape == (P, 2) and st.static[:, 0].tolist() == [float(g[f"p{i}.male"]) for i in range(P)]
    assert st.nbytes == st.n_hours * (18 * 12 + 8) + st.n_events * 13
    assert np.isinf(st.hour_min[~st.present]).all() and np.isfinite(st.hour_min[np.diff(st.ev_ptr) > 0]).all()
    assert st.to("cpu") is st


def test_plan_on_the_golden_cases():
    g, st = M.golden(), M.golden_store()
    seen = 0
    for rt, tl, sel in M.golden_groups():
        b = st.plan(g["case"][sel][:, 2:5], tl, rt)
        assert isinstance(b, TieWindowBatch) and b.batch_size == len(sel) and b.store is st
        assert b.input_lengths.tolist() == g["len"][sel].tolist() and b.max_len == int(g["len"][sel].max())
        assert b.cu_seqlens.dtype == torch.int32 and b.cu_seqlens.tolist() == np.concatenate([[0], np.cumsum(g["len"][sel])]).tolist()
        if rt == 1:                                   # the reference returns -selectedKey' as txt_time
            assert b.txt_time.tolist() == g["ttime"][sel].tolist()
            assert (-b.selected_key).tolist() == g["ttime"][sel].tolist()
        assert torch.equal(b.static, torch.from_numpy(g["static"][sel]))
        seen += len(sel)
    assert seen == len(g["case"]) == 440


def test_kernel_model_reproduces_the_golden_sequences():
    g, st, off = M.golden(), M.golden_store(), M.golden_offsets()
    for rt, tl, sel in M.golden_groups():
        rows = M.model_rows(st, st.plan(g["case"][sel][:, 2:5], tl, rt))
        for c, got in zip(sel, rows):
            want = g["seq_cat"][off[c]:off[c] + int(g["len"][c])]
            assert got.dtype == np.float32 and got.tobytes() == np.ascontiguousarray(want).tobytes(), (rt, tl, int(c))


def test_the_golden_fixture_is_thin_where_the_synthetic_patients_are_not():
    g, pats = M.golden(), M.golden_patients()
    head = tail = 0
    for rt, tl, i, key, L in g["case"]:
        tdl = pats[i]["data_in_time"][key - L + 1:key + 1]
        head += tdl[0] is None
        tail += tdl[0] is not None and tdl[-1] is None
    assert (head, tail) == (2, 2)
    assert not any(a is not None and len(a) == 0 for p in pats for a in p["data_in_time"])
    assert int(g["case"][:, 1].min()) == 40
    assert int(g["len"].max()) == 172                 # rows of the longest window (initial rows + events)
    assert max(sum(len(a) for a in pats[i]["data_in_time"][key - L + 1:key + 1] if a is not None)
               for _, _, i, key, L in g["case"]) == 159


def test_synthetic_patients_against_tie_window():
    """plan + kernel model == tie_window, bit for bit, on None hours at either and both ends, empty present hours, windows over
    1000 events, tie_len cutting inside the initial rows and inside the events, empty and full initial blocks; with the coverage
    counted.  train_missing False on the late-trimmed windows as well."""
    pats, st, wins = M.synthetic_patients(), M.synthetic_store(), M.synthetic_windows()
    cover = collections.Counter()
    for rt, tl in M.SYNTHETIC_CONFIGS:
        b = st.plan(wins, tl, rt)
        rows = M.model_rows(st, b)
        for (p, key, L), got, n, key2 in zip(wins.tolist(), rows, b.input_lengths.tolist(), b.selected_key.tolist()):
            want, n_ref, key_ref = M.reference_window(pats, M.FMIN, M.FMAX, p, key, L, tl, rt)
            assert (n, key2) == (n_ref, key_ref), (rt, tl, p, key, L)
            assert got.tobytes() == want.tobytes(), (rt, tl, p, key, L)
            if rt == 1:
                cover.update(M.kinds_of(pats, p, key, L, tl))
    kinds = ("none_head", "none_tail", "none_both", "empty_present_hour", "over_1000_events", "no_initial_row",
             "all_18_initial_rows", "cut_inside_initial_rows", "cut_inside_events")
    print("synthetic coverage:", {k: cover[k] for k in kinds})
    assert all(cover[k] >= 5 for k in kinds), cover
    late = np.asarray([w for w in wins.tolist() if "none_tail" in M.kinds_of(pats, *w, 1000)], np.int64)
    b = st.plan(late, 1000, 1, train_missing=False)
    assert b.selected_key.tolist() == late[:, 1].tolist()          # the prediction hour does not move ...
    for (p, key, L), got in zip(late.tolist(), M.model_rows(st, b)):
        want, _, _ = M.reference_window(pats, M.FMIN, M.FMAX, p, key, L, 1000, 1, train_missing=False)
        assert got.tobytes() == want.tobytes(), (p, key, L)       # ... and t0 follows it
    # the fp16 rounding of the hand-over, as PackedTieBatch.on_device applies it
    b = st.plan(wins[:40], 1000, 1)
    for got, raw in zip(M.model_rows(st, b, round_fp16=True), M.model_rows(st, b)):
        assert torch.equal(torch.from_numpy(got), torch.from_numpy(raw).half().float())


def test_chunk_case_is_a_few_rows_past_a_chunk_boundary():
    st = M.synthetic_store()
    b = st.plan(np.asarray([M.CHUNK_CASE["window"]]), M.CHUNK_CASE["tie_len"], 1)
    assert int(b.n_events[0]) > 1000 and b.max_len == M.CHUNK_CASE["tie_len"] == 4 * M.CHUNK_ROWS + 6
    hip = open(os.path.join(ROOT, "medical_tri_modal_pilot_amd", "csrc", "tie_store.hip")).read()
    assert re.search(r"CHUNK_ROWS\s*=\s*%d\b" % M.CHUNK_ROWS, hip)


def test_store_window_dataset_draws_the_windows_of_sample_tie_dataset(tmp_path):
    g, pats = M.golden(), M.golden_patients()
    for i, p in enumerate(pats[:3]):
        with open(tmp_path / f"{i:03d}_txt0_img0.pkl", "wb") as fh:
            pickle.dump(p, fh)
    ds = SampleTieDataset(str(tmp_path), g["feature_mins"], g["feature_maxs"], tie_len=1000, realtime=1)
    st = TieEventStore.from_directory(str(tmp_path), g["feature_mins"], g["feature_maxs"])
    assert st.n_patients == 3 and st.names == sorted(os.listdir(tmp_path))
    wd = StoreWindowDataset(st)
    assert len(wd) == len(ds) == 3
    random.seed(4)
    items = [ds[i % 3] for i in range(12)]
    random.seed(4)
    triples = [wd[i % 3] for i in range(12)]
    batch = collate_windows(triples, st, tie_len=1000, realtime=1)
    for (ev, static, ttime), got, b in zip(items, M.model_rows(st, batch), range(12)):
        assert got.tobytes() == ev.tobytes() and float(batch.txt_time[b]) == ttime
        assert batch.static[b].tolist() == static.tolist()
    assert batch.windows[:, 0].tolist() == [i % 3 for i in range(12)]


@pytest.mark.parametrize("window,word", [((3, 0, 1), "patient"), ((-1, 0, 1), "patient"), ((0, 14, 1), "hour"), ((0, -1, 1), "hour"),
                                         ((0, 3, 5), r"rand_length > selected_key \+ 1"), ((0, 3, 0), "rand_length < 1"),
                                         (M.ALL_NONE_WINDOW, "all None"), (M.ZERO_ROW_WINDOW, "no row")])
def test_plan_refuses_and_names_the_window(window, word):
    st = M.synthetic_store()
    good = (1, 5, 3)
    with pytest.raises(ValueError, match=r"window 1 \(patient %d, selected_key %d, rand_length %d\).*%s" % (*window, word)):
        st.plan(np.asarray([good, window, good]), 1000, 1)
    assert st.plan(np.asarray([good]), 1000, 1).batch_size == 1
    with pytest.raises(ValueError, match="integer"):
        st.plan(np.asarray([[0.0, 1.0, 1.0]]), 1000, 1)


def test_store_refuses_non_finite_event_times_and_odd_feature_indices():
    pats = [dict(p) for p in M.synthetic_patients()[:1]]
    dit = [None if a is None else a.copy() for a in pats[0]["data_in_time"]]
    dit[3][1, 0] = np.inf
    with pytest.raises(ValueError, match="patient who.*hour 3.*non-finite"):
        TieEventStore.from_patients([dict(pats[0], data_in_time=dit)], M.FMIN, M.FMAX, ["who"])
    dit[3][1, 0] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        TieEventStore.from_patients([dict(pats[0], data_in_time=dit)], M.FMIN, M.FMAX)
    dit[3][1, 0], dit[3][2, 2] = 3.5, 2.5
    with pytest.raises(ValueError, match="feature index"):
        TieEventStore.from_patients([dict(pats[0], data_in_time=dit)], M.FMIN, M.FMAX)


def test_new_entry_point_declared_listed_and_exported():
    from medical_tri_modal_pilot_amd import _lib
    from tests import abi
    hdr = abi.header_text()
    ret, args = abi.declaration("mtmp_tie_window_gather")
    restype, argtypes = _lib.SIGNATURES["mtmp_tie_window_gather"]
    assert ret == "int" and restype is ctypes.c_int and len(args) == len(argtypes) == 20
    assert (restype, argtypes) == abi.ctypes_of("mtmp_tie_window_gather")
    L = _lib.lib()
    assert L.mtmp_tie_window_gather and L.mtmp_abi_version() == 6
    from medical_tri_modal_pilot_amd.builder.data import tie_store as TS
    assert "int64 [B][8]" in hdr and TS.DESC_WORDS == 8


def test_entry_point_argument_errors():
    """every refusal returns before anything touches a GPU; the message is the thread's last error"""
    from medical_tri_modal_pilot_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))

    def call(**over):
        a = dict(ev_time=p, ev_val=p, ev_feat=p, norm=p, delta=p, hour_min=p, n_events=10, n_hours=4, desc=p, cu=p, out=p, B=2,
                 max_len=5, t_pad=8, total_rows=7, out_rows=16, padded=0, realtime=1, round_fp16=1, stream=None)
        a.update(over)
        rc = L.mtmp_tie_window_gather(*a.values())
        return rc, L.mtmp_last_error().decode()
    for over, word in ((dict(B=0), "bad argument"), (dict(B=-3), "bad argument"), (dict(out=None), "null pointer"),
                       (dict(desc=None), "null pointer"), (dict(cu=None), "null pointer"), (dict(ev_time=None), "null pointer"),
                       (dict(norm=None), "null pointer"), (dict(padded=1, t_pad=4), "t_pad 4 is smaller"),
                       (dict(out_rows=6), "holds 6 rows, the batch has 7"), (dict(total_rows=11), "bad argument"),
                       (dict(max_len=0), "bad argument")):
        rc, msg = call(**over)
        assert rc != 0 and "mtmp_tie_window_gather" in msg and word in msg, (over, rc, msg)


def test_tie_windows_raises_on_a_host_store():
    from medical_tri_modal_pilot_amd import ops
    st = M.synthetic_store()
    with pytest.raises(RuntimeError, match="no CPU fallback|store.to"):
        ops.tie_windows(st.plan(np.asarray([(1, 5, 3)]), 1000, 1), "cpu", 64)
