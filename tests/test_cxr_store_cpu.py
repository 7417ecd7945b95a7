"""Host half of the image store (builder/data/cxr_store.py) and the plain-Python model of its two kernels
(tests/cxr_store_model.py) against PIL's own decodes (tests/golden/jpeg_cases.npz): what the store holds against plan_files on
the same files, the one-span-per-subsequence decode from the model's sync rows, the refusals, the 64-bit offsets, and
collate_raw_cxr fed handles against the same call fed the files' bytes.  All comparisons are exact."""
import ctypes
import os

import numpy as np
import pytest
import torch

from medical_tri_modal_pilot_amd.builder.data import cxr_store as CS
from medical_tri_modal_pilot_amd.builder.data import cxr_transform as CT
from medical_tri_modal_pilot_amd.builder.data import jpeg as J
from tests import abi
from tests import cxr_store_model as M
from tests import jpeg_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = jpeg_cases.names()


def test_store_holds_what_plan_files_gives():
    store = M.golden_store()
    plan, sizes = J.plan_files([jpeg_cases.file_of(n) for n in NAMES])
    desc, segs = plan.desc.numpy().astype(np.int64), plan.segs.numpy().astype(np.int64)
    assert store.n_images == len(NAMES) == 13 and store.names == NAMES
    same = [J.JPG_SEG0, J.JPG_NSEG, J.JPG_H, J.JPG_W, J.JPG_BPR, J.JPG_NBLK, J.JPG_QT, J.JPG_DC, J.JPG_AC, J.JPG_RI]
    assert np.array_equal(store.rows[:, same], desc[:, same])
    assert not store.rows[:, [J.JPG_STREAM, J.JPG_DST, J.JPG_COEF, 15]].any()
    assert np.array_equal(store.wide[:, CS.WIDE_STREAM], desc[:, J.JPG_STREAM]) and store.wide.dtype == np.int64
    img = segs[:, J.SEG_IMG]
    assert store.segs.shape == segs.shape and store.segs.shape[0] == int(desc[:, J.JPG_NSEG].sum())
    assert np.array_equal(store.segs[:, CS.TSEG_OFF], segs[:, J.SEG_OFF] - desc[img, J.JPG_STREAM])
    assert np.array_equal(store.segs[:, CS.TSEG_BYTES], segs[:, J.SEG_BYTES])
    assert np.array_equal(store.segs[:, CS.TSEG_BLOCK0], segs[:, J.SEG_BLOCK0])
    assert np.array_equal(store.tables, plan.tables.numpy()) and np.array_equal(store.streams, plan.streams.numpy())
    assert store.tables.size == 5 * 64 + 4 * J.HUFF_WORDS       # five qualities; the standard and one optimised table pair
    assert [(h.h, h.w) for h in map(store.image, range(13))] == sizes and store.image(5).store is store
    assert store.nbytes_streams == plan.streams.numel() and store.nbytes_sync == store.n_sync * 16
    assert store.nbytes == store.nbytes_streams + store.nbytes_sync + 4 * (store.segs.size + store.tables.size)
    with pytest.raises(IndexError):
        store.image(13)


@pytest.mark.parametrize("bits", M.SUBSEQ_BITS)
def test_subsequence_length_is_the_images_own(bits):
    """what JpegPlan.subseq_bits chooses for each image alone; sync rows per segment: ceil(bits / S), at least one"""
    store = M.golden_store(bits)
    for i, n in enumerate(NAMES):
        plan, _ = J.plan_files([jpeg_cases.file_of(n)])
        S = int(store.rows[i, CS.JPG_SUBSEQ])
        assert S == plan.subseq_bits(bits) and S % 32 == 0
        t = store.segs[store.rows[i, J.JPG_SEG0]:store.rows[i, J.JPG_SEG0] + store.rows[i, J.JPG_NSEG]].astype(np.int64)
        nsub = np.maximum(-(-(t[:, CS.TSEG_BYTES] * 8) // S), 1)
        assert nsub.max() <= J.MAX_SUBSEQ and int(nsub.sum()) == store.rows[i, CS.JPG_NSYNC]
        assert np.array_equal(t[:, CS.TSEG_SYNC0], np.cumsum(nsub) - nsub)
    assert np.array_equal(store.wide[:, CS.WIDE_SYNC0], np.cumsum(store.rows[:, CS.JPG_NSYNC]) - store.rows[:, CS.JPG_NSYNC])
    if bits == 32:
        assert sorted(set(store.rows[:, CS.JPG_SUBSEQ].tolist())) == [32, 64, 128]     # the two large files were raised
    with pytest.raises(ValueError, match="positive"):
        CS.CxrStore.from_files([jpeg_cases.file_of("1x1")], 0)


@pytest.mark.parametrize("bits", M.SUBSEQ_BITS)
def test_one_span_per_subsequence_from_the_sync_rows_equals_pil(bits):
    store = M.golden_store(bits)
    sync, status = M.golden_sync(bits)
    assert not status.any() and sync.shape == (store.n_sync, 4)
    first = store.wide[:, CS.WIDE_SYNC0]
    assert not sync[first, :3].any()                            # the first subsequence of a segment starts at state 0
    got = M.decode(store, sync, range(store.n_images))
    for g, n in zip(got, NAMES):
        want = jpeg_cases.pixels_of(n)
        print(f"store model[{n}, {bits}]: {int((g != want).sum())} of {want.size} pixels differ")
        assert np.array_equal(g, want)


def test_sync_rows_of_a_truncated_stream_set_the_status():
    store = CS.CxrStore.from_files([jpeg_cases.file_of("5x3"), jpeg_cases.truncated()], None, ["whole", "cut"])
    _, status = M.sync_rows(store)
    assert status.tolist() == [0, 1]


def _bad_files():
    g = jpeg_cases.golden()
    data = jpeg_cases.file_of("one_block")
    sof = data.index(b"\xff\xc0")
    return {"progressive": (g["bad.progressive"].tobytes(), NotImplementedError, "SOF2"),
            "rgb": (g["bad.rgb"].tobytes(), NotImplementedError, "components"),
            "12bit": (data[:sof + 4] + b"\x0c" + data[sof + 5:], NotImplementedError, "precision 12")}


@pytest.mark.parametrize("kind", ["progressive", "rgb", "12bit"])
def test_from_files_refuses_by_name(kind):
    data, exc, word = _bad_files()[kind]
    with pytest.raises(exc, match=r"file 1 \(study/b\.jpg\).*" + word):
        CS.CxrStore.from_files([jpeg_cases.file_of("5x3"), data], names=["study/a.jpg", "study/b.jpg"])


def test_handles_of_two_stores_in_one_batch_are_refused():
    a = M.golden_store()
    b = CS.CxrStore.from_files([jpeg_cases.file_of("5x3")])
    with pytest.raises(ValueError, match="sample 1 image 0.*one CxrStore"):
        CT.collate_raw_cxr([([a.image(1)], [-1.0]), ([b.image(0)], [-1.0])], CT.CxrTransform(32, "resize", True), 0)


def test_offsets_above_2_to_the_31_are_carried_exactly():
    """a host mirror of three images whose streams and sync rows lie behind 2^31 and 2^33"""
    rows = M.golden_store().rows[[4, 5, 6]].copy()
    rows[:, J.JPG_SEG0] = np.cumsum(rows[:, J.JPG_NSEG]) - rows[:, J.JPG_NSEG]
    wide = np.array([[5, 7], [2 ** 31 + 12345, 2 ** 31 + 99], [2 ** 33 + 1, 2 ** 32 + 5]], np.int64)
    segs = np.zeros((int(rows[:, J.JPG_NSEG].sum()), 4), np.int32)
    store = CS.CxrStore(None, rows, wide, segs, M.golden_store().tables, ["a", "b", "c"])
    assert store.n_sync == 2 ** 32 + 5 + int(rows[2, CS.JPG_NSYNC]) and store.nbytes_sync == store.n_sync * 16
    sb = store.batch([2, 1, 1, 0], pin=False)
    assert sb.wide.dtype == torch.int64 and sb.wide.tolist() == wide[[2, 1, 1, 0]].tolist()
    assert sb.desc[:, J.JPG_STREAM].tolist() == [0, 0, 0, 0] and sb.indices.tolist() == [2, 1, 1, 0]
    lanes = rows[[2, 1, 1, 0], CS.JPG_NSYNC]
    assert sb.prefix.tolist() == [0] + np.cumsum(lanes).tolist() and sb.lanes == int(lanes.sum())
    nblk = rows[[2, 1, 1, 0], J.JPG_NBLK]
    assert sb.desc[:, J.JPG_COEF].tolist() == (np.cumsum(nblk) - nblk).tolist()
    assert sb.total_blocks == int(nblk.sum()) and sb.max_blocks == int(nblk.max())
    moved = sb.to("cpu")
    assert torch.equal(moved.wide, sb.wide) and torch.equal(moved.desc, sb.desc) and torch.equal(moved.prefix, sb.prefix)
    assert sb.nbytes == 4 * (4 * 4 + 4 * 16 + 5)
    with pytest.raises(RuntimeError, match="host mirror"):
        store.to(torch.device("cuda", 0))


def _same_batch(a, b):
    for f in ("desc", "tables", "slot_map", "img_time"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    for f in ("image_size", "batch", "n_images", "scratch_bytes", "max_pixels", "max_rh", "max_rw", "lds_rows", "params", "stages",
              "pixel_bytes"):
        assert getattr(a, f) == getattr(b, f), f


@pytest.mark.parametrize("kind", ["resize_affine_crop", "randaug"])
def test_collate_on_handles_equals_collate_on_file_bytes(kind):
    store = M.golden_store()
    pick = [5, 0, 10, 5, 12, 3]                                # cxr_like twice, 1x1, the 98-segment file, the largest, 37x51
    K = 3
    mk_samples = lambda f: [([f(pick[0]), f(pick[1])], [-1.0, -2.5]), ([], []), ([f(pick[2]), f(pick[3]), f(pick[4])], [0.0, -4.0, -1.0]),
                            ([f(pick[5])], [-3.0])]
    kw = {}
    if kind == "randaug":
        tr = CT.CxrRandomTransform(32, kind)
        ops = [("Rotate", 12.0), ("Brightness", 0.3), ("ShearX", -0.1), ("Equalize", 0.0), ("Sharpness", 0.5), ("Identity", 0.0)]
        kw["aug_params"] = [(ops[i], ops[(i + 1) % 6]) for i in range(6)]
        hw = [jpeg_cases.pixels_of(NAMES[i]).shape for i in pick]
        kw["crop_params"] = [(0, 0, h, w) if i % 2 else (h // 8, w // 8, max(h // 2, 1), max(w // 2, 1)) for i, (h, w) in enumerate(hw)]
    else:
        tr = CT.CxrTransform(32, kind, True)
        kw["affine_params"] = [(3.0 - i, i, -i, 1.0 + 0.02 * i) for i in range(6)]
    got = CT.collate_raw_cxr(mk_samples(store.image), tr, K, **kw)
    want = CT.collate_raw_cxr(mk_samples(lambda i: jpeg_cases.file_of(NAMES[i])), tr, K, **kw)
    _same_batch(got, want)
    if kind == "randaug":
        assert torch.equal(got.aug, want.aug)
    assert got.jpeg is None and want.stored is None and got.pixels is None          # all stored: no host pixel buffer
    sb, jp = got.stored, want.jpeg
    assert sb.store is store and sb.indices.tolist() == pick and sb.images == jp.images == list(range(6))
    for c in (J.JPG_H, J.JPG_W, J.JPG_BPR, J.JPG_NBLK, J.JPG_DST, J.JPG_COEF, J.JPG_RI, J.JPG_NSEG):
        assert sb.desc[:, c].tolist() == jp.desc[:, c].tolist(), c
    assert sb.desc[:, J.JPG_DST].tolist() == got.desc[:, CT.DESC_SRC].tolist()
    assert (sb.total_blocks, sb.max_blocks) == (jp.total_blocks, jp.max_blocks)
    moved = got.to("cpu")
    assert moved.pixels.dtype == torch.uint8 and moved.pixels.numel() == got.pixel_bytes == want.pixels.numel()
    assert moved.stored.store is store and torch.equal(moved.stored.buf, sb.buf)


def test_collate_mixes_arrays_file_bytes_and_handles():
    store = M.golden_store()
    arr = jpeg_cases.pixels_of("rst_rows1")
    tr = CT.CxrTransform(32, "resize", True)
    raw = CT.collate_raw_cxr([([arr], [-1.0]), ([jpeg_cases.file_of("37x51_q30")], [-2.0]), ([store.image(4)], [-3.0]), ([], [])], tr, 0)
    plain = CT.collate_raw_cxr([([arr], [-1.0]), ([jpeg_cases.pixels_of("37x51_q30")], [-2.0]), ([jpeg_cases.pixels_of(NAMES[4])], [-3.0]),
                                ([], [])], tr, 0)
    _same_batch(raw, plain)
    assert plain.stored is None and plain.jpeg is None
    assert raw.jpeg.images == [1] and raw.stored.images == [2] and raw.stored.indices.tolist() == [4]
    assert raw.pixels is not None and torch.equal(raw.pixels[:arr.size], plain.pixels[:arr.size]) and not raw.pixels[arr.size:].any()
    assert int(raw.stored.desc[0, J.JPG_DST]) == arr.size + 37 * 51
    none = CT.collate_raw_cxr([([], []), ([], [])], tr, 0)
    assert none.stored is None and none.pixels is not None and none.to("cpu").stored is None


def test_new_entry_points_declared_listed_and_exported():
    from medical_tri_modal_pilot_amd import _lib
    from medical_tri_modal_pilot_amd.builder import data
    hdr = abi.header_text()
    L = _lib.lib()
    for name, nargs in (("mtmp_jpeg_sync_points", 12), ("mtmp_jpeg_store_entropy", 15)):
        ret, args = abi.declaration(name)
        restype, argtypes = _lib.SIGNATURES[name]
        assert ret == "int" and restype is ctypes.c_int and len(args) == len(argtypes) == nargs
        assert (restype, argtypes) == abi.ctypes_of(name)
        assert getattr(L, name)
    assert "int32 [n_sync][4]" in hdr and "int64 [n][2]" in hdr
    L.mtmp_abi_version.restype = ctypes.c_int
    assert L.mtmp_abi_version() == 6
    assert data.CxrStore is CS.CxrStore and data.image_wanted is CS.image_wanted


def test_store_ops_raise_without_a_device():
    from medical_tri_modal_pilot_amd import ops
    store = CS.CxrStore.from_files([jpeg_cases.file_of("one_block")])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cxr_store_decode(store, [0])
    raw = CT.collate_raw_cxr([([store.image(0)], [-1.0])], CT.CxrTransform(32, "resize", True), 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cxr_prepare(raw.to("cpu"))


# ---- which images a sample gets: CxrStore.select / image_wanted against the reference's own __getitem__ -----------------
def _select_golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "cxr_select_cases.npz")) as z:
        return {k: z[k] for k in z.files}


def test_select_and_image_wanted_equal_the_references_image_branch():
    """tests/golden/cxr_select_cases.npz (made by tests/golden/gen/make_golden_cxr_select.py): every case through
    image_wanted, CxrStore.select and collate_raw_cxr -- the chosen files in order, cxr_time as float32 bytes, the missing flag"""
    import types
    g = _select_golden()
    P, one = int(g["n_patients"]), jpeg_cases.file_of("1x1")
    patients = [[(g["file_time"][i], f"{int(g['file_rank'][i]):04d}", one) for i in np.flatnonzero(g["file_patient"] == p)]
                for p in range(P)]
    store = CS.CxrStore.from_patients(patients)
    assert store.n_images == g["file_time"].size == 17 and sorted(len(p) for p in patients if p) == [1, 1, 1, 4, 4, 6]
    tr = CT.CxrTransform(32, "resize", True)
    n_cases = g["patient"].size
    seen = set()
    for c in range(n_cases):
        pat, multi, comb, type_id, rt, full = (int(g[k][c]) for k in ("patient", "multi", "comb", "type_id", "realtime", "train_full"))
        args = types.SimpleNamespace(input_types=str(g["input_types"]), fullmodal_definition=str(g["fullmodal_definition"]),
                                     modality_inclusion="train-full_test-full" if full else "train-missing_test-missing")
        wanted = CS.image_wanted(args, type_id, comb, bool(patients[pat]))
        K = 3 if multi else 0
        pairs, missing = store.select([(pat, float(g["selected_key"][c]), float(g["t0"][c]), wanted)], K, rt, bool(full))
        raw = CT.collate_raw_cxr(pairs, tr, K)
        chosen = [h.index for h in pairs[0][0]]
        want = [int(v) for v in g["chosen"][c] if v >= 0]
        per = 3 if multi else 1
        assert chosen == want, (c, chosen, want)
        assert bool(missing[0]) == bool(g["missing"][c][1]) == (not want), c
        assert raw.img_time.numpy().astype(np.float32).tobytes() == g["cxr_time"][c][:per].tobytes(), (c, raw.img_time, g["cxr_time"][c])
        seen.add((multi, len(want), wanted))
    assert n_cases == 680 and {(0, 0, False), (0, 1, True), (1, 3, True), (1, 2, True), (1, 1, True), (1, 0, True)} <= seen


def test_select_refusals():
    one = jpeg_cases.file_of("1x1")
    store = CS.CxrStore.from_patients([[(5.0, "b", one), (5.0, "a", one), (-3.0, "c", one)], []])
    pairs, missing = store.select([(0, 5.0, 1.0, True), (0, -4.0, 0.0, True), (1, 9.0, 9.0, True), (0, 9.0, 2.0, False)], 0, 0)
    assert [[h.index for h in hs] for hs, _ in pairs] == [[0], [], [], []] and missing.tolist() == [False, True, True, True]
    assert pairs[0][1] == [4.0]                                 # (5.0, "b") is the last of sorted(); realtime 0: minus t0
    pairs, _ = store.select([(0, 5.0, 1.0, True)], 3, 0)
    assert [h.index for h in pairs[0][0]] == [2, 1, 0] and pairs[0][1] == [-8.0, 0.0, 0.0]
    with pytest.raises(ValueError, match="sample 1 .*patient 0.*train-full"):
        store.select([(0, 5.0, 5.0, True), (0, -4.0, -4.0, True)], 0, 1, train_full=True)
    with pytest.raises(ValueError, match="patient 2"):
        store.select([(2, 5.0, 5.0, True)], 0, 1)
    with pytest.raises(RuntimeError, match="patient table"):
        M.golden_store().select([(0, 5.0, 5.0, True)], 0, 1)
