"""Host half of the JPEG decoder (builder/data/jpeg.py) and the NumPy model of its kernels (tests/jpeg_model.py) against PIL's
own decodes (tests/golden/jpeg_cases.npz): the parser on every case and on what it must refuse, the model for every
subsequence length, a truncated stream, and collate_raw_cxr with file bytes in the batch."""
import ctypes

import numpy as np
import pytest
import torch

from medical_tri_modal_pilot_amd.builder.data import cxr_transform as CT
from medical_tri_modal_pilot_amd.builder.data import jpeg as J
from tests import jpeg_cases, jpeg_model

STD_DC = (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0)                 # Annex K.3, luminance
STD_AC = (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125)
# restart interval, segments
RESTARTS = {"rst_blocks1": (1, 6), "rst_blocks8": (8, 98), "rst_rows1": (6, 5)}


@pytest.mark.parametrize("name", jpeg_cases.names())
def test_parse_jpeg(name):
    data, pix = jpeg_cases.file_of(name), jpeg_cases.pixels_of(name)
    info = J.parse_jpeg(data)
    assert (info.h, info.w) == pix.shape
    ri, nseg = RESTARTS.get(name, (0, 1))
    assert info.restart_interval == ri and len(info.segments) == len(info.stream_segments) == nseg
    std = (info.dc.bits, info.ac.bits) == (STD_DC, STD_AC)
    assert std == (name != "smooth_opt") and len(info.dc.vals) == sum(info.dc.bits) and len(info.ac.vals) == sum(info.ac.bits)
    if std:
        assert info.dc.vals == tuple(range(12)) and info.ac.vals[:6] == (1, 2, 3, 0, 4, 17) and len(info.ac.vals) == 162
    assert info.qtable.shape == (64,) and info.qtable.dtype == np.int32
    if name.endswith("q100"):
        assert (info.qtable == 1).all()
    if name in ("one_block", "cxr_like"):              # quality 75 of the Annex K.1 table, rows 0 and 1 in natural order
        assert info.qtable[:3].tolist() == [8, 6, 5] and info.qtable[8:11].tolist() == [6, 6, 7]
    assert data[info.ecs_offset + info.ecs_length:] == b"\xff\xd9"
    raw = np.frombuffer(data, np.uint8)
    stuffed = 0
    for (off, length), (soff, slen) in zip(info.segments, info.stream_segments):
        seg = raw[off:off + length].tobytes()
        assert seg.replace(b"\xff\x00", b"\xff") == info.stream[soff:soff + slen].tobytes()
        stuffed += length - slen
    assert info.stream.size == info.ecs_length - stuffed - 2 * (nseg - 1)
    if name == "noise_q100":
        assert stuffed > 10
    for k in range(1, nseg):                            # RSTn between the segments, n counting modulo 8
        off = int(info.segments[k][0])
        assert raw[off - 2] == 0xFF and raw[off - 1] == 0xD0 + (k - 1) % 8


@pytest.mark.parametrize("bad,exc,word", [("progressive", NotImplementedError, "SOF2"), ("rgb", NotImplementedError, "SOF0"),
                                          ("cut", ValueError, "DHT")])
def test_parse_jpeg_refuses_by_name(bad, exc, word):
    data = jpeg_cases.golden()[f"bad.{bad}"].tobytes()
    with pytest.raises(exc, match=word):
        J.parse_jpeg(data)
    with pytest.raises(exc, match="sample 0 image 1.*" + word):          # no silent fallback in the collate either
        CT.collate_raw_cxr([([jpeg_cases.pixels_of("5x3"), data], [-1.0, -2.0])], CT.CxrTransform(32, "resize", True), 3)


def test_parse_jpeg_refuses_other_input():
    with pytest.raises(ValueError, match="SOI"):
        J.parse_jpeg(b"\x89PNG\r\n\x1a\n")
    data = jpeg_cases.file_of("one_block")
    with pytest.raises(ValueError, match="truncated"):
        J.parse_jpeg(data[:J.parse_jpeg(data).ecs_offset - 3])             # inside the SOS header
    sof = data.index(b"\xff\xc0")
    with pytest.raises(NotImplementedError, match="precision 12"):
        J.parse_jpeg(data[:sof + 4] + b"\x0c" + data[sof + 5:])
    with pytest.raises(ValueError, match="DQT table"):
        J.parse_jpeg(data[:sof + 12] + b"\x03" + data[sof + 13:])          # SOF0 names a quantisation table that is not there


@pytest.mark.parametrize("name", jpeg_cases.names())
def test_model_equals_pil(name):
    data, want = jpeg_cases.file_of(name), jpeg_cases.pixels_of(name)
    for bits in jpeg_cases.SUBSEQ_BITS:
        (got,), status, rounds = jpeg_model.decode_files([data], bits)
        print(f"jpeg model[{name}, {bits} bits]: {int((got != want).sum())} of {want.size} pixels differ, status {status.tolist()}, "
              f"rounds {max(rounds)}")
        assert status.tolist() == [0] and np.array_equal(got, want)
        if bits == 0:
            assert max(rounds) == 1
        if bits == 128 and name in ("noise_q100", "cxr_like", "100x9_q100"):
            assert max(rounds) > 1                      # several subsequences: the lanes had to synchronise


def test_model_choice_of_subsequence_length():
    plan, _ = J.plan_files([jpeg_cases.file_of("noise_q100")])
    assert plan.subseq_bits(None) == J.DEFAULT_SUBSEQ_BITS and plan.subseq_bits(0) == 0 and plan.subseq_bits(100) == 128
    plan.max_seg_bytes = 1 << 20                        # a megabyte segment: 8192 bits per lane fill the 1,024 lanes
    assert plan.subseq_bits(None) == plan.subseq_bits(128) == 8192


def test_model_on_a_truncated_stream():
    """half of the entropy-coded data is missing: the span function runs to the end of what is there, the image's status is set
    and it is written as zeros; its neighbour is untouched"""
    cut, other = jpeg_cases.truncated(), jpeg_cases.file_of("37x51_q30")
    info = J.parse_jpeg(cut)
    assert (info.h, info.w) == (64, 64) and len(cut) < len(jpeg_cases.file_of("noise_q100")) * 0.6
    for bits in jpeg_cases.SUBSEQ_BITS:
        (a, b), status, _ = jpeg_model.decode_files([cut, other], bits)
        assert status[0] & jpeg_model.STATUS_SHORT and status[1] == 0
        assert not a.any() and np.array_equal(b, jpeg_cases.pixels_of("37x51_q30"))


def _same_batch(a, b, pixels: bool):
    for f in ("desc", "tables", "slot_map", "img_time") + (("pixels",) if pixels else ()):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    for f in ("image_size", "batch", "n_images", "scratch_bytes", "max_pixels", "max_rh", "max_rw", "lds_rows", "params", "stages"):
        assert getattr(a, f) == getattr(b, f), f


@pytest.mark.parametrize("kind", ["resize_affine_crop", "randaug"])
def test_collate_mixed_batch(kind):
    """(array, JPEG, none): descriptors, tables and draws of the batch of PIL's decodes; one JPEG row"""
    tr = CT.CxrRandomTransform(32, kind) if kind == "randaug" else CT.CxrTransform(32, kind, True)
    arr, name = jpeg_cases.pixels_of("rst_rows1"), "37x51_q30"
    mk = lambda im: CT.collate_raw_cxr([([arr], [-1.0]), ([im], [-2.0]), ([], [])], tr, 0, generator=torch.Generator().manual_seed(9))
    for src in (jpeg_cases.file_of(name), bytearray(jpeg_cases.file_of(name)), memoryview(jpeg_cases.file_of(name))):
        mixed, plain = mk(src), mk(jpeg_cases.pixels_of(name))
        assert plain.jpeg is None
        _same_batch(mixed, plain, pixels=False)
        if kind == "randaug":
            assert torch.equal(mixed.aug, plain.aug)
        jp = mixed.jpeg
        assert jp.n == 1 and jp.images == [1] and jp.desc.shape == (1, J.JPG_WORDS) and jp.segs.shape == (1, J.SEG_WORDS)
        d = jp.desc[0].tolist()
        assert [d[k] for k in (J.JPG_H, J.JPG_W, J.JPG_BPR, J.JPG_NBLK, J.JPG_DST)] == [37, 51, 7, 35, arr.size]
        assert d[J.JPG_DST] == int(mixed.desc[1, CT.DESC_SRC]) and jp.tables.numel() == 64 + 2 * J.HUFF_WORDS
        assert torch.equal(mixed.pixels[:arr.size], plain.pixels[:arr.size]) and not mixed.pixels[arr.size:].any()
        moved = mixed.to("cpu")
        assert moved.jpeg is not None and torch.equal(moved.jpeg.streams, jp.streams) and moved.jpeg.images == [1]
        pix = mixed.pixels.numpy().copy()
        status, _ = jpeg_model.decode_plan(jp, pix)
        assert status.tolist() == [0] and np.array_equal(pix, plain.pixels.numpy())


def test_collate_shares_tables_between_files():
    files = [jpeg_cases.file_of(n) for n in ("one_block", "cxr_like", "smooth_opt", "100x9_q100")]
    raw = CT.collate_raw_cxr([([f], [-1.0]) for f in files], CT.CxrTransform(32, "resize", True), 0)
    d = raw.jpeg.desc
    assert d[0, J.JPG_QT] == d[1, J.JPG_QT] != d[3, J.JPG_QT] and d[0, J.JPG_DC] == d[1, J.JPG_DC] == d[3, J.JPG_DC]
    assert d[2, J.JPG_DC] != d[0, J.JPG_DC] and d[2, J.JPG_AC] != d[0, J.JPG_AC]
    assert raw.jpeg.tables.numel() == 2 * 64 + 4 * J.HUFF_WORDS and raw.jpeg.images == [0, 1, 2, 3]


def test_collate_of_arrays_is_unchanged():
    """no JPEG in the batch: no ``jpeg`` member, the pixel buffer is the arrays back to back, the rows are those of the golden
    chain case I (whose output tests/test_cxr_plan_cpu.py holds equal to PIL)"""
    from tests import cxr_cases
    raw, _ = cxr_cases.raw_and_expected("I")
    assert raw.jpeg is None and raw.to("cpu").jpeg is None
    srcs = [im for ims, _ in cxr_cases.samples_of("I") for im in ims]
    assert np.array_equal(raw.pixels.numpy(), np.concatenate([s.ravel() for s in srcs]))
    assert raw.desc[:, CT.DESC_SRC].tolist() == np.concatenate([[0], np.cumsum([s.size for s in srcs])])[:-1].tolist()
    assert raw.desc[:, CT.DESC_H].tolist() == [s.shape[0] for s in srcs]


def test_new_entry_points_declared_listed_and_exported():
    from medical_tri_modal_pilot_amd import _lib
    from tests import abi
    hdr = abi.header_text()
    L = _lib.lib()
    for name, nargs in (("mtmp_jpeg_entropy", 12), ("mtmp_jpeg_idct", 8)):
        ret, args = abi.declaration(name)
        restype, argtypes = _lib.SIGNATURES[name]
        assert ret == "int" and restype is ctypes.c_int and len(args) == len(argtypes) == nargs
        assert (restype, argtypes) == abi.ctypes_of(name)
        assert set(argtypes) == {ctypes.c_void_p, ctypes.c_int}
        assert getattr(L, name)
    assert "int32 [n][16]" in hdr and str(J.HUFF_WORDS) in hdr and J.JPG_WORDS == 16
    L.mtmp_abi_version.restype = ctypes.c_int
    assert L.mtmp_abi_version() == 6


def test_jpeg_ops_raise_on_host_tensors():
    from medical_tri_modal_pilot_amd import ops
    raw = CT.collate_raw_cxr([([jpeg_cases.file_of("one_block")], [-1.0])], CT.CxrTransform(32, "resize", True), 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cxr_prepare(raw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.jpeg_decode_images([jpeg_cases.file_of("one_block")], "cpu")
