"""The JPEG decoder on the GPU (csrc/jpeg.hip through ops.jpeg_decode / ops.jpeg_decode_images / ops.cxr_prepare): bit-equal to
PIL's own decodes (tests/golden/jpeg_cases.npz) for every subsequence length, one batch of all cases, the image chains fed file
bytes, a truncated stream, and a trainer step fed file bytes against the same step fed PIL's arrays."""
import math

import numpy as np
import pytest
import torch

import filler
from tests import cxr_aug_cases, cxr_cases, jpeg_cases
from tests.test_cxr_gpu import _two_steps
from tests.test_gpu_parity import DEV

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from medical_tri_modal_pilot_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def CT():
    from medical_tri_modal_pilot_amd.builder.data import cxr_transform
    return cxr_transform


@pytest.mark.parametrize("bits", jpeg_cases.SUBSEQ_BITS)
@pytest.mark.parametrize("name", jpeg_cases.names())
def test_jpeg_decode_images_equals_pil(ops, name, bits):
    (got,) = ops.jpeg_decode_images([jpeg_cases.file_of(name)], DEV, subseq_bits=bits)
    want = torch.from_numpy(jpeg_cases.pixels_of(name))
    assert got.dtype == torch.uint8 and got.shape == want.shape and got.is_cuda
    got = got.cpu()
    print(f"jpeg[{name}, {bits} bits]: {int((got != want).sum())} of {want.numel()} pixels differ from PIL's decode")
    assert torch.equal(got, want)


@pytest.mark.parametrize("stage", [0, 8192])
def test_segments_read_from_global_memory_and_from_lds(ops, stage):
    """stage_bytes 0: every segment is decoded out of global memory; 8192: the 15 KB segment of the 260 x 312 file is, the 6 KB
    one beside it out of LDS (the default stages both, as in the tests above)"""
    names = ("cxr_like", "noise_q100")
    got = ops.jpeg_decode_images([jpeg_cases.file_of(n) for n in names], DEV, stage_bytes=stage)
    for g, n in zip(got, names):
        assert torch.equal(g.cpu(), torch.from_numpy(jpeg_cases.pixels_of(n))), n


def _with_pattern(raw, guard: int):
    """the batch on the device, every JPEG image's bytes of ``pixels`` set to 0x5A and `guard` bytes of 0xA5 behind the last"""
    from medical_tri_modal_pilot_amd.builder.data import jpeg as J
    pix = raw.pixels.clone()
    for d in raw.jpeg.desc.tolist():
        pix[d[J.JPG_DST]:d[J.JPG_DST] + d[J.JPG_H] * d[J.JPG_W]] = 0x5A
    dev = raw.to(DEV)
    dev.pixels = torch.cat([pix, torch.full((guard,), 0xA5, dtype=torch.uint8)]).to(DEV)
    return dev


@pytest.mark.parametrize("bits", [None, 0, 128])
def test_batch_of_all_cases_fills_pixels_like_the_batch_of_arrays(ops, CT, bits):
    """every case in one RawCxrBatch: different tables and restart intervals, odd destination offsets (1 x 1 and 5 x 3 come first),
    an array image between two files; every byte of the files' regions is written, the array and the guard bytes are not"""
    tr = CT.CxrTransform(32, "resize", True)
    raw = CT.collate_raw_cxr(jpeg_cases.all_cases_samples(True), tr, 0)
    want = CT.collate_raw_cxr(jpeg_cases.all_cases_samples(False), tr, 0)
    n = len(jpeg_cases.names())
    assert want.jpeg is None and raw.jpeg.n == n and raw.jpeg.images == [0, 1] + list(range(3, n + 1))
    assert torch.equal(raw.desc, want.desc) and any(int(o) % 2 for o in raw.desc[:, CT.DESC_SRC])
    dev = _with_pattern(raw, 64)
    status = ops.jpeg_decode(dev, subseq_bits=bits)
    assert status.dtype == torch.int32 and status.cpu().tolist() == [0] * n
    got = dev.pixels.cpu()
    print(f"jpeg batch[{bits}]: {int((got[:-64] != want.pixels).sum())} of {want.pixels.numel()} bytes differ")
    assert torch.equal(got[:-64], want.pixels) and (got[-64:] == 0xA5).all()


def _chain_batches(CT, name):
    """(batch fed file bytes, batch fed PIL's decodes of them) of a golden chain case with its sources re-encoded as JPEG"""
    g = jpeg_cases.golden()
    if name in cxr_cases.names():
        samples, prefix = cxr_cases.samples_of(name), "cxr"
        srcs = [str(s) for s in cxr_cases.golden()[f"{name}.srcs"]]
        params = [tuple(float(v) for v in p) for p in cxr_cases.golden()[f"{name}.params"]]
        mk = lambda ss: CT.collate_raw_cxr(ss, cxr_cases.transform_of(name), int(cxr_cases.golden()[f"{name}.K"]),
                                           affine_params=params)
    else:
        samples, prefix = cxr_aug_cases.samples_of(name), "aug"
        srcs = [str(s) for s in cxr_aug_cases.golden()[f"{name}.srcs"]]
        ga = cxr_aug_cases.golden()
        aug, boxes = cxr_aug_cases.plan_of(name)
        mk = lambda ss: CT.collate_raw_cxr(ss, CT.CxrRandomTransform(int(ga[f"{name}.S"]), str(ga[f"{name}.kind"])),
                                           int(ga[f"{name}.K"]), aug_params=aug, crop_params=boxes)
    it = iter(srcs)
    keys = [[next(it) for _ in ims] for ims, _ in samples]
    files = [([g[f"file.{prefix}.{k}"].tobytes() for k in ks], t) for ks, (_, t) in zip(keys, samples)]
    arrays = [([g[f"pix.{prefix}.{k}"] for k in ks], t) for ks, (_, t) in zip(keys, samples)]
    return mk(files), mk(arrays)


@pytest.mark.parametrize("name", ["A", "E", "a_multi"])
def test_cxr_prepare_on_file_bytes_equals_cxr_prepare_on_pils_decodes(ops, CT, name):
    raw, plain = _chain_batches(CT, name)
    assert raw.jpeg is not None and raw.jpeg.n == raw.n and plain.jpeg is None
    got = ops.cxr_prepare(raw.to(DEV))
    want = ops.cxr_prepare(plain.to(DEV))
    print(f"jpeg chain[{name}]: {int((got != want).sum())} of {want.numel()} values differ")
    assert got.shape == want.shape and torch.equal(got, want) and float(want.max()) > 0.5


@pytest.mark.parametrize("bits", jpeg_cases.SUBSEQ_BITS)
def test_truncated_stream_sets_the_status_and_zeros_the_image(ops, CT, bits):
    """the 64 x 64 quality-100 file with the second half of its entropy-coded data missing, between two whole files: the call
    returns, that image's status is set and its pixels are zeros, the neighbours are bit-equal, cxr_prepare raises"""
    from medical_tri_modal_pilot_amd.builder.data import jpeg as J
    tr = CT.CxrTransform(32, "resize", True)
    names = ("37x51_q30", None, "rst_rows1")
    files = [jpeg_cases.truncated() if n is None else jpeg_cases.file_of(n) for n in names]
    raw = CT.collate_raw_cxr([([f], [-1.0]) for f in files], tr, 0)
    dev = _with_pattern(raw, 32)
    status = ops.jpeg_decode(dev, subseq_bits=bits).cpu().tolist()
    got = dev.pixels.cpu().numpy()
    assert status[0] == 0 and status[2] == 0 and status[1] & 1
    for d, n in zip(raw.jpeg.desc.tolist(), names):
        region = got[d[J.JPG_DST]:d[J.JPG_DST] + d[J.JPG_H] * d[J.JPG_W]]
        assert np.array_equal(region, jpeg_cases.pixels_of(n).ravel()) if n else not region.any()
    assert (got[-32:] == 0xA5).all()
    with pytest.raises(ValueError, match="image.* 1 .*truncated or corrupt"):
        ops.cxr_prepare(raw.to(DEV), subseq_bits=bits)
    out = ops.cxr_prepare(raw.to(DEV), check=False, subseq_bits=bits)
    assert float(out[1].abs().max()) == 0.0 and float(out[0].max()) > 0.5
    with pytest.raises(ValueError, match="truncated or corrupt"):
        ops.jpeg_decode_images([jpeg_cases.truncated()], DEV, subseq_bits=bits)


def test_trainer_step_on_file_bytes_equals_step_on_pils_arrays(CT):
    """TRI_MBT_VSLTCLS, B 2, 2 layers, TIE-len 64, 224 px, --hip-graph 1, two steps: the batch fed the files' bytes through the
    trainer's ops.cxr_prepare against the batch fed PIL's decodes of the same files"""
    bt = filler.make_batch(4321, 2, 64, missing_mode="none")
    names = ("cxr_like", "rst_blocks8")
    gen = lambda: torch.Generator().manual_seed(3)
    tr = CT.CxrTransform(224, "resize_affine_crop", True)
    times = [float(t) for t in bt["img_time"]]
    raw = CT.collate_raw_cxr([([jpeg_cases.file_of(n)], [t]) for n, t in zip(names, times)], tr, 0, generator=gen())
    plain = CT.collate_raw_cxr([([jpeg_cases.pixels_of(n)], [t]) for n, t in zip(names, times)], tr, 0, generator=gen())
    assert raw.jpeg.n == 2 and plain.jpeg is None and torch.equal(raw.desc, plain.desc) and torch.equal(raw.img_time, bt["img_time"])
    l_jpg, p_jpg = _two_steps(bt, raw)
    l_arr, p_arr = _two_steps(bt, plain)
    print(f"jpeg trainer: losses files {l_jpg} arrays {l_arr}")
    assert all(math.isfinite(v) for v in l_jpg)
    assert [np.float32(v).tobytes() for v in l_jpg] == [np.float32(v).tobytes() for v in l_arr]
    assert torch.equal(p_jpg, p_arr)
