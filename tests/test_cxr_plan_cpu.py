"""Host half of the chest X-ray input chain (builder/data/cxr_transform.py) without a GPU: the goldens are PIL's own
output (tests/golden/gen/make_golden_cxr.py), and a numpy executor of the launch plan -- descriptor rows, int32 bound /
coefficient tables, 16.16 affine words, crop offsets, slot map -- must equal every one of them bit for bit.  The executor
walks the plan the way csrc/image_prep.hip does (same tiles, same LDS row budget) and checks every address it forms."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from medical_tri_modal_pilot_amd.builder.data import cxr_transform as CT
from tests import cxr_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def equalize_lut(hist):
    """ImageOps.equalize's table from a 256-bin histogram; entries saturate at 255 as PIL's point() stores them."""
    hist = [int(v) for v in hist]
    nz = [v for v in hist if v]
    ident = np.arange(256, dtype=np.uint8)
    if len(nz) <= 1:
        return ident
    step = (sum(nz) - nz[-1]) // 255
    if step == 0:
        return ident
    lut, n = [], step // 2
    for v in hist:
        lut.append(min(n // step, 255))
        n += v
    return np.array(lut, np.uint8)


def run_plan(raw):
    """float32 output of the plan held by a host RawCxrBatch, computed the way the three kernels compute it."""
    pix, desc, tab, slot_map = raw.pixels.numpy(), raw.desc.numpy().astype(np.int64), raw.tables.numpy(), raw.slot_map.numpy()
    S = raw.image_size
    scratch = np.zeros(max(raw.scratch_bytes, 1), np.uint8)
    TR, TC = CT.TILE_ROWS, CT.TILE_COLS
    for d in desc:
        src, h, w, rh, rw = (int(d[i]) for i in (CT.DESC_SRC, CT.DESC_H, CT.DESC_W, CT.DESC_RH, CT.DESC_RW))
        assert 0 <= src and src + h * w <= pix.size and h * w <= raw.max_pixels and rh <= raw.max_rh and rw <= raw.max_rw
        img = pix[src:src + h * w].reshape(h, w)
        img = equalize_lut(np.bincount(img.ravel(), minlength=256))[img].astype(np.int64)
        hb0, hk0, hks, vb0, vk0, vks = (int(d[i]) for i in (CT.DESC_HB, CT.DESC_HK, CT.DESC_HKS, CT.DESC_VB, CT.DESC_VK, CT.DESC_VKS))
        assert max(hk0 + rw * hks, vk0 + rh * vks) <= tab.size and hb0 + 2 * rw <= hk0 and vb0 + 2 * rh <= vk0
        hb, hk = tab[hb0:hb0 + 2 * rw].reshape(rw, 2), tab[hk0:hk0 + rw * hks].reshape(rw, hks).astype(np.int64)
        vb, vk = tab[vb0:vb0 + 2 * rh].reshape(rh, 2), tab[vk0:vk0 + rh * vks].reshape(rh, vks).astype(np.int64)
        so = int(d[CT.DESC_SCRATCH])
        assert 0 <= so and so + rh * rw <= raw.scratch_bytes
        out = scratch[so:so + rh * rw].reshape(rh, rw)
        half = 1 << (CT.PRECISION_BITS - 1)
        for r0 in range(0, rh, TR):
            r1 = min(r0 + TR, rh)
            y0 = int(vb[r0, 0])
            rows = int(vb[r1 - 1, 0] + vb[r1 - 1, 1]) - y0
            assert 0 < rows <= raw.lds_rows and 0 <= y0 and y0 + rows <= h
            for c0 in range(0, rw, TC):
                c1 = min(c0 + TC, rw)
                lds = np.zeros((rows, TC), np.int64)
                for c in range(c0, c1):
                    x0, n = int(hb[c, 0]), int(hb[c, 1])
                    assert 0 <= x0 and 0 < n <= hks and x0 + n <= w
                    lds[:, c - c0] = np.clip((img[y0:y0 + rows, x0:x0 + n] @ hk[c, :n] + half) >> CT.PRECISION_BITS, 0, 255)
                for r in range(r0, r1):
                    ya, n = int(vb[r, 0]) - y0, int(vb[r, 1])
                    assert 0 <= ya and 0 < n <= vks and ya + n <= rows
                    out[r, c0:c1] = np.clip((vk[r, :n] @ lds[ya:ya + n, :c1 - c0] + half) >> CT.PRECISION_BITS, 0, 255)
    res = np.zeros((slot_map.size, S, S), np.float32)
    yy, xx = np.mgrid[0:S, 0:S].astype(np.int64)
    for slot, i in enumerate(slot_map):
        if i < 0:
            continue
        d = desc[i]
        assert int(d[CT.DESC_SLOT]) == slot
        rh, rw = int(d[CT.DESC_RH]), int(d[CT.DESC_RW])
        y, x = yy + int(d[CT.DESC_TOP]), xx + int(d[CT.DESC_LEFT])
        assert y.max() < rh and x.max() < rw
        if int(d[CT.DESC_FLAGS]) & CT.FLAG_AFFINE:
            a = [int(v) for v in d[CT.DESC_A0:CT.DESC_A5 + 1]]
            x, y = (a[2] + a[0] * x + a[1] * y) >> 16, (a[5] + a[3] * x + a[4] * y) >> 16
            assert max(abs(a[2]) + abs(a[0]) * rw + abs(a[1]) * rh, abs(a[5]) + abs(a[3]) * rw + abs(a[4]) * rh) < 2 ** 31
        ok = (x >= 0) & (x < rw) & (y >= 0) & (y < rh)
        so = int(d[CT.DESC_SCRATCH])
        v = scratch[so + np.where(ok, y * rw + x, 0)]
        res[slot] = np.where(ok, v, 0).astype(np.float32) / np.float32(255.0)
    return torch.from_numpy(res).view(raw.out_shape)


def test_generator_reproduces_committed_goldens():
    pytest.importorskip("PIL")
    spec = importlib.util.spec_from_file_location("make_golden_cxr", os.path.join(ROOT, "tests", "golden", "gen", "make_golden_cxr.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    fresh, kept = mod.build(), cxr_cases.golden()
    assert set(fresh) == set(kept)
    for k, v in fresh.items():
        assert np.array_equal(np.asarray(v), kept[k]) and np.asarray(v).dtype == kept[k].dtype, k
    assert os.path.getsize(cxr_cases.GOLDEN) < 200 * 1024


def test_golden_cases_reach_the_paths_they_are_there_for():
    g = cxr_cases.golden()
    assert cxr_cases.names() == list("ABCDEFGHI")
    assert g["src.A"].size < 255 and len(np.unique(g["src.F"])) == 1
    h = np.bincount(g["src.E"].ravel(), minlength=256)
    assert h[10] == 383 and h[200] == 64 * 64 - 383                       # level 200 maps to 383 before saturation
    assert g["E.crop"].max() == 255                # what PIL does there: it saturates (a wrapped entry, 383 & 255, gives <= 127)
    assert (g["B.crop"] == 0).mean() > 0.02                              # the zoom-out shows the zero fill
    raw, _ = cxr_cases.raw_and_expected("I")
    offs = raw.desc[:, CT.DESC_SRC].tolist()
    assert raw.slot_map.tolist() == [0, 1, -1, -1, -1, -1, 2, -1, -1] and offs[1] % 2 == 1 and offs[2] % 2 == 0
    rawd, _ = cxr_cases.raw_and_expected("D")
    assert rawd.desc[0, [CT.DESC_RH, CT.DESC_RW, CT.DESC_TOP, CT.DESC_LEFT]].tolist() == [37, 45, 2, 6]   # round half to even
    assert int(rawd.desc[0, CT.DESC_HKS]) == 3 and rawd.tables[int(rawd.desc[0, CT.DESC_HK])] == 1 << 22  # identity pass: one tap


@pytest.mark.parametrize("name", list("ABCDEFGHI"))
def test_numpy_executor_of_the_plan_equals_pil(name):
    raw, want = cxr_cases.raw_and_expected(name)
    assert raw.desc.dtype == torch.int32 and raw.tables.dtype == torch.int32 and raw.pixels.dtype == torch.uint8
    got = run_plan(raw)
    assert got.shape == want.shape and got.dtype == torch.float32
    assert torch.equal(got, want), f"{int((got != want).sum())} of {got.numel()} values differ"


def test_from_args_mapping_and_what_is_not_built():
    from medical_tri_modal_pilot_amd.control.config import parse_args
    a = parse_args([])
    tr, te = CT.CxrTransform.from_args(a, True), CT.CxrTransform.from_args(a, False)
    assert (tr.kind, tr.affine, tr.resize_to, tr.image_size) == ("resize_affine_crop", True, 256, 224)
    assert (te.kind, te.affine, te.resize_to, te.square) == ("resize_crop", False, 256, False)
    assert tr.resized(256, 311) == (256, 311) and tr.resized(1024, 841) == (311, 256) and tr.crop(256, 311) == (16, 44)
    a = parse_args(["--image-size", "512", "--image-train-type", "resize", "--image-test-type", "resize"])
    tr, te = CT.CxrTransform.from_args(a, True), CT.CxrTransform.from_args(a, False)
    assert (tr.resize_to, tr.square, tr.affine, tr.resized(256, 311)) == (512, False, False, (512, 622))
    assert (te.resize_to, te.square, te.resized(256, 311), te.crop(512, 512)) == (512, True, (512, 512), (0, 0))
    a = parse_args(["--image-size", "512", "--image-test-type", "center"])
    assert CT.CxrTransform.from_args(a, True).resize_to == 585 and CT.CxrTransform.from_args(a, False).resize_to == 512
    for kind, train in (("random", True), ("randaug", True), ("resize_larger", False)):
        with pytest.raises(NotImplementedError):
            CT.CxrTransform(224, kind, train)
    with pytest.raises(ValueError):
        CT.CxrTransform(224, "center", True)


def test_draw_affine_is_four_uniform_draws_in_get_params_order():
    w, h = 311, 256
    got = CT.draw_affine(w, h, torch.Generator().manual_seed(77))
    g = torch.Generator().manual_seed(77)
    angle = float(torch.empty(1).uniform_(-5.0, 5.0, generator=g).item())
    tx = int(round(float(torch.empty(1).uniform_(-0.15 * w, 0.15 * w, generator=g).item())))
    ty = int(round(float(torch.empty(1).uniform_(-0.15 * h, 0.15 * h, generator=g).item())))
    scale = float(torch.empty(1).uniform_(0.85, 1.15, generator=g).item())
    assert got == (angle, tx, ty, scale)
    assert -5 <= angle <= 5 and abs(tx) <= 47 and abs(ty) <= 38 and 0.85 <= scale <= 1.15
    # collate draws once per image in batch order and keeps what it drew
    ims = [np.full((40, 50), 9, np.uint8), np.full((50, 40), 9, np.uint8)]
    raw = CT.collate_raw_cxr([(ims, [-1.0, -2.0])], CT.CxrTransform(32, "resize_affine_crop", True), 3,
                             generator=torch.Generator().manual_seed(5))
    g = torch.Generator().manual_seed(5)
    p0, p1 = CT.draw_affine(46, 37, g), CT.draw_affine(37, 46, g)
    assert raw.params == [p0, p1]
    assert raw.desc[1, CT.DESC_A0:CT.DESC_A5 + 1].tolist() == CT.affine_words(CT.affine_matrix(37, 46, *p1))
    assert raw.img_time.tolist() == [[-1.0, -2.0, 10.0]] and raw.out_shape == (1, 3, 1, 32, 32)


def test_cxr_prepare_raises_on_host_tensors():
    from medical_tri_modal_pilot_amd import ops
    raw, _ = cxr_cases.raw_and_expected("A")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cxr_prepare(raw)
