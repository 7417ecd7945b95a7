"""Host half of the ``random`` / ``randaug`` image chains (builder/data/cxr_transform.py) without a GPU: the goldens are
PIL's own output (tests/golden/gen/make_golden_cxr_aug.py), and a numpy executor of the launch plan -- AUG_* descriptor
rows, coefficient tables of the crop boxes, slot map -- must equal every one of them, and PIL called live, bit for bit.
The executor shares the descriptor constants with the kernels of csrc/image_aug.hip and nothing else.  The rules PIL
was probed for (the blend, the SMOOTH filter, the Translate shift, Color on an ``L`` image) are pinned here as well."""
import ctypes
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from medical_tri_modal_pilot_amd.builder.data import cxr_transform as CT
from tests import cxr_aug_cases
from tests.test_cxr_plan_cpu import equalize_lut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = cxr_aug_cases.names()


def blend(a, b, bits):
    """Image.blend(a, b, f) on int arrays: float32 ``a + f * (b - a)``, clipped, truncated."""
    f = np.array([bits], np.int32).view(np.float32)[0]
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    t = a.astype(np.float32) + f * (b - a).astype(np.float32)
    assert t.dtype == np.float32
    return np.clip(t, np.float32(0), np.float32(255)).astype(np.int64)


def table_of(code, par, hist):
    """the 256-entry table of one table op for an image with these counts"""
    v = np.arange(256, dtype=np.int64)
    hist = [int(x) for x in hist]
    if code == CT.TABLE_EQUALIZE:
        return equalize_lut(hist).astype(np.int64)
    if code == CT.TABLE_BRIGHTNESS:
        return blend(np.zeros(256, np.int64), v, par)
    if code == CT.TABLE_CONTRAST:
        n, s = sum(hist), sum(i * c for i, c in enumerate(hist))
        mean = (2 * s + n) // (2 * n)                         # int(s / n + 0.5): the quotient is never within 2^-32 of a half
        assert mean == int(s / n + 0.5)
        return blend(np.full(256, mean, np.int64), v, par)
    if code == CT.TABLE_POSTERIZE:
        return v & par
    if code == CT.TABLE_SOLARIZE:
        return np.where(v < par, v, 255 - v)
    if code == CT.TABLE_AUTOCONTRAST:
        nz = [i for i, c in enumerate(hist) if c]
        lo, hi = nz[0], nz[-1]
        if hi <= lo:
            return v
        scale = 255.0 / (hi - lo)
        offset = -lo * scale
        return np.array([min(max(int(i * scale + offset), 0), 255) for i in range(256)], np.int64)
    raise AssertionError(f"table code {code}")


def smooth(img):
    """ImageFilter.SMOOTH on an int array: (1 1 1 / 1 5 1 / 1 1 1) / 13 rounded half up, the border copied."""
    out = img.copy()
    h, w = img.shape
    if h > 2 and w > 2:
        t = 4 * img[1:-1, 1:-1]
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                t = t + img[dy:dy + h - 2, dx:dx + w - 2]
        out[1:-1, 1:-1] = (2 * t + 13) // 26
    return out


def run_aug_plan(raw):
    """float32 output of the plan held by a host RawCxrBatch of the random chains."""
    pix, aug, tab, slot_map = raw.pixels.numpy(), raw.aug.numpy().astype(np.int64), raw.tables.numpy(), raw.slot_map.numpy()
    S = raw.image_size
    res = np.zeros((slot_map.size, S, S), np.float32)
    half = 1 << (CT.PRECISION_BITS - 1)
    for slot, n in enumerate(slot_map):
        if n < 0:
            continue
        d = aug[n]
        assert int(d[CT.AUG_SLOT]) == slot and raw.desc[n, [CT.DESC_SRC, CT.DESC_H, CT.DESC_W]].tolist() == \
            d[[CT.AUG_SRC, CT.AUG_H, CT.AUG_W]].tolist()
        src, h, w = int(d[CT.AUG_SRC]), int(d[CT.AUG_H]), int(d[CT.AUG_W])
        assert 0 <= src and src + h * w <= pix.size and h * w <= raw.max_pixels
        maps = {0: pix[src:src + h * w].reshape(h, w).astype(np.int64)}

        def read(r):
            """the map reader r sees: its base through the pending tables"""
            o = CT.AUG_READ + 8 * r
            base, nt = int(d[o]), int(d[o + 1])
            assert base in maps and 0 <= nt <= 3
            m = maps[base]
            hist = np.bincount(m.ravel(), minlength=256)
            lut = np.arange(256, dtype=np.int64)
            for t in range(nt):
                tb = table_of(int(d[o + 2 + t]), int(d[o + 5 + t]), hist)
                assert tb.min() >= 0 and tb.max() <= 255
                lut = tb[lut]
                hist = np.bincount(tb, weights=hist, minlength=256).astype(np.int64)
            return lut[m]

        for k in (0, 1):
            o = CT.AUG_STAGE + 8 * k
            kind = int(d[o])
            if kind == CT.STAGE_NONE:
                continue
            assert raw.stages >> k & 1 and int(d[CT.AUG_SCR]) % 16 == 0 and int(d[CT.AUG_SCR]) + h * w <= raw.scratch_bytes
            m = read(k)
            if kind == CT.STAGE_AFFINE:
                a = [int(v) for v in d[o + 1:o + 7]]
                assert max(abs(a[2]) + abs(a[0]) * w + abs(a[1]) * h, abs(a[5]) + abs(a[3]) * w + abs(a[4]) * h) < 2 ** 31
                y, x = np.mgrid[0:h, 0:w].astype(np.int64)
                xin, yin = (a[2] + a[0] * x + a[1] * y) >> 16, (a[5] + a[3] * x + a[4] * y) >> 16
                ok = (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)
                maps[k + 1] = np.where(ok, m[np.where(ok, yin, 0), np.where(ok, xin, 0)], 0)
            else:
                assert kind == CT.STAGE_SHARPNESS
                maps[k + 1] = blend(smooth(m), m, int(d[o + 1]))
        i, j, ch, cw = (int(v) for v in d[CT.AUG_I:CT.AUG_CW + 1])
        assert 0 <= i and 0 <= j and 0 < ch and 0 < cw and i + ch <= h and j + cw <= w
        win = read(2)[i:i + ch, j:j + cw]
        hb0, hk0, hks, vb0, vk0, vks = (int(v) for v in d[CT.AUG_HB:CT.AUG_VKS + 1])
        assert max(hk0 + S * hks, vk0 + S * vks) <= tab.size and hb0 + 2 * S <= hk0 and vb0 + 2 * S <= vk0
        hb, hk = tab[hb0:hb0 + 2 * S].reshape(S, 2), tab[hk0:hk0 + S * hks].reshape(S, hks).astype(np.int64)
        vb, vk = tab[vb0:vb0 + 2 * S].reshape(S, 2), tab[vk0:vk0 + S * vks].reshape(S, vks).astype(np.int64)
        for r0 in range(0, S, CT.TILE_ROWS):
            r1 = min(r0 + CT.TILE_ROWS, S) - 1
            assert 0 < int(vb[r1, 0] + vb[r1, 1] - vb[r0, 0]) <= raw.lds_rows
        hor = np.zeros((ch, S), np.int64)
        for c in range(S):
            x0, nn = int(hb[c, 0]), int(hb[c, 1])
            assert 0 <= x0 and 0 < nn <= hks and x0 + nn <= cw
            hor[:, c] = np.clip((win[:, x0:x0 + nn] @ hk[c, :nn] + half) >> CT.PRECISION_BITS, 0, 255)
        out = np.zeros((S, S), np.int64)
        for r in range(S):
            y0, nn = int(vb[r, 0]), int(vb[r, 1])
            assert 0 <= y0 and 0 < nn <= vks and y0 + nn <= ch
            out[r] = np.clip((vk[r, :nn] @ hor[y0:y0 + nn] + half) >> CT.PRECISION_BITS, 0, 255)
        res[slot] = out.astype(np.float32) / np.float32(255.0)
    return torch.from_numpy(res).view(raw.out_shape)


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_cxr_aug",
                                                  os.path.join(ROOT, "tests", "golden", "gen", "make_golden_cxr_aug.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_generator_reproduces_committed_goldens():
    pytest.importorskip("PIL")
    fresh, kept = _generator().build(), cxr_aug_cases.golden()
    assert set(fresh) == set(kept)
    for k, v in fresh.items():
        assert np.array_equal(np.asarray(v), kept[k]) and np.asarray(v).dtype == kept[k].dtype, k
    assert os.path.getsize(cxr_aug_cases.GOLDEN) < 200 * 1024


def test_golden_cases_reach_the_paths_they_are_there_for():
    g = cxr_aug_cases.golden()
    assert len(np.unique(g["src.C"])) == 1
    hb = np.bincount(g["src.B"].ravel(), minlength=256)
    assert sorted(hb[hb > 0].tolist()) == [1, 45 * 39 - 1]
    firsts = {str(g[f"{n}.ops"][0, 0]) for n in NAMES if n.startswith("a1_")}
    assert firsts == set(CT.RANDAUG_OPS) and all(str(g[f"{n}.ops"][0, 1]) == "Identity" for n in NAMES if n.startswith("a1_"))
    assert tuple(g["r_fallback.boxes"][0]) == CT.draw_resized_crop(40, 200, torch.Generator().manual_seed(0))  # no draw accepts
    raw, _ = cxr_aug_cases.raw_and_expected("r_up")
    assert int(raw.aug[0, CT.AUG_VKS]) == 3 and int(raw.aug[0, CT.AUG_CH]) < 48 <= int(raw.aug[0, CT.AUG_CW])   # upscaling: ksize 3
    assert raw.stages == 0 and raw.scratch_bytes == 0 and raw.image_size > CT.TILE_ROWS                      # two row tiles
    raw, _ = cxr_aug_cases.raw_and_expected("a_multi")
    assert raw.slot_map.tolist() == [0, 1, -1, -1, -1, -1, 2, -1, -1] and raw.aug[1, CT.AUG_SRC] % 2 == 1
    assert raw.stages == 3 and raw.aug[:, CT.AUG_STAGE].tolist() == [0, CT.STAGE_AFFINE, 0]
    assert raw.aug[:, CT.AUG_STAGE + 8].tolist() == [CT.STAGE_AFFINE, CT.STAGE_SHARPNESS, 0]
    rd = raw.aug[2, CT.AUG_READ + 16:CT.AUG_READ + 24].tolist()
    assert rd[:5] == [0, 3, CT.TABLE_EQUALIZE, CT.TABLE_EQUALIZE, CT.TABLE_POSTERIZE] and rd[7] == 0xFE
    raw, _ = cxr_aug_cases.raw_and_expected("a_rot_eq")              # the resize reads stage 0's map through Equalize alone
    assert raw.aug[0, CT.AUG_READ + 16:CT.AUG_READ + 19].tolist() == [1, 1, CT.TABLE_EQUALIZE] and raw.stages == 1


@pytest.mark.parametrize("name", NAMES)
def test_numpy_executor_of_the_plan_equals_pil(name):
    raw, want = cxr_aug_cases.raw_and_expected(name)
    assert raw.aug.dtype == torch.int32 and raw.aug.shape[1] == CT.AUG_WORDS and raw.desc.shape[1] == CT.DESC_WORDS
    got = run_aug_plan(raw)
    assert got.shape == want.shape and got.dtype == torch.float32
    assert torch.equal(got, want), f"{int((got != want).sum())} of {got.numel()} values differ"


def test_numpy_executor_equals_pil_called_live_on_drawn_plans():
    """ops and boxes drawn by the module itself (not the generator's nominal magnitudes), every op met, PIL run here"""
    pytest.importorskip("PIL")
    gen, g = _generator(), torch.Generator().manual_seed(2025)
    rng = np.random.default_rng(7)
    seen = set()
    for n in range(40):
        h, w = int(rng.integers(30, 70)), int(rng.integers(30, 70))
        src = gen.synth(rng, h, w)
        raw = CT.collate_raw_cxr([([src], [-1.0])], CT.CxrRandomTransform(32, "randaug"), 0, generator=g)
        ops, box = raw.params[0]
        seen.update(op for op, _ in ops)
        want = torch.from_numpy(np.array(gen.chain(src, ops, box, 32))).float() / 255.0
        got = run_aug_plan(raw)
        assert torch.equal(got[0, 0], want), (n, ops, box)
    assert seen == set(CT.RANDAUG_OPS)


@pytest.mark.parametrize("factor", [0.1, 1.9, 0.55])
def test_blend_rule_over_all_byte_pairs(factor):
    Image = pytest.importorskip("PIL.Image")
    a, b = np.mgrid[0:256, 0:256].astype(np.uint8)
    want = np.asarray(Image.blend(Image.fromarray(a), Image.fromarray(b), factor))
    got = blend(a, b, CT._f32_bits(factor))
    assert np.array_equal(got, want)


def test_smooth_translate_and_color_rules():
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageEnhance, ImageFilter
    rng = np.random.default_rng(11)
    for h, w in ((3, 3), (37, 53), (64, 5)):
        src = rng.integers(0, 256, (h, w), dtype=np.uint8)
        im = Image.fromarray(src)
        assert np.array_equal(smooth(src.astype(np.int64)), np.asarray(im.filter(ImageFilter.SMOOTH)))
        for f in (0.73, 1.27):
            assert np.array_equal(np.asarray(ImageEnhance.Color(im).enhance(f)), src)
        for tx, ty in ((5, 0), (-5, 0), (0, 7), (0, -2)):
            got = np.asarray(im.transform((w, h), Image.AFFINE, [1.0, 0.0, -float(tx), 0.0, 1.0, -float(ty)], Image.NEAREST,
                                          fillcolor=0))
            want = np.pad(src, 8)[8 - ty:8 - ty + h, 8 - tx:8 - tx + w]          # out[y, x] = in[y - ty, x - tx], 0 outside
            assert np.array_equal(got, want), (tx, ty)
            assert CT.plan_op("TranslateX", float(tx) + 0.6 * np.sign(tx), h, w) == \
                (("affine", [65536, 0, -tx * 65536 + 32768, 0, 65536, 32768]) if tx else None)


def test_draw_resized_crop():
    seen_fallback = seen_accept = False
    for seed in range(60):
        h, w = (40, 200) if seed % 3 == 0 else (37 + seed, 53 + 2 * seed)
        box = CT.draw_resized_crop(h, w, torch.Generator().manual_seed(seed))
        assert box == CT.draw_resized_crop(h, w, torch.Generator().manual_seed(seed))
        i, j, ch, cw = box
        assert 0 <= i and 0 <= j and 0 < ch and 0 < cw and i + ch <= h and j + cw <= w
        # replay: count the draws
        g = torch.Generator().manual_seed(seed)
        lr = torch.log(torch.tensor((3.0 / 4.0, 4.0 / 3.0)))
        want, draws = None, 0
        for _ in range(10):
            area = h * w * torch.empty(1).uniform_(0.8, 1.1, generator=g).item()
            asp = torch.exp(torch.empty(1).uniform_(float(lr[0]), float(lr[1]), generator=g)).item()
            draws += 2
            tw, th = int(round(math.sqrt(area * asp))), int(round(math.sqrt(area / asp)))
            if 0 < tw <= w and 0 < th <= h:
                want = (int(torch.randint(0, h - th + 1, (1,), generator=g)), int(torch.randint(0, w - tw + 1, (1,), generator=g)), th, tw)
                draws += 2
                break
        if want is None:
            fh, fw = (int(round(w / (3 / 4))), w) if w / h < 3 / 4 else (h, int(round(h * 4 / 3))) if w / h > 4 / 3 else (h, w)
            assert draws == 20 and box == ((h - fh) // 2, (w - fw) // 2, fh, fw)
            assert (h, w) != (40, 200) or box == (0, 73, 40, 53)
            seen_fallback = seen_fallback or (h, w) == (40, 200)
        else:
            assert box == want and draws % 2 == 0
            seen_accept = True
        g2 = torch.Generator().manual_seed(seed)
        CT.draw_resized_crop(h, w, g2)
        assert torch.equal(g2.get_state(), g.get_state())          # exactly these draws were consumed
    assert seen_fallback and seen_accept
    assert CT.draw_resized_crop(200, 40, torch.Generator().manual_seed(1)) == (73, 0, 53, 40)


def test_draw_randaug():
    seen = set()
    for seed in range(120):
        h, w = 256, 311
        ops = CT.draw_randaug(h, w, torch.Generator().manual_seed(seed))
        assert ops == CT.draw_randaug(h, w, torch.Generator().manual_seed(seed)) and len(ops) == 2
        g = torch.Generator().manual_seed(seed)
        for op, m in ops:
            assert CT.RANDAUG_OPS[int(torch.randint(14, (1,), generator=g))] == op
            mag = CT.randaug_magnitude(op, h, w)
            if op in CT.RANDAUG_SIGNED:
                mag = -mag if int(torch.randint(2, (1,), generator=g)) else mag
            assert m == mag
            seen.add(op)
        g2 = torch.Generator().manual_seed(seed)
        CT.draw_randaug(h, w, g2)
        assert torch.equal(g2.get_state(), g.get_state())
    assert seen == set(CT.RANDAUG_OPS)
    f = lambda v: float(np.float32(v))
    mags = {op: CT.randaug_magnitude(op, 256, 311) for op in CT.RANDAUG_OPS}
    assert mags["Posterize"] == 7.0 and mags["Solarize"] == 178.5 and mags["Rotate"] == 9.0 and mags["Identity"] == 0.0
    assert abs(mags["ShearX"] - 0.09) < 1e-7 and abs(mags["Contrast"] - 0.27) < 1e-7 and mags["Equalize"] == 0.0
    assert int(mags["TranslateX"]) == int(150 / 331 * 311 * 0.3) and int(mags["TranslateY"]) == int(150 / 331 * 256 * 0.3)
    assert mags["ShearX"] == f(mags["ShearX"])                      # float32 values, as the tensors hold them
    # collate draws the ops and then the box, per image, and keeps what it drew
    ims = [np.full((40, 50), 9, np.uint8), np.full((50, 40), 9, np.uint8)]
    raw = CT.collate_raw_cxr([(ims, [-1.0, -2.0])], CT.CxrRandomTransform(32, "randaug"), 3, generator=torch.Generator().manual_seed(5))
    g = torch.Generator().manual_seed(5)
    want = []
    for h, w in ((40, 50), (50, 40)):
        o = CT.draw_randaug(h, w, g)
        want.append((tuple(o), CT.draw_resized_crop(h, w, g)))
    assert raw.params == want and raw.img_time.tolist() == [[-1.0, -2.0, 10.0]] and raw.out_shape == (1, 3, 1, 32, 32)
    raw = CT.collate_raw_cxr([(ims[:1], [-1.0])], CT.CxrRandomTransform(32, "random"), 0, generator=torch.Generator().manual_seed(5))
    assert raw.params == [((), CT.draw_resized_crop(40, 50, torch.Generator().manual_seed(5)))] and raw.stages == 0


def test_transform_from_args_for_all_kinds():
    from medical_tri_modal_pilot_amd.control.config import parse_args
    for kind in ("resize", "resize_crop", "resize_affine_crop"):
        t = CT.transform_from_args(parse_args(["--image-train-type", kind]), True)
        assert type(t) is CT.CxrTransform and t.kind == kind and t.train
    for kind in ("center", "resize_crop", "resize"):
        t = CT.transform_from_args(parse_args(["--image-test-type", kind, "--image-train-type", "random"]), False)
        assert type(t) is CT.CxrTransform and t.kind == kind and not t.train
    for kind in ("random", "randaug"):
        t = CT.transform_from_args(parse_args(["--image-train-type", kind, "--image-size", "512"]), True)
        assert type(t) is CT.CxrRandomTransform and t.kind == kind and t.image_size == 512 and t.randaug == (kind == "randaug")
        with pytest.raises(NotImplementedError, match="transform_from_args"):
            CT.CxrTransform(224, kind, True)
    with pytest.raises(NotImplementedError):
        CT.transform_from_args(parse_args(["--image-test-type", "resize_larger"]), False)
    with pytest.raises(ValueError):
        CT.CxrRandomTransform(224, "resize")


def test_collate_rejects_what_the_kernels_cannot_take():
    im = np.zeros((40, 50), np.uint8)
    tr = CT.CxrRandomTransform(32, "random")
    for box in ((0, 0, 41, 50), (-1, 0, 10, 10), (0, 45, 10, 6), (0, 0, 0, 10)):
        with pytest.raises(ValueError, match="crop box"):
            CT.collate_raw_cxr([([im], [-1.0])], tr, 0, crop_params=[box])
    tall = np.zeros((4000, 8), np.uint8)                              # 32 output rows of a 4000 -> 32 resize read > 960 rows
    with pytest.raises(ValueError, match="source rows"):
        CT.collate_raw_cxr([([tall], [-1.0])], tr, 0, crop_params=[(0, 0, 4000, 8)])


def test_library_exports_the_new_entry_points_and_keeps_abi_6():
    from medical_tri_modal_pilot_amd import _lib
    L = _lib.lib()
    for name in ("mtmp_cxr_aug_stage", "mtmp_cxr_crop_resize", "mtmp_cxr_hist", "mtmp_cxr_resize", "mtmp_cxr_affine_crop"):
        assert name in _lib.SIGNATURES and getattr(L, name)
    L.mtmp_abi_version.restype = ctypes.c_int
    assert L.mtmp_abi_version() == 6


@pytest.mark.parametrize("name", ["r_corner", "a_multi"])
def test_cxr_prepare_raises_on_host_tensors(name):
    from medical_tri_modal_pilot_amd import ops
    raw, _ = cxr_aug_cases.raw_and_expected(name)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cxr_prepare(raw)
