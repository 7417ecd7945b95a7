"""Generate tests/golden/cxr_aug_cases.npz: the reference's ``random`` and ``randaug`` image chains run by PIL itself.

    python tests/golden/gen/make_golden_cxr_aug.py [OUT.npz]

Per image the reference's loader runs ``F_t.equalize`` and then RandAugment() (``randaug`` only) and
RandomResizedCrop(S, scale=(0.8, 1.1), ratio=(3/4, 4/3)) (builder/data/dataset_new.py:60-89, :2094-2096).  On a PIL ``L``
image torchvision turns every one of these into a PIL call, and those calls are made here directly, with explicit ops
and crop boxes instead of drawn ones: ``Image.transform(AFFINE, ..., NEAREST, fillcolor=0)`` for the shears and
translations, ``Image.rotate``, ``ImageEnhance.Brightness / Color / Contrast / Sharpness``, ``ImageOps.posterize /
solarize / autocontrast / equalize``, and ``img.crop((j, i, j + cw, i + ch)).resize((S, S), BILINEAR)``.  Only PIL and
numpy are imported.

Stored: the sources (``src.<name>``), per case ``kind``, ``S``, ``K`` (0 = one image per sample), which sources each
sample holds (``srcs``, ``counts``), per image its two ops (``ops`` names, ``mags`` float64; empty for ``random``) and crop
box (``boxes``: i, j, ch, cw), and PIL's uint8 result per output slot (``crop``, zeros where a slot has no image).
"""
import math
import os
import sys

import numpy as np
from PIL import Image, ImageEnhance, ImageOps

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)


def synth(rng, h, w, noise=10.0):
    y, x = np.mgrid[0:h, 0:w]
    a = 100 + 55 * np.sin(x / 11.0) * np.cos(y / 7.0) + 45 * (x / w) - 30 * (y / h) + rng.normal(0, noise, (h, w))
    return np.clip(a, 0, 255).astype(np.uint8)


def f32(v):
    return float(np.float32(v))


def apply_op(im, op, m):
    """what torchvision's RandAugment._apply_op does to a PIL ``L`` image (NEAREST, fill None -> 0)"""
    w, h = im.size
    if op == "Identity":
        return im
    if op == "ShearX":
        t = math.tan(math.radians(math.degrees(math.atan(m))))
        return im.transform((w, h), Image.AFFINE, [1.0, t, 0.0, 0.0, 1.0, 0.0], Image.NEAREST, fillcolor=0)
    if op == "ShearY":
        t = math.tan(math.radians(math.degrees(math.atan(m))))
        return im.transform((w, h), Image.AFFINE, [1.0, 0.0, 0.0, t, 1.0, 0.0], Image.NEAREST, fillcolor=0)
    if op == "TranslateX":
        return im.transform((w, h), Image.AFFINE, [1.0, 0.0, -float(int(m)), 0.0, 1.0, 0.0], Image.NEAREST, fillcolor=0)
    if op == "TranslateY":
        return im.transform((w, h), Image.AFFINE, [1.0, 0.0, 0.0, 0.0, 1.0, -float(int(m))], Image.NEAREST, fillcolor=0)
    if op == "Rotate":
        return im.rotate(m, Image.NEAREST, fillcolor=0)
    if op == "Brightness":
        return ImageEnhance.Brightness(im).enhance(1.0 + m)
    if op == "Color":
        return ImageEnhance.Color(im).enhance(1.0 + m)
    if op == "Contrast":
        return ImageEnhance.Contrast(im).enhance(1.0 + m)
    if op == "Sharpness":
        return ImageEnhance.Sharpness(im).enhance(1.0 + m)
    if op == "Posterize":
        return ImageOps.posterize(im, int(m))
    if op == "Solarize":
        return ImageOps.solarize(im, m)
    if op == "AutoContrast":
        return ImageOps.autocontrast(im)
    if op == "Equalize":
        return ImageOps.equalize(im)
    raise ValueError(op)


def chain(src, ops, box, S):
    im = ImageOps.equalize(Image.fromarray(src))
    for op, m in ops:
        im = apply_op(im, op, m)
    i, j, ch, cw = box
    out = np.asarray(im.crop((j, i, j + cw, i + ch)).resize((S, S), Image.BILINEAR))
    assert out.shape == (S, S) and out.dtype == np.uint8
    return out


def magnitude(op, h, w):
    """bin 9 of 31 of RandAugment's tables, to float32 as its tensors hold them"""
    return {"ShearX": f32(0.09), "ShearY": f32(0.09), "TranslateX": f32(150.0 / 331.0 * w * 0.3),
            "TranslateY": f32(150.0 / 331.0 * h * 0.3), "Rotate": 9.0, "Brightness": f32(0.27), "Color": f32(0.27),
            "Contrast": f32(0.27), "Sharpness": f32(0.27), "Posterize": 7.0, "Solarize": 178.5}.get(op, 0.0)


def build():
    rng = np.random.default_rng(20250)
    src = {"P": synth(rng, 37, 53), "Q": synth(rng, 53, 37), "R": synth(rng, 150, 181, noise=5.0),
           "L": synth(rng, 40, 200), "C": np.full((41, 59), 93, np.uint8)}
    b = np.full((45, 39), 140, np.uint8)
    b[17, 5] = 31                                   # one stray pixel below the single filled bin: equalize's step is 0
    src["B"] = b

    def ops_of(s, *pairs):
        h, w = src[s].shape
        return [(op, sign * magnitude(op, h, w)) for op, sign in pairs]

    ident = ("Identity", 1)
    # name: (kind, S, K, sources in batch order, images per sample, ops per image, crop box per image)
    cases = {
        "r_corner": ("random", 32, 0, ["P"], [1], [[]], [(0, 0, 33, 46)]),
        "r_far": ("random", 32, 0, ["Q"], [1], [[]], [(53 - 49, 37 - 35, 49, 35)]),
        "r_fallback": ("random", 32, 0, ["L"], [1], [[]], [(0, 73, 40, 53)]),
        "r_up": ("random", 48, 0, ["P"], [1], [[]], [(0, 2, 37, 50)]),
        "r_whole": ("random", 32, 0, ["C"], [1], [[]], [(0, 0, 41, 59)]),
        "a_224": ("randaug", 224, 0, ["R"], [1], [ops_of("R", ("ShearX", -1), ("Contrast", 1))], [(9, 14, 131, 160)]),
        "a_rot_eq": ("randaug", 48, 0, ["R"], [1], [ops_of("R", ("Rotate", 1), ("Equalize", 1))], [(11, 3, 136, 170)]),
        "a_shx_auto": ("randaug", 32, 0, ["P"], [1], [ops_of("P", ("ShearX", 1), ("AutoContrast", 1))], [(2, 3, 34, 47)]),
        "a_sol_ty": ("randaug", 32, 0, ["Q"], [1], [ops_of("Q", ("Solarize", 1), ("TranslateY", -1))], [(1, 0, 50, 36)]),
        "a_sharp_con": ("randaug", 32, 0, ["P"], [1], [ops_of("P", ("Sharpness", -1), ("Contrast", 1))], [(0, 4, 36, 45)]),
        "a_shy_rot": ("randaug", 32, 0, ["Q"], [1], [ops_of("Q", ("ShearY", -1), ("Rotate", -1))], [(3, 1, 47, 33)]),
        "a_id_id": ("randaug", 32, 0, ["P"], [1], [ops_of("P", ident, ident)], [(1, 1, 35, 50)]),
        "a_post_sharp": ("randaug", 32, 0, ["Q"], [1], [ops_of("Q", ("Posterize", 1), ("Sharpness", 1))], [(0, 0, 53, 37)]),
        "a_sharp_sharp": ("randaug", 32, 0, ["P"], [1], [ops_of("P", ("Sharpness", 1), ("Sharpness", -1))], [(0, 0, 37, 53)]),
        "a_con_auto": ("randaug", 32, 0, ["P"], [1], [ops_of("P", ("Contrast", -1), ("AutoContrast", 1))], [(2, 2, 33, 44)]),
        "a_const": ("randaug", 32, 0, ["C"], [1], [ops_of("C", ("AutoContrast", 1), ("Contrast", -1))], [(3, 5, 35, 48)]),
        "a_const_sharp": ("randaug", 32, 0, ["C"], [1], [ops_of("C", ("Sharpness", 1), ("Equalize", 1))], [(3, 5, 35, 48)]),
        "a_stray": ("randaug", 32, 0, ["B"], [1], [ops_of("B", ("AutoContrast", 1), ("Equalize", 1))], [(4, 0, 38, 39)]),
        "a_stray_rot": ("randaug", 32, 0, ["B"], [1], [ops_of("B", ("Rotate", -1), ("Equalize", 1))], [(4, 0, 38, 39)]),
        "a_multi": ("randaug", 32, 3, ["P", "Q", "R"], [2, 0, 1],
                    [ops_of("P", ("Brightness", -1), ("ShearY", 1)), ops_of("Q", ("TranslateX", 1), ("Sharpness", 1)),
                     ops_of("R", ("Equalize", 1), ("Posterize", 1))],
                    [(1, 2, 34, 48), (5, 0, 44, 37), (0, 20, 150, 150)]),
    }
    first = (("Identity", 1), ("ShearX", 1), ("ShearY", 1), ("TranslateX", -1), ("TranslateY", 1), ("Rotate", 1),
             ("Brightness", 1), ("Color", -1), ("Contrast", -1), ("Sharpness", 1), ("Posterize", 1), ("Solarize", 1),
             ("AutoContrast", 1), ("Equalize", 1))
    for n, (op, sign) in enumerate(first):
        s = "PQ"[n % 2]
        h, w = src[s].shape
        cases[f"a1_{op}"] = ("randaug", 32, 0, [s], [1], [ops_of(s, (op, sign), ident)], [(n % 3, n % 4, h - 3, w - 4)])
    store = {"names": np.array(sorted(cases))}
    for k, v in src.items():
        store[f"src.{k}"] = v
    for name, (kind, S, K, srcs, counts, ops, boxes) in cases.items():
        per = max(K, 1)
        crop = np.zeros((len(counts), per, S, S), np.uint8)
        i = 0
        for bi, c in enumerate(counts):
            for j in range(c):
                crop[bi, j] = chain(src[srcs[i]], ops[i], boxes[i], S)
                i += 1
        store[f"{name}.kind"] = np.array(kind)
        store[f"{name}.S"] = np.int64(S)
        store[f"{name}.K"] = np.int64(K)
        store[f"{name}.srcs"] = np.array(srcs)
        store[f"{name}.counts"] = np.array(counts, np.int64)
        store[f"{name}.ops"] = np.array([[op for op, _ in o] for o in ops]).reshape(len(ops), -1)
        store[f"{name}.mags"] = np.array([[m for _, m in o] for o in ops], np.float64).reshape(len(ops), -1)
        store[f"{name}.boxes"] = np.array(boxes, np.int64)
        store[f"{name}.crop"] = crop
    return store


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(GOLD, "cxr_aug_cases.npz")
    store = build()
    np.savez_compressed(out, **store)
    print("cases", len(store["names"]), "bytes", os.path.getsize(out))


if __name__ == "__main__":
    main()
