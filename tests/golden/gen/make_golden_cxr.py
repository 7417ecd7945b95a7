"""Generate tests/golden/cxr_cases.npz: the reference's chest X-ray input chain run by PIL itself.

    python tests/golden/gen/make_golden_cxr.py [OUT.npz]

The reference's loader runs, per image, ``F_t.equalize`` and one of the torchvision chains of
builder/data/dataset_new.py:91-160 on a PIL image (:2094-2096, :2110-2112).  torchvision is not needed to restate
them: on a PIL image ``equalize`` is ``ImageOps.equalize``, ``Resize`` is ``Image.resize(BILINEAR)`` to (short side n,
long side int(n long / short)), ``RandomAffine`` is ``Image.transform(AFFINE, inverse matrix, NEAREST, fillcolor=0)``,
``CenterCrop`` is ``Image.crop`` at ``int(round((size - S) / 2.0))`` and ``ToTensor`` divides the bytes by 255.  Only PIL
and numpy are imported here; the affine parameters are fixed instead of drawn.

Stored: the sources (generated from a seed, ``src.<name>``), per case its chain (``kind``, ``train``, ``S``, ``K``: 0 = one
image per sample), which sources each sample holds (``srcs``, ``counts``), the affine parameters (angle, tx, ty, scale)
per image, and PIL's uint8 crop per output slot (zeros where a slot has no image).  The expected float is crop / 255.
"""
import math
import os
import sys

import numpy as np
from PIL import Image, ImageOps

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)


def synth(rng, h, w, noise=12.0):
    y, x = np.mgrid[0:h, 0:w]
    a = 90 + 60 * np.sin(x / 37.0) * np.cos(y / 23.0) + 40 * (x / w) + rng.normal(0, noise, (h, w))
    return np.clip(a, 0, 255).astype(np.uint8)


def inverse_matrix(w, h, angle, tx, ty, s):
    cx, cy = w * 0.5, h * 0.5
    r = math.radians(angle)
    m = [math.cos(r) / s, math.sin(r) / s, 0.0, -math.sin(r) / s, math.cos(r) / s, 0.0]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def chain(src, kind, train, S, params):
    im = ImageOps.equalize(Image.fromarray(src))
    h, w = src.shape
    square = (not train) and kind == "resize"
    n = round(S * 1.142) if kind in ("resize_crop", "resize_affine_crop") else S
    if square:
        rw, rh = n, n
    elif w <= h:
        rw, rh = n, int(n * h / w)
    else:
        rw, rh = int(n * w / h), n
    im = im.resize((rw, rh), Image.BILINEAR)
    if train and kind == "resize_affine_crop":
        im = im.transform((rw, rh), Image.AFFINE, inverse_matrix(rw, rh, *params), Image.NEAREST, fillcolor=0)
    if not square:
        top, left = int(round((rh - S) / 2.0)), int(round((rw - S) / 2.0))
        im = im.crop((left, top, left + S, top + S))
    out = np.asarray(im)
    assert out.shape == (S, S) and out.dtype == np.uint8
    return out


def build():
    rng = np.random.default_rng(20240)
    src = {"A": synth(rng, 12, 15), "B": synth(rng, 97, 131), "C": synth(rng, 131, 97), "D": synth(rng, 37, 45),
           "G": synth(rng, 50, 81), "H": synth(rng, 256, 311, noise=4.0)}
    e = np.full(64 * 64, 200, np.uint8)
    e[rng.permutation(64 * 64)[:383]] = 10          # step = 383 // 255 = 1: the LUT entry of level 200 is 383 before PIL stores it
    src["E"] = e.reshape(64, 64)
    src["F"] = np.full((40, 50), 77, np.uint8)
    pB, pC = (4.3, 5, -4, 0.9), (-3.1, -3, 5, 1.12)
    none = (0.0, 0, 0, 1.0)
    # name: (kind, train, S, K, sources in batch order, images per sample, affine parameters per image)
    cases = {
        "A": ("resize_crop", 1, 16, 0, ["A"], [1], [none]),
        "B": ("resize_affine_crop", 1, 32, 0, ["B"], [1], [pB]),
        "C": ("resize_affine_crop", 1, 32, 0, ["C"], [1], [pC]),
        "D": ("resize_crop", 1, 32, 0, ["D"], [1], [none]),
        "E": ("resize", 1, 32, 0, ["E"], [1], [none]),
        "F": ("center", 0, 32, 0, ["F"], [1], [none]),
        "G": ("resize", 0, 32, 0, ["G"], [1], [none]),
        "H": ("resize_affine_crop", 1, 224, 0, ["H"], [1], [(-2.7, 11, -9, 1.06)]),
        "I": ("resize_affine_crop", 1, 32, 3, ["B", "C", "D"], [2, 0, 1],
              [(1.9, -2, 3, 1.05), (-4.6, 4, 1, 0.88), (2.2, 1, -2, 0.97)]),
    }
    store = {"names": np.array(sorted(cases))}
    for k, v in src.items():
        store[f"src.{k}"] = v
    for name, (kind, train, S, K, srcs, counts, params) in cases.items():
        per = max(K, 1)
        crop = np.zeros((len(counts), per, S, S), np.uint8)
        i = 0
        for b, c in enumerate(counts):
            for j in range(c):
                crop[b, j] = chain(src[srcs[i]], kind, bool(train), S, params[i])
                i += 1
        store[f"{name}.kind"] = np.array(kind)
        store[f"{name}.train"] = np.int64(train)
        store[f"{name}.S"] = np.int64(S)
        store[f"{name}.K"] = np.int64(K)
        store[f"{name}.srcs"] = np.array(srcs)
        store[f"{name}.counts"] = np.array(counts, np.int64)
        store[f"{name}.params"] = np.array(params, np.float64)
        store[f"{name}.crop"] = crop
    return store


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(GOLD, "cxr_cases.npz")
    store = build()
    np.savez_compressed(out, **store)
    print("cases", list(store["names"]), "bytes", os.path.getsize(out))


if __name__ == "__main__":
    main()
