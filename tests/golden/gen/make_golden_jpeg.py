"""Generate tests/golden/jpeg_cases.npz: baseline greyscale JPEG files written and decoded by PIL itself.

    python tests/golden/gen/make_golden_jpeg.py [OUT.npz]

The reference's images are what ``Image.convert('L').save(path)`` writes (1_mimic_cxr_preprocess.py:81-82) and its loader reads
them back with ``Image.open`` (builder/data/dataset_new.py:2094).  Each case here is the smallest input at which one part of a
decoder can go wrong; ``file.<case>`` holds the file's bytes and ``pix.<case>`` the array PIL decodes from them.  Only PIL and
numpy are imported.

Also stored: three files a baseline greyscale decoder must refuse (``bad.progressive``, ``bad.rgb``, ``bad.cut``: a header cut
short), and the sources of the golden chains A and E of cxr_cases.npz and of a_multi of cxr_aug_cases.npz re-encoded as JPEG
(``file.cxr.<source>`` / ``file.aug.<source>`` with their decodes), for the tests that feed file bytes to ops.cxr_prepare.
"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)


def encode(a, **kw):
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", **kw)
    return buf.getvalue()


def decode(data):
    im = Image.open(io.BytesIO(data))
    assert im.mode == "L"
    return np.asarray(im).copy()


def smooth(rng, h, w, noise):
    y, x = np.mgrid[0:h, 0:w]
    a = 90 + 60 * np.sin(x / 37.0) * np.cos(y / 23.0) + 40 * (x / max(w, 1)) + rng.normal(0, noise, (h, w))
    return np.clip(a, 0, 255).astype(np.uint8)


def cxr_like(rng, h, w):
    """synthetic.make_raw_cxr's formula, with a white and a black patch"""
    y, x = np.mgrid[0:h, 0:w]
    a = (70 + 90 * rng.random() + 60 * np.sin(x / (20 + 40 * rng.random())) * np.cos(y / (15 + 30 * rng.random()))
         + 40 * (x / w) + rng.normal(0, 10, (h, w)))
    a = np.clip(a, 0, 255).astype(np.uint8)
    a[20:60, 30:90] = 255
    a[h - 50:h - 10, w - 80:w - 20] = 0
    return a


def build():
    rng = np.random.default_rng(20260)
    noise = lambda h, w: rng.integers(0, 256, (h, w), dtype=np.uint8)
    checker = (((np.mgrid[0:48, 0:40][0] // 3 + np.mgrid[0:48, 0:40][1] // 5) & 1) * 255).astype(np.uint8)
    # name: (pixels, save() arguments)
    cases = {
        "one_block": (smooth(rng, 8, 8, 12.0), dict(quality=75)),
        "1x1": (noise(1, 1), dict(quality=75)),
        "5x3": (noise(5, 3), dict(quality=75)),
        "37x51_q30": (smooth(rng, 37, 51, 12.0), dict(quality=30)),
        "100x9_q100": (smooth(rng, 100, 9, 12.0), dict(quality=100)),
        "noise_q100": (noise(64, 64), dict(quality=100)),
        "noise_q1": (noise(64, 64), dict(quality=1)),
        "checker_q3": (checker, dict(quality=3)),
        "smooth_opt": (smooth(rng, 64, 72, 3.0), dict(quality=75, optimize=True)),
        "rst_blocks1": (smooth(rng, 16, 24, 12.0), dict(quality=75, restart_marker_blocks=1)),
        "rst_blocks8": (smooth(rng, 224, 224, 0.5), dict(quality=75, restart_marker_blocks=8)),
        "rst_rows1": (smooth(rng, 33, 47, 12.0), dict(quality=75, restart_marker_rows=1)),
        "cxr_like": (cxr_like(rng, 260, 312), dict(quality=75)),
    }
    store = {"names": np.array(list(cases))}
    for name, (a, kw) in cases.items():
        data = encode(a, **kw)
        store[f"file.{name}"] = np.frombuffer(data, np.uint8)
        store[f"pix.{name}"] = decode(data)
        assert store[f"pix.{name}"].shape == a.shape
    base = smooth(rng, 24, 24, 12.0)
    store["bad.progressive"] = np.frombuffer(encode(base, quality=75, progressive=True), np.uint8)
    store["bad.rgb"] = np.frombuffer(encode(np.stack([base] * 3, 2), quality=75), np.uint8)
    whole = encode(base, quality=75)
    store["bad.cut"] = np.frombuffer(whole[:whole.index(b"\xff\xc4") + 10], np.uint8)          # inside the first DHT
    with np.load(os.path.join(GOLD, "cxr_cases.npz")) as z:
        srcs = {f"cxr.{k}": z[f"src.{k}"] for k in ("A", "E")}
    with np.load(os.path.join(GOLD, "cxr_aug_cases.npz")) as z:
        srcs.update({f"aug.{k}": z[f"src.{k}"] for k in ("P", "Q", "R")})
    for k, a in srcs.items():
        data = encode(a, quality=75)
        store[f"file.{k}"] = np.frombuffer(data, np.uint8)
        store[f"pix.{k}"] = decode(data)
    return store


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(GOLD, "jpeg_cases.npz")
    store = build()
    np.savez_compressed(out, **store)
    print("cases", list(store["names"]), "bytes", os.path.getsize(out))
    for n in store["names"]:
        print(f"  {n}: {store[f'file.{n}'].size} file bytes, {store[f'pix.{n}'].shape}")


if __name__ == "__main__":
    main()
