"""Chest X-ray input chain as a launch plan for the HIP kernels of csrc/image_prep.hip.

Reference behaviour restated here (file:line in the reference's builder/data/dataset_new.py):
  * :2094-2096, :2110-2112  ``F_t.equalize(image)`` then ``self.transform(image)`` for every image of a sample;
  * :91-120                 the train chains ``resize`` (Resize(S), CenterCrop(S)), ``resize_crop`` (Resize(round(1.142 S)),
                            CenterCrop(S)) and ``resize_affine_crop`` (the same with RandomAffine(5, translate .15, scale
                            .85-1.15) in front of the crop), each closed by ToTensor;
  * :122-160                the test chains ``center`` (= train ``resize``), ``resize_crop`` and ``resize``
                            (Resize((S, S)), no crop);
  * :2085-2087, :2116-2118  a slot without an image is ``torch.zeros(image_size)``.
What is NOT restated: ``random`` / ``randaug`` (:60-89, RandomResizedCrop and RandAugment) and ``resize_larger`` (the reference
names a function for it that it never defines) raise NotImplementedError; JPEG decoding stays with the loader.

All of the chain is integer arithmetic in PIL (ImageOps.equalize, the 22-bit fixed-point antialiased bilinear resize with a
uint8 rounding between its two passes, the 16.16 fixed-point nearest-neighbour affine map), so the kernels reproduce it bit
for bit.  This module holds the host half: which sizes, which coefficient tables, which affine words, which crop -- written
into one int32 descriptor row per image (``DESC_*``), which is all the kernels read.  Two things rest on torchvision's
documented behaviour only (it is not a dependency here): the inverse affine matrix of ``affine_matrix`` and the draw order
of ``draw_affine`` (RandomAffine.get_params: angle, tx, ty, scale, each one ``torch.empty(1).uniform_(lo, hi)``).
"""
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

PRECISION_BITS = 22                 # PIL's 8-bit resampling: 32 - 8 - 2
TILE_ROWS, TILE_COLS = 32, 64       # output tile of one workgroup of mtmp_cxr_resize (csrc/image_prep.hip)
RESIZE_LDS_LIMIT = 60 * 1024        # bytes of horizontal-pass rows one workgroup may hold

# int32 words of one descriptor row (include/mtmp.h, mtmp_cxr_*)
DESC_WORDS = 24
(DESC_SRC, DESC_H, DESC_W, DESC_RH, DESC_RW, DESC_HB, DESC_HK, DESC_HKS, DESC_VB, DESC_VK, DESC_VKS, DESC_FLAGS,
 DESC_A0, DESC_A1, DESC_A2, DESC_A3, DESC_A4, DESC_A5, DESC_TOP, DESC_LEFT, DESC_SLOT, DESC_SCRATCH) = range(22)
FLAG_AFFINE = 1

TRAIN_KINDS = ("resize", "resize_crop", "resize_affine_crop")
TEST_KINDS = ("center", "resize_crop", "resize")
_NOT_BUILT = {"random": "RandomResizedCrop is not built", "randaug": "RandAugment is not built",
              "resize_larger": "the reference names a transform for it that it never defines"}


def resize_coeffs(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """PIL's precompute_coeffs + normalize_coeffs_8bpc for the bilinear (triangle) filter on one axis.
    Returns (bounds int32 [out, 2] = (first source index, taps), coeffs int32 [out, ksize], unused taps zero)."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss)) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, xmax)
        kk[xx, :xmax] = [int(0.5 + v * (1 << PRECISION_BITS)) for v in w]
    return bounds, kk


_coeff_cache = {}


def cached_coeffs(in_size: int, out_size: int):
    key = (int(in_size), int(out_size))
    if key not in _coeff_cache:
        _coeff_cache[key] = resize_coeffs(*key)
    return _coeff_cache[key]


def affine_matrix(w: int, h: int, angle: float, tx: float, ty: float, scale: float) -> List[float]:
    """torchvision's inverse matrix (output pixel -> source pixel) for centre (w/2, h/2) and no shear."""
    cx, cy = w * 0.5, h * 0.5
    r = math.radians(angle)
    m = [math.cos(r) / scale, math.sin(r) / scale, 0.0, -math.sin(r) / scale, math.cos(r) / scale, 0.0]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def _fix(v: float) -> int:
    return int(math.floor(v * 65536.0 + 0.5))


def affine_words(m: Sequence[float]) -> List[int]:
    """The six 16.16 words of PIL's nearest-neighbour affine: xin = (a2 + a0 x + a1 y) >> 16, yin = (a5 + a3 x + a4 y) >> 16."""
    return [_fix(m[0]), _fix(m[1]), _fix(m[2] + m[0] * 0.5 + m[1] * 0.5),
            _fix(m[3]), _fix(m[4]), _fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]


AFFINE_DEGREES, AFFINE_TRANSLATE, AFFINE_SCALE = 5.0, (0.15, 0.15), (0.85, 1.15)


def draw_affine(w: int, h: int, generator: Optional[torch.Generator] = None) -> Tuple[float, int, int, float]:
    """(angle, tx, ty, scale) in RandomAffine.get_params' order: four ``uniform_`` draws of one element each."""
    def u(lo, hi):
        return float(torch.empty(1).uniform_(lo, hi, generator=generator).item())
    angle = u(-AFFINE_DEGREES, AFFINE_DEGREES)
    max_dx, max_dy = float(AFFINE_TRANSLATE[0] * w), float(AFFINE_TRANSLATE[1] * h)
    tx = int(round(u(-max_dx, max_dx)))
    ty = int(round(u(-max_dy, max_dy)))
    return angle, tx, ty, u(*AFFINE_SCALE)


class CxrTransform:
    """One of the reference's transform chains for images of ``image_size`` (S): sizes, crop and whether an affine is drawn."""

    def __init__(self, image_size: int, kind: str, train: bool):
        if kind in _NOT_BUILT:
            raise NotImplementedError(f"image transform '{kind}': {_NOT_BUILT[kind]}")
        if kind not in (TRAIN_KINDS if train else TEST_KINDS):
            raise ValueError(f"unknown image {'train' if train else 'test'} transform '{kind}'")
        self.image_size, self.kind, self.train = int(image_size), kind, bool(train)
        self.affine = train and kind == "resize_affine_crop"
        self.square = (not train) and kind == "resize"                      # Resize((S, S)), no crop
        larger = kind in ("resize_crop", "resize_affine_crop")
        self.resize_to = round(self.image_size * 1.142) if larger else self.image_size

    @classmethod
    def from_args(cls, args, train: bool) -> "CxrTransform":
        return cls(int(args.image_size), args.image_train_type if train else args.image_test_type, train)

    def resized(self, h: int, w: int) -> Tuple[int, int]:
        """(Rh, Rw) of torchvision's Resize: the short side goes to n, the long side to int(n long / short)."""
        n = self.resize_to
        if self.square:
            return n, n
        if w <= h:
            return int(n * h / w), n
        return n, int(n * w / h)

    def crop(self, rh: int, rw: int) -> Tuple[int, int]:
        """CenterCrop's (top, left) with Python's round."""
        if self.square:
            return 0, 0
        s = self.image_size
        return int(round((rh - s) / 2.0)), int(round((rw - s) / 2.0))


class RawCxrBatch:
    """uint8 source pixels of a batch plus everything ``ops.cxr_prepare`` needs to turn them into the float batch.

    pixels    uint8 [bytes]       the present images back to back (the four tensors are pinned when a GPU is present)
    desc      int32 [max(n, 1), DESC_WORDS]
    tables    int32 [words]       bound and coefficient tables, one set per distinct (in, out) pair of the batch
    slot_map  int32 [B K]         image index of every output slot, -1 for a slot without an image
    img_time  float32 [B] | [B, K]
    """

    def __init__(self, pixels, desc, tables, slot_map, img_time, image_size, batch, n_images, scratch_bytes, max_pixels,
                 max_rh, max_rw, lds_rows, params):
        self.pixels, self.desc, self.tables, self.slot_map, self.img_time = pixels, desc, tables, slot_map, img_time
        self.image_size, self.batch, self.n_images = int(image_size), int(batch), int(n_images)
        self.scratch_bytes, self.max_pixels, self.max_rh, self.max_rw = int(scratch_bytes), int(max_pixels), int(max_rh), int(max_rw)
        self.lds_rows = int(lds_rows)
        self.params = params             # per image (angle, tx, ty, scale) or None: what was drawn at collate time

    @property
    def n(self) -> int:
        """images present (a batch without any keeps one zero descriptor row that no slot points to)"""
        return len(self.params)

    @property
    def out_shape(self):
        s = self.image_size
        return (self.batch, self.n_images, 1, s, s) if self.n_images else (self.batch, 1, s, s)

    def to(self, device, non_blocking: bool = False) -> "RawCxrBatch":
        mv = lambda t: t.to(device, non_blocking=non_blocking)
        return RawCxrBatch(mv(self.pixels), mv(self.desc), mv(self.tables), mv(self.slot_map), self.img_time, self.image_size,
                           self.batch, self.n_images, self.scratch_bytes, self.max_pixels, self.max_rh, self.max_rw,
                           self.lds_rows, self.params)


def _tile_rows_needed(vb: np.ndarray) -> int:
    """Most source rows any tile of TILE_ROWS output rows reads (bounds are monotonic in the output index)."""
    worst = 0
    for r0 in range(0, vb.shape[0], TILE_ROWS):
        r1 = min(r0 + TILE_ROWS, vb.shape[0]) - 1
        worst = max(worst, int(vb[r1, 0] + vb[r1, 1] - vb[r0, 0]))
    return worst


def collate_raw_cxr(samples, transform: CxrTransform, n_images: int, generator: Optional[torch.Generator] = None,
                    affine_params=None) -> RawCxrBatch:
    """samples: one ``(images, times)`` pair per sample.  n_images = K > 0: the multi-image layout [B, K, 1, S, S] (absent
    slots zero, their time 10); n_images = 0: one image per sample, [B, 1, S, S] (absent: zeros, time -1).
    affine_params: per image ``(angle, tx, ty, scale)`` in batch order instead of drawing them (tests)."""
    K = int(n_images)
    B = len(samples)
    per = max(K, 1)
    S = transform.image_size
    rows, chunks, params = [], [], []
    tab_off, tab_parts, tab_words = {}, [], 0
    slot_map = np.full(B * per, -1, np.int32)
    img_time = np.full((B, per), 10.0 if K else -1.0, np.float32)
    src_off = scratch_off = max_pixels = max_rh = max_rw = lds_rows = 0

    def table(in_size, out_size):
        nonlocal tab_words
        key = (in_size, out_size)
        if key not in tab_off:
            b, k = cached_coeffs(in_size, out_size)
            tab_off[key] = (tab_words, tab_words + b.size, k.shape[1])
            tab_parts.extend([b.ravel(), k.ravel()])
            tab_words += b.size + k.size
        return tab_off[key]

    for b, (images, times) in enumerate(samples):
        if len(images) > per or len(images) != len(times):
            raise ValueError(f"sample {b}: {len(images)} images, {len(times)} times, {per} slots")
        for j, (im, t) in enumerate(zip(images, times)):
            im = np.ascontiguousarray(im)
            if im.dtype != np.uint8 or im.ndim != 2 or im.size == 0:
                raise ValueError(f"sample {b} image {j}: a non-empty uint8 [h, w] array is required")
            h, w = im.shape
            rh, rw = transform.resized(h, w)
            top, left = transform.crop(rh, rw)
            if top < 0 or left < 0 or top + S > rh or left + S > rw:
                raise ValueError(f"sample {b} image {j}: the {S} x {S} crop leaves the {rh} x {rw} map")
            d = np.zeros(DESC_WORDS, np.int64)
            d[[DESC_SRC, DESC_H, DESC_W, DESC_RH, DESC_RW]] = (src_off, h, w, rh, rw)
            d[[DESC_HB, DESC_HK, DESC_HKS]] = table(w, rw)
            d[[DESC_VB, DESC_VK, DESC_VKS]] = table(h, rh)
            if transform.affine:
                p = affine_params[len(rows)] if affine_params is not None else draw_affine(rw, rh, generator)
                d[DESC_FLAGS] = FLAG_AFFINE
                a = affine_words(affine_matrix(rw, rh, *p))
                if max(abs(a[2]) + abs(a[0]) * rw + abs(a[1]) * rh, abs(a[5]) + abs(a[3]) * rw + abs(a[4]) * rh) >= 2 ** 31:
                    raise ValueError(f"sample {b} image {j}: the 16.16 affine map of a {rh} x {rw} map leaves 32 bits")
                d[DESC_A0:DESC_A5 + 1] = a
                params.append(tuple(p))
            else:
                params.append(None)
            d[[DESC_TOP, DESC_LEFT, DESC_SLOT, DESC_SCRATCH]] = (top, left, b * per + j, scratch_off)
            slot_map[b * per + j] = len(rows)
            img_time[b, j] = t
            rows.append(d)
            chunks.append(im.ravel())
            src_off += h * w
            scratch_off += rh * rw
            max_pixels, max_rh, max_rw = max(max_pixels, h * w), max(max_rh, rh), max(max_rw, rw)
            lds_rows = max(lds_rows, _tile_rows_needed(cached_coeffs(h, rh)[0]))
    desc = np.stack(rows) if rows else np.zeros((1, DESC_WORDS), np.int64)
    if max(src_off, scratch_off, tab_words, B * per * S * S) >= 2 ** 31 or (rows and np.abs(desc).max() >= 2 ** 31):
        raise ValueError("collate_raw_cxr: the batch does not fit 32-bit offsets")
    if lds_rows * TILE_COLS > RESIZE_LDS_LIMIT:
        raise ValueError(f"collate_raw_cxr: a tile of {TILE_ROWS} resized rows reads {lds_rows} source rows (limit "
                         f"{RESIZE_LDS_LIMIT // TILE_COLS}): reduce the image before it is handed over")
    pin = torch.cuda.is_available()       # all four tensors pinned: RawCxrBatch.to(device, non_blocking=True) then never waits

    def host(a, dtype):
        t = torch.empty(a.shape, dtype=dtype, pin_memory=pin)
        t.copy_(torch.from_numpy(a))
        return t
    pixels = host(np.concatenate(chunks) if chunks else np.zeros(1, np.uint8), torch.uint8)
    tables = host(np.concatenate(tab_parts).astype(np.int32) if tab_parts else np.zeros(1, np.int32), torch.int32)
    t_img = torch.from_numpy(img_time if K else img_time[:, 0].copy())
    return RawCxrBatch(pixels, host(desc.astype(np.int32), torch.int32), tables, host(slot_map, torch.int32), t_img, S, B, K,
                       scratch_off, max_pixels, max_rh, max_rw, lds_rows, params)
