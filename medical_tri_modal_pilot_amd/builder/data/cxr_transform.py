"""Chest X-ray input chain as a launch plan for the HIP kernels of csrc/image_prep.hip.

Reference behaviour restated here (file:line in the reference's builder/data/dataset_new.py):
  * :2094-2096, :2110-2112  ``F_t.equalize(image)`` then ``self.transform(image)`` for every image of a sample;
  * :91-120                 the train chains ``resize`` (Resize(S), CenterCrop(S)), ``resize_crop`` (Resize(round(1.142 S)),
                            CenterCrop(S)) and ``resize_affine_crop`` (the same with RandomAffine(5, translate .15, scale
                            .85-1.15) in front of the crop), each closed by ToTensor;
  * :122-160                the test chains ``center`` (= train ``resize``), ``resize_crop`` and ``resize``
                            (Resize((S, S)), no crop);
  * :2085-2087, :2116-2118  a slot without an image is ``torch.zeros(image_size)``.
  * :60-89                  the train chains ``random`` (RandomResizedCrop(S, scale (0.8, 1.1), ratio (3/4, 4/3))) and ``randaug``
                            (RandAugment() in front of that crop): ``CxrRandomTransform``, see "The random chains" below.
What is NOT restated: ``resize_larger`` (the reference names a function for it that it never defines) raises
NotImplementedError.  ``transform_from_args`` picks the class for a set of flags.  An image may be handed over as the bytes
of its JPEG file instead of the decoded array: builder/data/jpeg.py plans its decoding (csrc/jpeg.hip), which then runs in front
of the chain on the device.  Or as ``store.image(i)``, a handle into a device-resident store of such files
(builder/data/cxr_store.py): nothing is parsed and no byte of it crosses the link.

All of the chain is integer arithmetic in PIL (ImageOps.equalize, the 22-bit fixed-point antialiased bilinear resize with a
uint8 rounding between its two passes, the 16.16 fixed-point nearest-neighbour affine map), so the kernels reproduce it bit
for bit.  This module holds the host half: which sizes, which coefficient tables, which affine words, which crop -- written
into one int32 descriptor row per image (``DESC_*``), which is all the kernels read.  Two things rest on torchvision's
documented behaviour only (it is not a dependency here): the inverse affine matrix of ``affine_matrix`` and the draw order
of ``draw_affine`` (RandomAffine.get_params: angle, tx, ty, scale, each one ``torch.empty(1).uniform_(lo, hi)``).

The random chains (csrc/image_aug.hip).  Per image: equalise, RandAugment's two ops (``randaug`` only), the crop box,
``img.crop((j, i, j + cw, i + ch)).resize((S, S), BILINEAR)``, ToTensor.  The resize tables are those of (cw -> S) and
(ch -> S), read through a window of the source; there is no centre crop.  What each RandAugment op is on an ``L`` image,
with the PIL call it is pinned to (bit-equal, tests/golden/cxr_aug_cases.npz):
  Identity, Color    nothing: ``ImageEnhance.Color`` blends an ``L`` image with itself
  ShearX / ShearY    ``img.transform(size, AFFINE, [1, t, 0, 0, 1, 0] / [1, 0, 0, t, 1, 0], NEAREST)``, t = the tangent of
                     ``radians(degrees(atan(m)))``, centre (0, 0): PIL's generic 16.16 affine routine (``affine_words``)
  TranslateX / Y     ``[1, 0, -int(m), 0, 1, 0]`` / ``[1, 0, 0, 0, 1, -int(m)]``: PIL takes its scale routine, which for these
                     matrices is an integer shift with zero fill -- the same 16.16 words give it
  Rotate             ``img.rotate(m, NEAREST)``: ``rotate_matrix`` restates the matrix Image.rotate builds (its
                     ``round(., 15)`` included), then the generic affine routine
  Brightness         ``ImageEnhance.Brightness(img).enhance(1 + m)`` = ``Image.blend(0, img, 1 + m)``: a 256-entry table
  Contrast           ``Image.blend(int(mean + .5), img, 1 + m)``: a table, the mean taken from the histogram
  Sharpness          ``Image.blend(img.filter(SMOOTH), img, 1 + m)``: SMOOTH is (1 1 1 / 1 5 1 / 1 1 1) / 13 rounded half up
                     in the interior and a copy on the one-pixel border
  Posterize          ``ImageOps.posterize(img, int(m))``: ``v & mask``
  Solarize           ``ImageOps.solarize(img, m)``: ``v if v < m else 255 - v``
  AutoContrast       ``ImageOps.autocontrast(img)``: ``int(v * (255.0 / (hi - lo)) - lo * (255.0 / (hi - lo)))`` in doubles,
                     clipped; the identity when ``hi <= lo``
  Equalize           ``ImageOps.equalize(img)``
``Image.blend(a, b, f)`` is ``a + f * (b - a)`` in float32 (f rounded to float32, the product rounded before the sum),
clipped to [0, 255] and truncated.  Geometric ops fill with 0.  Table ops cost no pass over the pixels: a chain of them
is one composed 256-entry table that the next kernel to read the image builds from the histogram (the counts pushed
through each table in turn); only geometric ops and Sharpness write a full-size uint8 map (a *stage*).  One int32
descriptor row of ``AUG_WORDS`` words per image (``AUG_*``) holds the plan.
torchvision is not a dependency and was not run: the device work is pinned against the PIL calls above, while the
parameter logic -- the draw order and magnitude tables of ``draw_randaug`` (RandAugment.forward / _augmentation_space),
``draw_resized_crop`` (RandomResizedCrop.get_params), which PIL call each op becomes and with which matrix
(``shear_matrix`` = _get_inverse_affine_matrix) -- rests on torchvision's published source.
"""
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .cxr_store import CxrImage
from .jpeg import is_jpeg_source, parse_jpeg, plan_jpegs

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
RANDOM_KINDS = ("random", "randaug")
_NOT_BUILT = {"random": "CxrRandomTransform holds this chain; build transforms with transform_from_args(args, train)",
              "randaug": "CxrRandomTransform holds this chain; build transforms with transform_from_args(args, train)",
              "resize_larger": "the reference names a transform for it that it never defines"}

# int32 words of one descriptor row of the random chains (include/mtmp.h, mtmp_cxr_aug_stage / mtmp_cxr_crop_resize)
AUG_WORDS = 64
(AUG_SRC, AUG_H, AUG_W, AUG_SLOT, AUG_SCR, AUG_I, AUG_J, AUG_CH, AUG_CW, AUG_HB, AUG_HK, AUG_HKS, AUG_VB, AUG_VK,
 AUG_VKS) = range(15)
# + 8 k: stage k = RandAugment op k + 1 when it writes a map: kind, then six affine words or the float32 bits of the blend factor
AUG_STAGE = 16
STAGE_NONE, STAGE_AFFINE, STAGE_SHARPNESS = 0, 1, 2
# + 8 r: what reader r (stage 0, stage 1, the resize) reads: base (0 source pixels, 1 + k map of stage k), number of pending table
# ops (<= 3), their three codes, their three parameters
AUG_READ = 32
(TABLE_EQUALIZE, TABLE_BRIGHTNESS, TABLE_CONTRAST, TABLE_POSTERIZE, TABLE_SOLARIZE, TABLE_AUTOCONTRAST) = range(1, 7)
RANDAUG_OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast",
               "Sharpness", "Posterize", "Solarize", "AutoContrast", "Equalize")
RANDAUG_SIGNED = frozenset(RANDAUG_OPS[1:10])
RANDAUG_BINS, RANDAUG_MAGNITUDE = 31, 9
CROP_SCALE, CROP_RATIO = (0.8, 1.1), (3.0 / 4.0, 4.0 / 3.0)


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
        if len(_coeff_cache) >= 4096:             # the random chains meet a new (crop side, S) pair with almost every image
            _coeff_cache.clear()
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


def draw_resized_crop(h: int, w: int, generator: Optional[torch.Generator] = None) -> Tuple[int, int, int, int]:
    """(i, j, ch, cw) as RandomResizedCrop.get_params draws it: up to ten attempts of two ``uniform_`` draws (area, log
    aspect; the log-ratio bounds and the exponential are float32 as there), an accepted attempt followed by two ``randint``
    draws; the centre fallback draws nothing more."""
    area = h * w
    log_ratio = torch.log(torch.tensor(CROP_RATIO))
    lo, hi = float(log_ratio[0]), float(log_ratio[1])
    for _ in range(10):
        target = area * torch.empty(1).uniform_(CROP_SCALE[0], CROP_SCALE[1], generator=generator).item()
        aspect = torch.exp(torch.empty(1).uniform_(lo, hi, generator=generator)).item()
        cw = int(round(math.sqrt(target * aspect)))
        ch = int(round(math.sqrt(target / aspect)))
        if 0 < cw <= w and 0 < ch <= h:
            i = int(torch.randint(0, h - ch + 1, size=(1,), generator=generator).item())
            j = int(torch.randint(0, w - cw + 1, size=(1,), generator=generator).item())
            return i, j, ch, cw
    in_ratio = float(w) / float(h)
    if in_ratio < min(CROP_RATIO):
        cw = w
        ch = int(round(cw / min(CROP_RATIO)))
    elif in_ratio > max(CROP_RATIO):
        ch = h
        cw = int(round(ch * max(CROP_RATIO)))
    else:
        cw, ch = w, h
    return (h - ch) // 2, (w - cw) // 2, ch, cw


def randaug_magnitude(op: str, h: int, w: int) -> float:
    """Bin 9 of the op's table in RandAugment._augmentation_space (float32 tensors, 31 bins); 0.0 for the ops without one."""
    n = RANDAUG_BINS
    if op in ("ShearX", "ShearY"):
        t = torch.linspace(0.0, 0.3, n)
    elif op == "TranslateX":
        t = torch.linspace(0.0, 150.0 / 331.0 * w, n)
    elif op == "TranslateY":
        t = torch.linspace(0.0, 150.0 / 331.0 * h, n)
    elif op == "Rotate":
        t = torch.linspace(0.0, 30.0, n)
    elif op in ("Brightness", "Color", "Contrast", "Sharpness"):
        t = torch.linspace(0.0, 0.9, n)
    elif op == "Posterize":
        t = 8 - (torch.arange(n) / ((n - 1) / 4)).round().int()
    elif op == "Solarize":
        t = torch.linspace(255.0, 0.0, n)
    else:
        return 0.0
    return float(t[RANDAUG_MAGNITUDE].item())


def draw_randaug(h: int, w: int, generator: Optional[torch.Generator] = None) -> List[Tuple[str, float]]:
    """Two ``(op, magnitude)`` pairs in RandAugment.forward's order: per op ``randint(14)``, then ``randint(2)`` for a signed
    op (1 negates)."""
    out = []
    for _ in range(2):
        op = RANDAUG_OPS[int(torch.randint(len(RANDAUG_OPS), (1,), generator=generator).item())]
        m = randaug_magnitude(op, h, w)
        if op in RANDAUG_SIGNED and int(torch.randint(2, (1,), generator=generator).item()):
            m *= -1.0
        out.append((op, m))
    return out


def shear_matrix(sx_deg: float, sy_deg: float) -> List[float]:
    """torchvision's inverse matrix for a pure shear about (0, 0): no rotation, no translation, scale 1."""
    sx, sy = math.radians(sx_deg), math.radians(sy_deg)
    a = math.cos(-sy) / math.cos(sy)
    b = -math.cos(-sy) * math.tan(sx) / math.cos(sy)
    c = math.sin(-sy) / math.cos(sy)
    d = -math.sin(-sy) * math.tan(sx) / math.cos(sy) + 1.0
    return [d, -b, 0.0, -c, a, 0.0]


def rotate_matrix(w: int, h: int, angle: float) -> Optional[List[float]]:
    """The matrix Image.rotate(angle) hands to Image.transform; None where it copies the image (a multiple of 360)."""
    angle = angle % 360.0
    if angle == 0:
        return None
    if angle == 180 or (angle in (90, 270) and w == h):
        raise ValueError("rotate_matrix: PIL transposes for this angle")
    cx, cy = w / 2, h / 2
    r = -math.radians(angle)
    m = [round(math.cos(r), 15), round(math.sin(r), 15), 0.0, round(-math.sin(r), 15), round(math.cos(r), 15), 0.0]
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def _f32_bits(v: float) -> int:
    return int(np.array([v], np.float32).view(np.int32)[0])


def plan_op(op: str, m: float, h: int, w: int):
    """One RandAugment op as the kernels see it: None (nothing), ("table", code, parameter), ("affine", six 16.16 words) or
    ("sharpness", float32 bits of the factor)."""
    if op in ("Identity", "Color"):
        return None
    if op in ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate"):
        if op == "ShearX":
            mat = shear_matrix(math.degrees(math.atan(m)), 0.0)
        elif op == "ShearY":
            mat = shear_matrix(0.0, math.degrees(math.atan(m)))
        elif op == "TranslateX":
            mat = [1.0, 0.0, -float(int(m)), 0.0, 1.0, 0.0]
        elif op == "TranslateY":
            mat = [1.0, 0.0, 0.0, 0.0, 1.0, -float(int(m))]
        else:
            mat = rotate_matrix(w, h, m)
        if mat is None or mat == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]:
            return None
        a = affine_words(mat)
        if max(abs(a[2]) + abs(a[0]) * w + abs(a[1]) * h, abs(a[5]) + abs(a[3]) * w + abs(a[4]) * h) >= 2 ** 31:
            raise ValueError(f"{op}: the 16.16 affine map of a {h} x {w} image leaves 32 bits")
        return ("affine", a)
    if op == "Brightness":
        return ("table", TABLE_BRIGHTNESS, _f32_bits(1.0 + m))
    if op == "Contrast":
        return ("table", TABLE_CONTRAST, _f32_bits(1.0 + m))
    if op == "Sharpness":
        return ("sharpness", _f32_bits(1.0 + m))
    if op == "Posterize":
        return ("table", TABLE_POSTERIZE, ~(2 ** (8 - int(m)) - 1) & 255)
    if op == "Solarize":
        return ("table", TABLE_SOLARIZE, int(math.ceil(m)))           # v < m for an integer v
    if op == "AutoContrast":
        return ("table", TABLE_AUTOCONTRAST, 0)
    if op == "Equalize":
        return ("table", TABLE_EQUALIZE, 0)
    raise ValueError(f"unknown RandAugment op '{op}'")


def plan_chain(ops: Sequence[Tuple[str, float]], h: int, w: int):
    """(stages, reads) of one image: stages[k] = the map op k writes or None; reads[r] = (base, pending table ops) of reader r
    (stage 0, stage 1, the resize), base 0 = the source pixels, 1 + k = the map of stage k.  The loader's equalisation opens
    the chain of the source pixels."""
    pending, base = [(TABLE_EQUALIZE, 0)], 0
    stages, reads = [None, None], [(0, []), (0, []), None]
    for k, (op, m) in enumerate(ops):
        st = plan_op(op, m, h, w)
        if st is None:
            continue
        if st[0] == "table":
            pending.append((st[1], st[2]))
        else:
            stages[k], reads[k] = st, (base, pending)
            pending, base = [], k + 1
    reads[2] = (base, pending)
    return stages, reads


class CxrRandomTransform:
    """The train chains ``random`` (RandomResizedCrop) and ``randaug`` (RandAugment, then that crop) for images of
    ``image_size`` (S)."""

    def __init__(self, image_size: int, kind: str):
        if kind not in RANDOM_KINDS:
            raise ValueError(f"CxrRandomTransform holds {RANDOM_KINDS}, not '{kind}'")
        self.image_size, self.kind, self.train = int(image_size), kind, True
        self.randaug = kind == "randaug"


def transform_from_args(args, train: bool):
    """The transform of ``--image-train-type`` / ``--image-test-type`` and ``--image-size``."""
    kind = args.image_train_type if train else args.image_test_type
    if train and kind in RANDOM_KINDS:
        return CxrRandomTransform(int(args.image_size), kind)
    return CxrTransform(int(args.image_size), kind, train)


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
    The random chains (``aug`` is not None) add
    aug       int32 [max(n, 1), AUG_WORDS]   their plan; ``desc`` then holds source offset, h, w and the slot only
    stages    bit k set: some image's RandAugment op k writes a map, so stage k is launched; ``scratch_bytes`` is one of the
              two maps' buffers, ``lds_rows`` belongs to the tables of the crop boxes
    Images handed over as JPEG file bytes add
    jpeg      builder/data/jpeg.JpegPlan | None   their streams, descriptor rows, segment rows and decode tables; their regions
              of ``pixels`` are left for ``ops.jpeg_decode`` to fill (``ops.cxr_prepare`` calls it)
    Images handed over as handles of a ``CxrStore`` add
    stored    builder/data/cxr_store.CxrStoreBatch | None   their store, indices, descriptor rows and lane prefix; filled by
              ``ops.jpeg_decode`` as well.  When EVERY present image is stored, ``pixels`` is None on the host and ``to(device)``
              allocates its ``pixel_bytes`` bytes there: no pixel byte crosses the link.
    """

    def __init__(self, pixels, desc, tables, slot_map, img_time, image_size, batch, n_images, scratch_bytes, max_pixels,
                 max_rh, max_rw, lds_rows, params, aug=None, stages=0, jpeg=None, stored=None, pixel_bytes=None):
        self.aug, self.stages, self.jpeg, self.stored = aug, int(stages), jpeg, stored
        self.pixel_bytes = int(pixels.numel() if pixel_bytes is None else pixel_bytes)
        self.pixels, self.desc, self.tables, self.slot_map, self.img_time = pixels, desc, tables, slot_map, img_time
        self.image_size, self.batch, self.n_images = int(image_size), int(batch), int(n_images)
        self.scratch_bytes, self.max_pixels, self.max_rh, self.max_rw = int(scratch_bytes), int(max_pixels), int(max_rh), int(max_rw)
        self.lds_rows = int(lds_rows)
        # per image what was drawn at collate time: (angle, tx, ty, scale) or None; the random chains: (ops, (i, j, ch, cw))
        self.params = params

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
        pixels = mv(self.pixels) if self.pixels is not None else torch.empty(self.pixel_bytes, dtype=torch.uint8, device=device)
        return RawCxrBatch(pixels, mv(self.desc), mv(self.tables), mv(self.slot_map), self.img_time, self.image_size,
                           self.batch, self.n_images, self.scratch_bytes, self.max_pixels, self.max_rh, self.max_rw,
                           self.lds_rows, self.params, None if self.aug is None else mv(self.aug), self.stages,
                           None if self.jpeg is None else self.jpeg.to(device, non_blocking=non_blocking),
                           None if self.stored is None else self.stored.to(device, non_blocking=non_blocking), self.pixel_bytes)


def _tile_rows_needed(vb: np.ndarray) -> int:
    """Most source rows any tile of TILE_ROWS output rows reads (bounds are monotonic in the output index)."""
    worst = 0
    for r0 in range(0, vb.shape[0], TILE_ROWS):
        r1 = min(r0 + TILE_ROWS, vb.shape[0]) - 1
        worst = max(worst, int(vb[r1, 0] + vb[r1, 1] - vb[r0, 0]))
    return worst


def _aug_row(im_h, im_w, ops, box, stages_reads, tabs):
    """The AUG_WORDS words of one image behind source offset, slot and scratch offset."""
    d = np.zeros(AUG_WORDS, np.int64)
    d[[AUG_H, AUG_W]] = (im_h, im_w)
    d[[AUG_I, AUG_J, AUG_CH, AUG_CW]] = box
    d[AUG_HB:AUG_VKS + 1] = tabs
    stages, reads = stages_reads
    for k, st in enumerate(stages):
        if st is None:
            continue
        o = AUG_STAGE + 8 * k
        if st[0] == "affine":
            d[o], d[o + 1:o + 7] = STAGE_AFFINE, st[1]
        else:
            d[o], d[o + 1] = STAGE_SHARPNESS, st[1]
    for r, (base, pend) in enumerate(reads):
        o = AUG_READ + 8 * r
        d[o], d[o + 1] = base, len(pend)
        for t, (code, par) in enumerate(pend):
            d[o + 2 + t], d[o + 5 + t] = code, par
    return d


def collate_raw_cxr(samples, transform, n_images: int, generator: Optional[torch.Generator] = None,
                    affine_params=None, aug_params=None, crop_params=None) -> RawCxrBatch:
    """samples: one ``(images, times)`` pair per sample.  n_images = K > 0: the multi-image layout [B, K, 1, S, S] (absent
    slots zero, their time 10); n_images = 0: one image per sample, [B, 1, S, S] (absent: zeros, time -1).
    affine_params: per image ``(angle, tx, ty, scale)`` in batch order instead of drawing them (tests).
    An image is a ``uint8 [h, w]`` array or the ``bytes`` / ``bytearray`` / ``memoryview`` of a baseline greyscale JPEG file
    (builder/data/jpeg.parse_jpeg says what is accepted; anything else raises -- the loader then decodes that file itself and
    passes the array).  The file's header gives h and w, so everything below is planned as for an array; the file's region of
    ``pixels`` is left zero and ``RawCxrBatch.jpeg`` holds what the device needs to fill it.
    Or it is ``store.image(i)`` of a ``CxrStore``: h and w come from the handle, nothing is parsed, ``RawCxrBatch.stored`` holds
    the plan; all handles of a batch must come from one store.  The three kinds may mix in one batch.
    A ``CxrRandomTransform`` draws per image, in the reference's order, the RandAugment ops (``randaug``) and then the crop
    box; aug_params: per image two ``(op, magnitude)`` pairs, crop_params: per image ``(i, j, ch, cw)``, instead (tests)."""
    rnd = isinstance(transform, CxrRandomTransform)
    aug_rows, stage_mask = [], 0
    K = int(n_images)
    B = len(samples)
    per = max(K, 1)
    S = transform.image_size
    rows, chunks, params = [], [], []
    tab_off, tab_parts, tab_words = {}, [], 0
    slot_map = np.full(B * per, -1, np.int32)
    img_time = np.full((B, per), 10.0 if K else -1.0, np.float32)
    src_off = scratch_off = max_pixels = max_rh = max_rw = lds_rows = 0
    jpg_infos, jpg_dst, jpg_rows, jpg_bytes = [], [], [], 0
    store, st_idx, st_dst, st_rows = None, [], [], []

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
            if isinstance(im, CxrImage):
                if store is not None and im.store is not store:
                    raise ValueError(f"sample {b} image {j}: the stored images of a batch must come from one CxrStore")
                store = im.store
                st_idx.append(im.index)
                st_dst.append(src_off)
                st_rows.append(len(rows))
                h, w = im.h, im.w
                im = None                                          # ops.jpeg_decode writes these bytes on the device
            elif is_jpeg_source(im):
                try:
                    info = parse_jpeg(im)
                except (ValueError, NotImplementedError) as e:
                    raise type(e)(f"sample {b} image {j}: {e}") from None
                jpg_infos.append(info)
                jpg_dst.append(src_off)
                jpg_rows.append(len(rows))
                jpg_bytes += memoryview(im).nbytes
                h, w = info.h, info.w
                im = np.zeros(h * w, np.uint8)                     # ops.jpeg_decode writes these bytes on the device
            else:
                im = np.ascontiguousarray(im)
                if im.dtype != np.uint8 or im.ndim != 2 or im.size == 0:
                    raise ValueError(f"sample {b} image {j}: a non-empty uint8 [h, w] array or the bytes of a JPEG file is required")
                h, w = im.shape
            if rnd:
                if transform.randaug:
                    ops = [(str(o), float(m)) for o, m in aug_params[len(rows)]] if aug_params is not None \
                        else draw_randaug(h, w, generator)
                else:
                    ops = []
                box = tuple(int(v) for v in crop_params[len(rows)]) if crop_params is not None \
                    else draw_resized_crop(h, w, generator)
                ci, cj, ch, cw = box
                if not (0 < ch and 0 < cw and 0 <= ci and 0 <= cj and ci + ch <= h and cj + cw <= w):
                    raise ValueError(f"sample {b} image {j}: the crop box {box} leaves the {h} x {w} image")
                plan = plan_chain(ops, h, w)
                a = _aug_row(h, w, ops, box, plan, table(cw, S) + table(ch, S))
                a[[AUG_SRC, AUG_SLOT, AUG_SCR]] = (src_off, b * per + j, scratch_off)
                d = np.zeros(DESC_WORDS, np.int64)
                d[[DESC_SRC, DESC_H, DESC_W, DESC_SLOT]] = (src_off, h, w, b * per + j)
                for k, st in enumerate(plan[0]):
                    stage_mask |= (st is not None) << k
                params.append((tuple(ops), box))
                slot_map[b * per + j] = len(rows)
                img_time[b, j] = t
                rows.append(d)
                aug_rows.append(a)
                chunks.append((h * w) if im is None else im.ravel())
                src_off += h * w
                scratch_off += (h * w + 15) // 16 * 16          # the stages store four pixels at a time
                max_pixels, max_rh, max_rw = max(max_pixels, h * w), S, S
                lds_rows = max(lds_rows, _tile_rows_needed(cached_coeffs(ch, S)[0]))
                continue
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
            chunks.append((h * w) if im is None else im.ravel())
            src_off += h * w
            scratch_off += rh * rw
            max_pixels, max_rh, max_rw = max(max_pixels, h * w), max(max_rh, rh), max(max_rw, rw)
            lds_rows = max(lds_rows, _tile_rows_needed(cached_coeffs(h, rh)[0]))
    desc = np.stack(rows) if rows else np.zeros((1, DESC_WORDS), np.int64)
    aug = (np.stack(aug_rows) if aug_rows else np.zeros((1, AUG_WORDS), np.int64)) if rnd else None
    if rnd and not stage_mask:
        scratch_off = 0
    if max(src_off, 2 * scratch_off, tab_words, B * per * S * S) >= 2 ** 31 or (rows and np.abs(desc).max() >= 2 ** 31):
        raise ValueError("collate_raw_cxr: the batch does not fit 32-bit offsets")
    if lds_rows * TILE_COLS > RESIZE_LDS_LIMIT:
        raise ValueError(f"collate_raw_cxr: a tile of {TILE_ROWS} resized rows reads {lds_rows} source rows (limit "
                         f"{RESIZE_LDS_LIMIT // TILE_COLS}): reduce the image before it is handed over")
    pin = torch.cuda.is_available()       # all four tensors pinned: RawCxrBatch.to(device, non_blocking=True) then never waits

    def host(a, dtype):
        t = torch.empty(a.shape, dtype=dtype, pin_memory=pin)
        t.copy_(torch.from_numpy(a))
        return t
    if st_rows and len(st_rows) == len(rows):             # every present image is stored: the pixel buffer exists on the device only
        pixels = None
    else:
        chunks = [np.zeros(c, np.uint8) if isinstance(c, int) else c for c in chunks]
        pixels = host(np.concatenate(chunks) if chunks else np.zeros(1, np.uint8), torch.uint8)
    tables = host(np.concatenate(tab_parts).astype(np.int32) if tab_parts else np.zeros(1, np.int32), torch.int32)
    t_img = torch.from_numpy(img_time if K else img_time[:, 0].copy())
    return RawCxrBatch(pixels, host(desc.astype(np.int32), torch.int32), tables, host(slot_map, torch.int32), t_img, S, B, K,
                       scratch_off, max_pixels, max_rh, max_rw, lds_rows, params,
                       None if aug is None else host(aug.astype(np.int32), torch.int32), stage_mask,
                       plan_jpegs(jpg_infos, jpg_dst, jpg_rows, jpg_bytes, pin) if jpg_infos else None,
                       store.batch(st_idx, st_dst, st_rows, pin) if st_rows else None, max(src_off, 1))
