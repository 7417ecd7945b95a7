"""The dropout mask of the kernels, replayed on the host: written from the comment above dropout_keep4 in csrc/common.hip.h (a
counter hash, no state), in vectorised numpy uint32 with wrap-around.  Nothing here imports the HIP library.

    threshold(p)    thr = 0 for p <= 0, else int(float64(float32(p)) * 65536 + 0.5): a 16-bit field is kept iff field >= thr
    keep_scale(p)   the float32 value 1 / (1 - float32(p)), formed in fp32 as the kernels form it.  Every chain, float64 and fp32
                    alike, multiplies by this ONE value, so both sides of a comparison get the same bits
    element e of a contiguous tensor: group g = e >> 2, field number e & 3
        x = fmix32((g * 0x9E3779B1) ^ seed_eff)          fmix32: the 32-bit murmur3 finaliser
        y = x * 0x27D4EB2F;  y ^= y >> 15                one more mixing round for the upper pair
        fields 0..3 = x & 0xFFFF, x >> 16, y & 0xFFFF, y >> 16
        seed_eff = seed ^ (word & 0xFFFFFFFF) when a device seed word is set (ops.set_seed_word), else seed

Where the kernels put the mask (read from the code; the models of gemm_model.py / row_kernels_model.py take a Keep):
    GEMM epilogues (ln_gemm_kernel, ln_gemm_dma_kernel, gemm_nt_kernel): element row * N + col of the [M, N] output, whatever its
        row stride; v = act(acc + bias) in fp32, then keep ? v * keep_scale : 0, then the rounding to T, then gate / row scale / residual
    dropout_bwd_kernel and the operand drop of the gated dH launch: element of the contiguous tensor; T(float32(g) * keep_scale) or 0
    stream input: element (b (N + 1) + t) * 256 + col -- CLS and token rows only, the bottleneck rows are not counted and not masked;
        after LayerNorm + PE, in front of the one rounding of the store; backward: g = keep ? g * keep_scale : 0 in front of the
        LayerNorm backward

FAULTS: mistakes a kernel could make, as masks (faulty_keep) or as a switch of a model (`fault=`), for tests/test_dropout_model_cpu.py.
"""
from collections import namedtuple

import numpy as np
import torch

GOLDEN = 0x9E3779B1
M32 = 0xFFFFFFFF

Keep = namedtuple("Keep", "mask scale")          # mask: torch bool tensor, scale: keep_scale(p) as a Python float

MASK_FAULTS = ("ld_indexed", "fields_hi_lo", "other_seed", "word_ignored", "gt_for_ge")
MODEL_FAULTS = ("no_scale", "scale_after_round", "behind_residual")
STREAM_FAULTS = ("bwd_shifted_group", "bott_masked", "bott_counted")
FAULTS = MASK_FAULTS + MODEL_FAULTS + STREAM_FAULTS


def threshold(p):
    if p <= 0:
        return 0
    return int(float(np.float32(p)) * 65536.0 + 0.5)


def keep_scale(p):
    one = np.float32(1.0)
    return float(one / (one - np.float32(p)))


def seed_eff(seed, word=None):
    seed = int(seed) & M32
    return seed if word is None else seed ^ (int(word) & M32)


def _u32(a):
    return np.asarray(a, dtype=np.uint64).astype(np.uint32)


def fmix32(h):
    """the murmur3 finaliser on a uint32 array"""
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def group_fields(groups, seed, word=None):
    """uint32 [..., 4]: the four 16-bit fields of every group number"""
    x = fmix32((_u32(groups) * np.uint32(GOLDEN)) ^ np.uint32(seed_eff(seed, word)))
    y = x * np.uint32(0x27D4EB2F)
    y = y ^ (y >> np.uint32(15))
    return np.stack([x & np.uint32(0xFFFF), x >> np.uint32(16), y & np.uint32(0xFFFF), y >> np.uint32(16)], -1)


def fields_of(elements, seed, word=None, order=(0, 1, 2, 3)):
    """the 16-bit field of every element number (any shape, values < 2^32) -> uint32 array of that shape.  order: which of the
    group's four fields element 4g + i takes (the kernels': 0 1 2 3)"""
    e = _u32(elements)
    four = group_fields(e >> np.uint32(2), seed, word)
    pick = np.asarray(order, dtype=np.int64)[(e & np.uint32(3)).astype(np.int64)]
    return np.take_along_axis(four, pick[..., None], -1)[..., 0]


def keep_of_elements(elements, p, seed, word=None, order=(0, 1, 2, 3), strict=False):
    """bool array: the keep decision of every element number.  strict: field > thr (the fault), else field >= thr"""
    f, thr = fields_of(elements, seed, word, order), np.uint32(threshold(p))
    return torch.from_numpy(np.ascontiguousarray(f > thr if strict else f >= thr))


def elements(shape):
    """the element numbers of a contiguous tensor"""
    n = int(np.prod(shape))
    assert 0 < n <= 1 << 32, shape
    return np.arange(n, dtype=np.uint64).reshape(shape)


def contiguous_fields(shape, seed, word=None):
    """fields_of(elements(shape)) with one hash per group: the fields of groups 0, 1, .. laid end to end"""
    n = int(np.prod(shape))
    assert 0 < n <= 1 << 32, shape
    return group_fields(np.arange((n + 3) // 4, dtype=np.uint64), seed, word).reshape(-1)[:n].reshape(shape)


def keep_mask(shape, p, seed, word=None):
    return torch.from_numpy(contiguous_fields(shape, seed, word) >= np.uint32(threshold(p)))


def keep(shape, p, seed, word=None):
    """what the models take: the mask and the one scale"""
    return Keep(keep_mask(shape, p, seed, word), keep_scale(p))


def stream_input_elements(B, N, nb=0):
    """[B, N + 1, 256]: element numbers of the stream input's LayerNorm rows, row b (N + 1) + t of 256 columns (t = 0: CLS).  The nb
    bottleneck rows in front of each sample are NOT counted; nb > 0 gives the numbering of the fault that counts them."""
    b, t, c = np.meshgrid(np.arange(B, dtype=np.uint64), np.arange(N + 1, dtype=np.uint64), np.arange(256, dtype=np.uint64), indexing="ij")
    return (b * np.uint64(nb + N + 1) + np.uint64(nb) + t) * np.uint64(256) + c


def equal_fields(shape, p, seed, word=None):
    """bool array: the elements whose field EQUALS the threshold -- the only ones that `>` for `>=` decides differently"""
    return torch.from_numpy(contiguous_fields(shape, seed, word) == np.uint32(threshold(p)))


def faulty_keep(fault, shape, p, seed, word=None, ld=None, other_seed=None):
    """the Keep a kernel with one of MASK_FAULTS would apply to a contiguous [M, N] tensor"""
    assert fault in MASK_FAULTS, fault
    if fault == "ld_indexed":                          # row * ld + col for row * N + col
        M, N = shape
        e = np.arange(M, dtype=np.uint64)[:, None] * np.uint64(ld) + np.arange(N, dtype=np.uint64)[None, :]
        m = keep_of_elements(e, p, seed, word)
    elif fault == "fields_hi_lo":                      # each 32-bit word's halves swapped
        m = keep_of_elements(elements(shape), p, seed, word, order=(1, 0, 3, 2))
    elif fault == "other_seed":
        m = keep_mask(shape, p, other_seed, word)
    elif fault == "word_ignored":
        m = keep_mask(shape, p, seed, None)
    else:
        m = keep_of_elements(elements(shape), p, seed, word, strict=True)
    return Keep(m, keep_scale(p))


def shifted_group(mask):
    """the mask a backward would apply that regenerates it one group (four elements) late"""
    flat = mask.reshape(-1)
    return torch.cat([flat[-4:], flat[:-4]]).reshape(mask.shape)


# ------------------------------------------------------------------------------------------ the cases of the GPU file
#                 M,   N,    K,   options (those of gemm_model.nt_inputs / test_gemm_model_gpu.NT_CASES)
NT_DROP_CASES = [
    (64, 128, 64, dict(res=True, ldr=136)),                                # residual rows wider than N
    (65, 160, 72, dict(act="gelu", lda=88)),                               # no phase 2: the masked value IS the store; N tail inside a block
    (129, 96, 192, dict(res=True, lda=208, ldr=104, act="relu")),
    (63, 256, 1024, dict(res=True)),                                       # the FFN2 shape: nk 16
    (8064, 1024, 72, dict(res=True)),                                      # the last 64-row launch
    (8193, 1024, 72, dict(res=True)),                                      # 128-row tiles, the last one with one row
]
NT_LIVE_CASE = (129, 160, 200, dict(act="gelu", row_scale=49, res=True, ldr=168), 65)       # ... and the rows in use
NT_WINDOW_CASE = (65, 160, 72, dict(res=True), 176)                        # ... and ldy: y is a column window of a wider buffer
STREAM_DROP_CASES = [(2, 5, 1, False), (3, 37, 4, True), (7, 146, 4, False)]
STREAM_SEED, FFN1_SEED, FFN2_SEED = 4242, 77, 78
STREAMS3 = dict(B=3, nb=4, K=2, Ns=(37, 14, 9), kv=(42, 10, 25), seeds=(17, 18, 19))        # ops.StreamInputsFn: three streams, stream 0 packed

# ------------------------------------------------------------------------------------------ seeds with a field equal to the threshold
P = 0.1
WORD = 0x5DEECE66D1234567                               # a seed word with bits above bit 31 set: only its low half may count
FFN1_M = (1, 33, 128, 129, 257)
# per FFN1 shape [M, 1024] at p = 0.1 the first seed >= 1000 with an element whose field equals the threshold AND whose reference
# output is well above zero (find_seeds_eq, on the CPU; pinned by tests/test_dropout_model_cpu.py)
SEEDS_EQ = {1: 1085, 33: 1004, 128: 1000, 129: 1007, 257: 1000}


def find_seed_eq(shape, p, matters, start=1000, limit=100000):
    """the first seed >= start with an element where the field equals the threshold and `matters` (bool, of `shape`) holds"""
    for s in range(start, start + limit):
        if bool((equal_fields(shape, p, s) & matters).any()):
            return s
    raise AssertionError(f"no seed in [{start}, {start + limit}) for {shape}")
