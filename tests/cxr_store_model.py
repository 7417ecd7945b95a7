"""The image store's two kernels (csrc/jpeg.hip: mtmp_jpeg_sync_points, mtmp_jpeg_store_entropy) in plain Python, on the host
half of a builder/data/cxr_store.CxrStore and tests/jpeg_model.span: the sync rows a sequential decode of every segment gives
(the fixed point the device's rounds reach), and the decode of a batch from such rows -- one span per subsequence, no rounds."""
import numpy as np

from medical_tri_modal_pilot_amd.builder.data import cxr_store as CS
from medical_tri_modal_pilot_amd.builder.data import jpeg as J
from tests import jpeg_model


def _segment(store, i, k):
    """(bytes, blocks, dc table, ac table, subsequence length, first sync row) of segment k of image i"""
    d, t = store.rows[i], store.segs[int(store.rows[i, J.JPG_SEG0]) + k]
    off = int(store.wide[i, CS.WIDE_STREAM]) + int(t[CS.TSEG_OFF])
    seg = store.streams[off:off + int(t[CS.TSEG_BYTES])].tobytes()
    left = int(d[J.JPG_NBLK]) - int(t[CS.TSEG_BLOCK0])
    nb = min(int(d[J.JPG_RI]), left) if d[J.JPG_RI] else left
    dc = store.tables[d[J.JPG_DC]:d[J.JPG_DC] + J.HUFF_WORDS]
    ac = store.tables[d[J.JPG_AC]:d[J.JPG_AC] + J.HUFF_WORDS]
    return seg, nb, dc, ac, int(d[CS.JPG_SUBSEQ]), int(store.wide[i, CS.WIDE_SYNC0]) + int(t[CS.TSEG_SYNC0])


def sync_rows(store):
    """(int32 [n_sync, 4], status int32 [n]): every segment decoded once from its start, subsequence by subsequence"""
    sync = np.zeros((store.n_sync, CS.SYNC_WORDS), np.int32)
    status = np.zeros(store.n_images, np.int32)
    for i in range(store.n_images):
        for k in range(int(store.rows[i, J.JPG_NSEG])):
            seg, nb, dc, ac, S, row = _segment(store, i, k)
            nbits = len(seg) * 8
            p = c = blk = pred = 0
            for j in range(max(-(-nbits // S), 1)):
                sync[row + j] = ((p << 6) | c, blk, pred, k)
                p, c, nblk, dcs = jpeg_model.span(seg, nbits, dc, ac, p, c, min((j + 1) * S, nbits))
                blk, pred = blk + nblk, pred + dcs
            if blk < nb:
                status[i] |= jpeg_model.STATUS_SHORT
    return sync, status


def decode(store, sync, indices):
    """[uint8 [h, w]] of images ``indices``: per sync row ONE span from its entry state, then the inverse DCT"""
    out = []
    for i in indices:
        d = store.rows[i]
        h, w, bpr, nblk = (int(d[c]) for c in (J.JPG_H, J.JPG_W, J.JPG_BPR, J.JPG_NBLK))
        coef = np.zeros((nblk, 64), np.int16)
        for l in range(int(d[CS.JPG_NSYNC])):
            state, blk, pred, k = (int(v) for v in sync[int(store.wide[i, CS.WIDE_SYNC0]) + l])
            seg, nb, dc, ac, S, row = _segment(store, i, k)
            j = int(store.wide[i, CS.WIDE_SYNC0]) + l - row
            b0 = int(store.segs[int(d[J.JPG_SEG0]) + k, CS.TSEG_BLOCK0])
            jpeg_model.span(seg, len(seg) * 8, dc, ac, state >> 6, state & 63, min((j + 1) * S, len(seg) * 8),
                            coef[b0:b0 + nb], blk, pred, nb)
        px = jpeg_model.idct_blocks(coef, store.tables[d[J.JPG_QT]:d[J.JPG_QT] + 64])
        out.append(px.reshape(nblk // bpr, bpr, 8, 8).transpose(0, 2, 1, 3).reshape(nblk // bpr * 8, bpr * 8)[:h, :w])
    return out


import functools  # noqa: E402

SUBSEQ_BITS = (None, 32, 128)         # the image's own length, and two forced ones


@functools.lru_cache(maxsize=None)
def golden_store(bits=None):
    """The host half of the store of the 13 golden files (tests/golden/jpeg_cases.npz), never moved to a device."""
    from tests import jpeg_cases
    names = jpeg_cases.names()
    return CS.CxrStore.from_files([jpeg_cases.file_of(n) for n in names], bits, names)


@functools.lru_cache(maxsize=None)
def golden_sync(bits=None):
    """(sync rows, status) of ``golden_store(bits)``: computed once, shared, never written to"""
    return sync_rows(golden_store(bits))
