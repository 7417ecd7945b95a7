"""Baseline greyscale JPEG files as a launch plan for the HIP kernels of csrc/jpeg.hip.

Every image the reference trains on is a JPEG that PIL wrote (1_mimic_cxr_preprocess.py:81-82 ``convert('L')`` + ``save()``:
8-bit, one component, baseline sequential, Huffman coded) and that its loader opens with ``Image.open`` inside ``__getitem__``
(builder/data/dataset_new.py:2094).  This module is the host half of decoding such files on the GPU: ``parse_jpeg`` reads the
markers of one file, ``plan_jpegs`` lays a batch of files out for the two kernels -- the entropy-coded bytes with the stuffed
``FF 00`` pairs and the RSTn markers taken out (one vectorised pass over the bytes), one int32 descriptor row per image
(``JPG_*``), one row per restart segment (``SEG_*``), and the quantisation and Huffman decode tables, shared between images that
carry the same payload.  What is NOT decoded is rejected by name: progressive (SOF2), extended / 12-bit (SOF1, precision),
arithmetic coding (SOF9.., DAC), more than one component, 16-bit quantisation tables.  There is no fallback: a loader that meets
such a file decodes it itself and hands over the array.

The arithmetic behind the entropy decoder is all integer and pinned to libjpeg's ``jpeg_idct_islow`` (csrc/jpeg.hip), so the
pixels equal ``PIL.Image.open`` bit for bit (tests/golden/jpeg_cases.npz).
"""
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

# int32 words of one image row (include/mtmp.h, mtmp_jpeg_*)
JPG_WORDS = 16
(JPG_STREAM, JPG_SEG0, JPG_NSEG, JPG_H, JPG_W, JPG_BPR, JPG_NBLK, JPG_DST, JPG_QT, JPG_DC, JPG_AC, JPG_COEF, JPG_RI) = range(13)
# int32 words of one segment row
SEG_WORDS = 4
SEG_OFF, SEG_BYTES, SEG_IMG, SEG_BLOCK0 = range(4)

LOOK_BITS = 10                        # codes of up to LOOK_BITS bits are decoded by one table read
# one Huffman decode table: look[1 << LOOK_BITS] ((code length << 8) | symbol, 0: longer than LOOK_BITS bits or no code),
# maxcode[18] (index = code length; -1: no code of that length; [17] = 0x7fffffff), valoff[18] (index of the first symbol of
# that length minus its first code), huffval[256]
HUFF_WORDS = (1 << LOOK_BITS) + 18 + 18 + 256
MAX_SUBSEQ = 1024                     # lanes of one workgroup of mtmp_jpeg_entropy
MAX_SEGMENT_BYTES = 1 << 22           # a bit position and the coefficient index share one 32-bit state word
MAX_STAGE_BYTES = 32 * 1024
DEFAULT_SUBSEQ_BITS = 1024            # the host's choice where a segment fits MAX_SUBSEQ subsequences of it (profiles/jpeg_decode.txt)

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60,
                   61, 54, 47, 55, 62, 63], np.int32)      # natural index of the k-th coefficient of the stream


class HuffSpec(NamedTuple):
    bits: Tuple[int, ...]             # 16 counts: codes of length 1..16
    vals: Tuple[int, ...]             # the symbols in code order


class JpegInfo(NamedTuple):
    h: int
    w: int
    qtable: np.ndarray                # int32 [64], natural (de-zigzagged) order
    dc: HuffSpec
    ac: HuffSpec
    restart_interval: int             # in blocks; 0: none
    ecs_offset: int                   # entropy-coded data in the file: first byte behind the SOS header ...
    ecs_length: int                   # ... up to EOI (or the end of a file that lacks it)
    segments: np.ndarray              # int64 [n, 2]: (offset, length) of every restart segment in the file, markers excluded
    stream: np.ndarray                # uint8: the segments back to back without stuffed zero bytes and without markers
    stream_segments: np.ndarray       # int64 [n, 2]: (offset, length) of every segment in ``stream``

    @property
    def blocks(self) -> Tuple[int, int]:
        return (self.h + 7) // 8, (self.w + 7) // 8


_SOF_NAMES = {0xC1: "SOF1 (extended sequential)", 0xC2: "SOF2 (progressive)", 0xC3: "SOF3 (lossless)",
              0xC5: "SOF5 (differential sequential)", 0xC6: "SOF6 (differential progressive)", 0xC7: "SOF7 (differential lossless)",
              0xC9: "SOF9 (arithmetic coding)", 0xCA: "SOF10 (arithmetic coding, progressive)",
              0xCB: "SOF11 (arithmetic coding, lossless)", 0xCD: "SOF13 (arithmetic coding)", 0xCE: "SOF14 (arithmetic coding)",
              0xCF: "SOF15 (arithmetic coding)"}


def _marker_name(m: int) -> str:
    if m == 0xC0:
        return "SOF0"
    if m == 0xC4:
        return "DHT"
    if m == 0xDB:
        return "DQT"
    if m == 0xDD:
        return "DRI"
    if m == 0xDA:
        return "SOS"
    if 0xE0 <= m <= 0xEF:
        return f"APP{m - 0xE0}"
    if m == 0xFE:
        return "COM"
    return f"marker FF{m:02X}"


def parse_jpeg(data) -> JpegInfo:
    """The markers of one baseline greyscale JPEG file (bytes, bytearray, memoryview or a uint8 array)."""
    d = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8).ravel()
    n = d.size
    if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise ValueError("parse_jpeg: SOI missing: not a JPEG file")
    pos = 2
    qt, huff, frame, ri = {}, {}, None, 0
    while True:
        if pos + 4 > n:
            raise ValueError(f"parse_jpeg: the header is truncated at byte {pos} in front of SOS")
        if d[pos] != 0xFF:
            raise ValueError(f"parse_jpeg: byte {pos} is {int(d[pos]):#04x} where a marker is expected")
        m = int(d[pos + 1])
        if m == 0xFF:                                 # fill byte in front of a marker
            pos += 1
            continue
        name = _marker_name(m)
        if m in _SOF_NAMES:
            raise NotImplementedError(f"parse_jpeg: {_SOF_NAMES[m]}: only baseline sequential Huffman files (SOF0) are decoded")
        if m == 0xCC:
            raise NotImplementedError("parse_jpeg: DAC (arithmetic coding) is not decoded")
        if m in (0xD8, 0xD9) or 0xD0 <= m <= 0xD7 or m == 0x01:
            raise ValueError(f"parse_jpeg: {name} at byte {pos} in front of SOS")
        L = (int(d[pos + 2]) << 8) | int(d[pos + 3])
        if L < 2 or pos + 2 + L > n:
            raise ValueError(f"parse_jpeg: {name} at byte {pos} is truncated ({L} bytes announced, {n - pos - 2} left)")
        p = d[pos + 4:pos + 2 + L]
        if m == 0xDB:
            i = 0
            while i < p.size:
                pq, tq = int(p[i]) >> 4, int(p[i]) & 15
                if pq != 0:
                    raise NotImplementedError(f"parse_jpeg: DQT table {tq} has 16-bit entries (12-bit files are not decoded)")
                if i + 65 > p.size:
                    raise ValueError(f"parse_jpeg: DQT at byte {pos} is truncated")
                nat = np.zeros(64, np.int32)
                nat[ZIGZAG] = p[i + 1:i + 65]
                qt[tq] = nat
                i += 65
        elif m == 0xC4:
            i = 0
            while i < p.size:
                if i + 17 > p.size:
                    raise ValueError(f"parse_jpeg: DHT at byte {pos} is truncated")
                tc, th = int(p[i]) >> 4, int(p[i]) & 15
                bits = tuple(int(v) for v in p[i + 1:i + 17])
                cnt = sum(bits)
                if tc > 1 or cnt > 256 or i + 17 + cnt > p.size:
                    raise ValueError(f"parse_jpeg: DHT at byte {pos}: bad table (class {tc}, {cnt} symbols)")
                code = 0
                for length, c in enumerate(bits, 1):
                    code = (code + c) << 1
                    if code > (1 << (length + 1)):
                        raise ValueError(f"parse_jpeg: DHT at byte {pos}: the code lengths over-subscribe the code space")
                huff[(tc, th)] = HuffSpec(bits, tuple(int(v) for v in p[i + 17:i + 17 + cnt]))
                i += 17 + cnt
        elif m == 0xDD:
            if L != 4:
                raise ValueError(f"parse_jpeg: DRI at byte {pos} has length {L}")
            ri = (int(p[0]) << 8) | int(p[1])
        elif m == 0xC0:
            if L < 8:
                raise ValueError(f"parse_jpeg: SOF0 at byte {pos} is truncated")
            prec, h, w, nf = int(p[0]), (int(p[1]) << 8) | int(p[2]), (int(p[3]) << 8) | int(p[4]), int(p[5])
            if prec != 8:
                raise NotImplementedError(f"parse_jpeg: SOF0 precision {prec}: only 8-bit samples are decoded")
            if nf != 1:
                raise NotImplementedError(f"parse_jpeg: SOF0 has {nf} components: only greyscale files are decoded")
            if L != 8 + 3 * nf or h == 0 or w == 0:
                raise ValueError(f"parse_jpeg: SOF0 at byte {pos}: bad frame header ({h} x {w}, length {L})")
            frame = (h, w, int(p[6]), int(p[8]))                       # component id, quantisation table
        elif m == 0xDA:
            if frame is None:
                raise ValueError("parse_jpeg: SOS in front of SOF0")
            if L != 8 or int(p[0]) != 1:
                raise NotImplementedError(f"parse_jpeg: SOS of {int(p[0])} components: one scan of one component is decoded")
            if int(p[1]) != frame[2] or int(p[3]) != 0 or int(p[4]) != 63 or int(p[5]) != 0:
                raise ValueError(f"parse_jpeg: SOS at byte {pos}: not a full sequential scan of the frame's component")
            td, ta = int(p[2]) >> 4, int(p[2]) & 15
            pos += 2 + L
            break
        elif not (0xE0 <= m <= 0xEF or m == 0xFE):
            raise NotImplementedError(f"parse_jpeg: {name} at byte {pos} is not handled")
        pos += 2 + L
    h, w, _cid, tq = frame
    if tq not in qt:
        raise ValueError(f"parse_jpeg: DQT table {tq}, which SOF0 names, is missing")
    if (0, td) not in huff or (1, ta) not in huff:
        raise ValueError(f"parse_jpeg: DHT table (DC {td} / AC {ta}), which SOS names, is missing")
    dc, ac = huff[(0, td)], huff[(1, ta)]
    if any(v > 15 for v in dc.vals):
        raise ValueError("parse_jpeg: DHT: a DC symbol above 15")

    # entropy-coded data: one pass over the bytes finds every FF; what follows it says what it is
    region = d[pos:]
    ff = np.flatnonzero(region[:-1] == 0xFF) if region.size > 1 else np.zeros(0, np.int64)
    nxt = region[ff + 1]
    other = np.flatnonzero((nxt != 0) & ~((nxt >= 0xD0) & (nxt <= 0xD7)))
    if other.size:
        end = int(ff[other[0]])
        if int(nxt[other[0]]) != 0xD9:
            raise ValueError(f"parse_jpeg: {_marker_name(int(nxt[other[0]]))} inside the entropy-coded data at byte {pos + end}")
        ff, nxt = ff[:other[0]], nxt[:other[0]]
    else:
        end = region.size                              # no EOI: the data runs to the end of the file
    rst = ff[nxt != 0]
    keep = np.ones(end, bool)
    stuffed = ff[nxt == 0] + 1
    keep[stuffed[stuffed < end]] = False
    keep[rst] = False
    keep[rst + 1] = False
    csum = np.concatenate([[0], np.cumsum(keep)])
    starts = np.concatenate([[0], rst + 2]).astype(np.int64)
    ends = np.concatenate([rst, [end]]).astype(np.int64)
    nblk = ((h + 7) // 8) * ((w + 7) // 8)
    want = (nblk + ri - 1) // ri if ri else 1
    if len(starts) > want:
        raise ValueError(f"parse_jpeg: {len(starts)} restart segments where DRI {ri} and {nblk} blocks give {want}")
    segs = np.stack([starts + pos, ends - starts], 1)
    ssegs = np.stack([csum[starts], csum[ends] - csum[starts]], 1).astype(np.int64)
    if ssegs[:, 1].max() > MAX_SEGMENT_BYTES:
        raise ValueError(f"parse_jpeg: a restart segment of {int(ssegs[:, 1].max())} bytes (limit {MAX_SEGMENT_BYTES})")
    return JpegInfo(h, w, qt[tq], dc, ac, ri, pos, end, segs, np.ascontiguousarray(region[:end][keep]), ssegs)


def huff_table_words(spec: HuffSpec) -> np.ndarray:
    """The HUFF_WORDS int32 words of one decode table (layout at HUFF_WORDS)."""
    look = np.zeros(1 << LOOK_BITS, np.int32)
    maxcode = np.full(18, -1, np.int32)
    valoff = np.zeros(18, np.int32)
    vals = np.zeros(256, np.int32)
    vals[:len(spec.vals)] = spec.vals
    code, k = 0, 0
    for length, c in enumerate(spec.bits, 1):
        if c:
            valoff[length] = k - code
            for _ in range(c):
                if length <= LOOK_BITS:
                    lo = code << (LOOK_BITS - length)
                    look[lo:lo + (1 << (LOOK_BITS - length))] = (length << 8) | spec.vals[k]
                code += 1
                k += 1
            maxcode[length] = code - 1
        code <<= 1
    maxcode[17] = 0x7FFFFFFF
    return np.concatenate([look, maxcode, valoff, vals])


def is_jpeg_source(im) -> bool:
    return isinstance(im, (bytes, bytearray, memoryview))


class JpegPlan:
    """What ``ops.jpeg_decode`` reads for the JPEG images of a batch.

    streams   uint8 [bytes]              every image's de-stuffed segments back to back (pinned when a GPU is present)
    desc      int32 [n, JPG_WORDS]       one row per JPEG image
    segs      int32 [n_seg, SEG_WORDS]   one row per restart segment, images in order
    tables    int32 [words]              quantisation tables (64 words, natural order) and Huffman decode tables (HUFF_WORDS)
    images    per row the image's index among the batch's present images (error messages, tests)
    """

    def __init__(self, streams, desc, segs, tables, images, total_blocks, max_blocks, max_seg_bytes, file_bytes):
        self.streams, self.desc, self.segs, self.tables = streams, desc, segs, tables
        self.images = list(images)
        self.total_blocks, self.max_blocks, self.max_seg_bytes = int(total_blocks), int(max_blocks), int(max_seg_bytes)
        self.file_bytes = int(file_bytes)

    @property
    def n(self) -> int:
        return self.desc.shape[0]

    def subseq_bits(self, requested: Optional[int] = None) -> int:
        """Bits of one subsequence: ``requested`` (0: one lane per segment) or the host's choice, raised to the smallest
        multiple of 32 that cuts the largest segment into at most MAX_SUBSEQ subsequences."""
        s = DEFAULT_SUBSEQ_BITS if requested is None else int(requested)
        if s < 0:
            raise ValueError("subseq_bits must not be negative")
        if s == 0:
            return 0
        least = -(-self.max_seg_bytes * 8 // MAX_SUBSEQ)
        return (max(s, least, 32) + 31) // 32 * 32

    def stage_bytes(self, requested: Optional[int] = None) -> int:
        """LDS bytes a workgroup of mtmp_jpeg_entropy stages its segment in: the largest segment's, at most MAX_STAGE_BYTES (a
        larger segment is decoded out of global memory), or ``requested`` (tests)."""
        s = min(self.max_seg_bytes, MAX_STAGE_BYTES) if requested is None else int(requested)
        if not 0 <= s <= MAX_STAGE_BYTES:
            raise ValueError(f"stage_bytes must lie in [0, {MAX_STAGE_BYTES}]")
        return (s + 15) // 16 * 16

    def to(self, device, non_blocking: bool = False) -> "JpegPlan":
        mv = lambda t: t.to(device, non_blocking=non_blocking)
        return JpegPlan(mv(self.streams), mv(self.desc), mv(self.segs), mv(self.tables), self.images, self.total_blocks,
                        self.max_blocks, self.max_seg_bytes, self.file_bytes)


def plan_jpegs(infos: Sequence[JpegInfo], dst_offsets: Sequence[int], images: Sequence[int], file_bytes: int = 0,
               pin: Optional[bool] = None) -> JpegPlan:
    """The plan of the parsed files ``infos``, image i going to byte ``dst_offsets[i]`` of the batch's pixel buffer."""
    rows, segs, parts, tab_parts = [], [], [], []
    tab_off, tab_words = {}, 0
    stream_off = coef = max_blocks = max_seg = 0

    def table(key, make):
        nonlocal tab_words
        if key not in tab_off:
            words = make()
            tab_off[key] = tab_words
            tab_parts.append(words.astype(np.int32))
            tab_words += words.size
        return tab_off[key]

    for i, (info, dst) in enumerate(zip(infos, dst_offsets)):
        bh, bw = info.blocks
        d = np.zeros(JPG_WORDS, np.int64)
        d[[JPG_STREAM, JPG_SEG0, JPG_NSEG, JPG_H, JPG_W, JPG_BPR, JPG_NBLK, JPG_DST]] = (
            stream_off, len(segs), len(info.stream_segments), info.h, info.w, bw, bh * bw, dst)
        d[JPG_QT] = table(("q", info.qtable.tobytes()), lambda: info.qtable)
        d[JPG_DC] = table(("h", info.dc), lambda: huff_table_words(info.dc))
        d[JPG_AC] = table(("h", info.ac), lambda: huff_table_words(info.ac))
        d[[JPG_COEF, JPG_RI]] = (coef, info.restart_interval)
        for k, (off, length) in enumerate(info.stream_segments):
            segs.append((stream_off + int(off), int(length), i, k * info.restart_interval))
            max_seg = max(max_seg, int(length))
        rows.append(d)
        parts.append(info.stream)
        stream_off += info.stream.size
        coef += bh * bw
        max_blocks = max(max_blocks, bh * bw)
    desc = np.stack(rows)
    if max(stream_off, coef * 64, tab_words, int(np.abs(desc).max())) >= 2 ** 31 or len(segs) > 2 ** 24:
        raise ValueError("plan_jpegs: the batch does not fit 32-bit offsets")
    if pin is None:
        pin = torch.cuda.is_available()

    def host(a, dtype):
        t = torch.empty(a.shape, dtype=dtype, pin_memory=pin)
        t.copy_(torch.from_numpy(a))
        return t
    streams = np.concatenate(parts) if stream_off else np.zeros(1, np.uint8)
    return JpegPlan(host(streams, torch.uint8), host(desc.astype(np.int32), torch.int32),
                    host(np.array(segs, np.int32).reshape(-1, SEG_WORDS), torch.int32),
                    host(np.concatenate(tab_parts), torch.int32), images, coef, max_blocks, max_seg, file_bytes)


def plan_files(files: Sequence) -> Tuple[JpegPlan, List[Tuple[int, int]]]:
    """The plan of stand-alone files decoded back to back into one pixel buffer, and their (h, w)."""
    infos = [parse_jpeg(f) for f in files]
    offs = np.concatenate([[0], np.cumsum([i.h * i.w for i in infos])])
    plan = plan_jpegs(infos, offs[:-1].tolist(), range(len(infos)), sum(len(f) for f in files))
    return plan, [(i.h, i.w) for i in infos]
