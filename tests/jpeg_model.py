"""The algorithm of csrc/jpeg.hip in NumPy / plain Python, reading the same plan (builder/data/jpeg.JpegPlan): the same span
function, the same synchronisation rounds between the subsequences of a segment, the same scan of block counts and DC sums, the
same write pass, and libjpeg's integer ``islow`` inverse DCT.  It is a model of the kernels for the CPU tests, not another
decoder: what it does lane by lane is what the workgroup does."""
import numpy as np

from medical_tri_modal_pilot_amd.builder.data import jpeg as J

LOOK = 1 << J.LOOK_BITS
STATUS_SHORT, STATUS_LANES, STATUS_SEGMENTS = 1, 2, 4


def _window(seg: bytes, p: int) -> int:
    """32 bits of the segment from bit p on; bits behind its end read as ones."""
    b = p >> 3
    chunk = seg[b:b + 5]
    v = int.from_bytes(chunk + b"\xff" * (5 - len(chunk)), "big")
    return (v >> (8 - (p & 7))) & 0xFFFFFFFF


def _symbol(tab, win: int):
    """(code length, symbol) of the code at the top of the 32-bit window, (0, 0) if there is none."""
    e = int(tab[win >> (32 - J.LOOK_BITS)])
    if e:
        return e >> 8, e & 255
    code16 = win >> 16
    for length in range(J.LOOK_BITS + 1, 17):
        code = code16 >> (16 - length)
        if code <= int(tab[LOOK + length]):
            return length, int(tab[LOOK + 36 + code + int(tab[LOOK + 18 + length])])
    return 0, 0


def _extend(v: int, s: int) -> int:
    return v if s == 0 or v >= (1 << (s - 1)) else v - (1 << s) + 1


def span(seg: bytes, nbits: int, dc, ac, p: int, k: int, end: int, coef=None, blk: int = 0, pred: int = 0, nb: int = 0):
    """Decode from state (bit p, coefficient index k; 0: a DC code is next) up to the first symbol that starts at or behind
    ``end``.  Returns (p, k, blocks completed, sum of their DC differences).  A code that is not in the table, or a symbol that
    would end behind the segment, moves on by one bit.  coef (int16 [blocks, 64], zeroed): the write pass, from block ``blk`` with
    DC predictor ``pred``, blocks >= nb dropped."""
    nblk = dcsum = 0
    while p < end:
        win = _window(seg, p)
        length, sym = _symbol(ac if k else dc, win)
        s = sym & 15
        if length == 0 or p + length + s > nbits:
            p += 1
            continue
        v = _extend((win >> (32 - length - s)) & ((1 << s) - 1), s) if s else 0
        p += length + s
        if k == 0:
            dcsum += v
            pred += v
            if coef is not None and blk < nb:
                coef[blk, 0] = np.int16(((pred + 32768) & 65535) - 32768)
            k = 1
        else:
            r = sym >> 4
            if s == 0:
                k = k + 16 if r == 15 else 64
            else:
                k += r
                if k < 64 and coef is not None and blk < nb:
                    coef[blk, J.ZIGZAG[k]] = v
                k += 1
        if k >= 64:
            k, nblk, blk = 0, nblk + 1, blk + 1
    return p, k, nblk, dcsum


def decode_segment(seg: bytes, nb: int, dc, ac, subseq_bits: int, coef):
    """One workgroup.  Returns (blocks found, synchronisation rounds)."""
    nbits = len(seg) * 8
    nsub = -(-nbits // subseq_bits) if subseq_bits else 1
    nsub = max(nsub, 1)
    if nsub > J.MAX_SUBSEQ:
        return -1, 0
    S = subseq_bits if subseq_bits else nbits
    ends = [min((i + 1) * S, nbits) for i in range(nsub)]
    used = [(i * S, 0) for i in range(nsub)]                  # the entry state a lane decoded from last
    res = [span(seg, nbits, dc, ac, i * S, 0, ends[i]) for i in range(nsub)]
    rounds = 1
    for _ in range(1, nsub):
        entry = [used[0]] + [res[i - 1][:2] for i in range(1, nsub)]       # read, barrier, decode
        changed = False
        for i in range(1, nsub):
            if entry[i] != used[i]:
                used[i] = entry[i]
                new = span(seg, nbits, dc, ac, entry[i][0], entry[i][1], ends[i])
                changed |= new[:2] != res[i][:2]
                res[i] = new
        if not changed:
            break
        rounds += 1                                           # rounds that moved an exit state, the first decode included
    blk0 = np.concatenate([[0], np.cumsum([r[2] for r in res])])
    dc0 = np.concatenate([[0], np.cumsum([r[3] for r in res])])
    for i in range(nsub):
        span(seg, nbits, dc, ac, used[i][0], used[i][1], ends[i], coef, int(blk0[i]), int(dc0[i]), nb)
    return int(blk0[-1]), rounds


C = dict(F_0_298631336=2446, F_0_390180644=3196, F_0_541196100=4433, F_0_765366865=6270, F_0_899976223=7373, F_1_175875602=9633,
         F_1_501321110=12299, F_1_847759065=15137, F_1_961570560=16069, F_2_053119869=16819, F_2_562915447=20995,
         F_3_072711026=25172)


def _pass(x, first: bool):
    """One pass of jpeg_idct_islow along axis 1 of x [blocks, 8 (the transformed axis), 8]."""
    x = x.astype(np.int64)
    i0 = x[:, 0] + (0 if first else 1 << 4)
    z2, z3 = x[:, 2], x[:, 6]
    z1 = (z2 + z3) * C["F_0_541196100"]
    tmp2 = z1 - z3 * C["F_1_847759065"]
    tmp3 = z1 + z2 * C["F_0_765366865"]
    tmp0, tmp1 = (i0 + x[:, 4]) << 13, (i0 - x[:, 4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[:, 7], x[:, 5], x[:, 3], x[:, 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * C["F_1_175875602"]
    tmp0, tmp1 = tmp0 * C["F_0_298631336"], tmp1 * C["F_2_053119869"]
    tmp2, tmp3 = tmp2 * C["F_3_072711026"], tmp3 * C["F_1_501321110"]
    z1, z2 = -z1 * C["F_0_899976223"], -z2 * C["F_2_562915447"]
    z3, z4 = -z3 * C["F_1_961570560"] + z5, -z4 * C["F_0_390180644"] + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    out = np.stack([tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2,
                    tmp10 - tmp3], 1)
    return (out + (1 << 10)) >> 11 if first else out >> 18


def range_limit(x):
    """libjpeg's sample_range_limit table behind its centre, read at x & 1023."""
    v = x & 1023
    return np.where(v < 128, v + 128, np.where(v < 512, 255, np.where(v < 896, 0, v - 896))).astype(np.uint8)


def idct_blocks(coef, q):
    """coef int16 [blocks, 64] natural order, q int32 [64] -> uint8 [blocks, 8, 8]"""
    x = (coef.astype(np.int64) * q.astype(np.int64)).reshape(-1, 8, 8)
    ws = _pass(x, True)                                        # columns: the transformed axis is the row index
    out = _pass(ws.transpose(0, 2, 1), False).transpose(0, 2, 1)
    return range_limit(out)


def decode_plan(plan, pixels, subseq_bits=None):
    """Fill the JPEG images' regions of ``pixels`` (uint8 array, in place).  Returns (status int32 [n], rounds per segment)."""
    S = plan.subseq_bits(subseq_bits)
    desc, segs, tables, streams = (t.numpy() for t in (plan.desc, plan.segs, plan.tables, plan.streams))
    status = np.zeros(plan.n, np.int32)
    coef = np.zeros((plan.total_blocks, 64), np.int16)
    rounds = []
    for si, (off, nbytes, img, b0) in enumerate(segs):
        d = desc[img]
        nb = min(int(d[J.JPG_RI]), int(d[J.JPG_NBLK]) - int(b0)) if d[J.JPG_RI] else int(d[J.JPG_NBLK])
        dc = tables[d[J.JPG_DC]:d[J.JPG_DC] + J.HUFF_WORDS]
        ac = tables[d[J.JPG_AC]:d[J.JPG_AC] + J.HUFF_WORDS]
        first = int(d[J.JPG_COEF]) + int(b0)
        found, r = decode_segment(streams[off:off + nbytes].tobytes(), nb, dc, ac, S, coef[first:first + nb])
        rounds.append(r)
        if found < 0:
            status[img] |= STATUS_LANES
        elif found < nb:
            status[img] |= STATUS_SHORT
        if si - int(d[J.JPG_SEG0]) == int(d[J.JPG_NSEG]) - 1 and int(b0) + nb < int(d[J.JPG_NBLK]):
            status[img] |= STATUS_SEGMENTS
    for i, d in enumerate(desc):
        h, w, bpr, nblk = (int(d[k]) for k in (J.JPG_H, J.JPG_W, J.JPG_BPR, J.JPG_NBLK))
        dst = pixels[int(d[J.JPG_DST]):int(d[J.JPG_DST]) + h * w].reshape(h, w)
        if status[i]:
            dst[:] = 0
            continue
        q = tables[d[J.JPG_QT]:d[J.JPG_QT] + 64]
        px = idct_blocks(coef[int(d[J.JPG_COEF]):int(d[J.JPG_COEF]) + nblk], q)
        full = px.reshape(nblk // bpr, bpr, 8, 8).transpose(0, 2, 1, 3).reshape(nblk // bpr * 8, bpr * 8)
        dst[:] = full[:h, :w]
    return status, rounds


def decode_files(files, subseq_bits=None):
    """[uint8 [h, w]] of stand-alone files, the statuses and the rounds per segment."""
    plan, sizes = J.plan_files(files)
    pixels = np.zeros(sum(h * w for h, w in sizes), np.uint8)
    status, rounds = decode_plan(plan, pixels, subseq_bits)
    out, o = [], 0
    for h, w in sizes:
        out.append(pixels[o:o + h * w].reshape(h, w))
        o += h * w
    return out, status, rounds
