"""Chest X-ray files as a device-resident store: every JPEG file is parsed ONCE, its de-stuffed entropy-coded bytes stay on the
device, and beside them a *sync table* holds, for every subsequence of every restart segment, the state a decoder lane needs to
start there (csrc/jpeg.hip, mtmp_jpeg_sync_points).  A sample then carries ``store.image(i)`` -- four integers -- in place of the
file's bytes, a batch is a few gathered rows (numpy, no per-image Python), and one flat launch decodes it
(mtmp_jpeg_store_entropy): no parsing, no synchronisation rounds, no stream and no pixel byte on the host-to-device link.

JPEG bytes, not pixels, are the stored form: the decoded uint8 images are about five times larger (profiles/jpeg_decode.txt).

Layout (all of it documented in include/mtmp.h at mtmp_jpeg_sync_points):
  streams  uint8 [bytes]              the de-stuffed segments of all images back to back
  rows     int32 [n, JPG_WORDS]       one row per image: the words of builder/data/jpeg.py's JPG_* rows that do not depend on the
                                      batch (JPG_SEG0: its first row of ``segs``; JPG_STREAM, JPG_DST, JPG_COEF zero), its own
                                      subsequence length (JPG_SUBSEQ) and its number of sync rows (JPG_NSYNC)
  wide     int64 [n, 2]               the two offsets that outgrow 32 bits: the image's first byte in ``streams`` and its first
                                      row of the sync table; everything inside one image is 32-bit
  segs     int32 [n_seg, 4]           one row per restart segment, relative to its image: byte offset, bytes, first block, first
                                      sync row
  tables   int32 [words]              quantisation and Huffman decode tables, shared between images of equal payload
  sync     int32 [n_sync, 4]          DEVICE ONLY, made by ``to(device)``: entry state (bit position << 6 | coefficient index),
                                      the block that symbol belongs to (relative to the segment), the DC predictor there, the
                                      segment (relative to the image)
``rows``, ``wide`` and ``segs`` stay on the host as numpy arrays (the mirror a batch is planned from); the device holds streams,
segs, tables and sync.

``from_patients`` / ``select`` / ``image_wanted`` resolve WHICH images a sample gets: the reference's image branch
(builder/data/dataset_new.py:2069-2133) on a CSR of (time, image) pairs per patient.
"""
from typing import Optional, Sequence

import numpy as np
import torch

from . import resolve_device
from .jpeg import (DEFAULT_SUBSEQ_BITS, JPG_AC, JPG_BPR, JPG_COEF, JPG_DC, JPG_DST, JPG_H, JPG_NBLK, JPG_NSEG, JPG_QT, JPG_RI,
                   JPG_SEG0, JPG_STREAM, JPG_W, JPG_WORDS, MAX_STAGE_BYTES, MAX_SUBSEQ, huff_table_words, parse_jpeg)

JPG_SUBSEQ, JPG_NSYNC = 13, 14        # words of an image row that only the store fills
WIDE_STREAM, WIDE_SYNC0 = 0, 1
TSEG_WORDS = 4
TSEG_OFF, TSEG_BYTES, TSEG_BLOCK0, TSEG_SYNC0 = range(4)
SYNC_WORDS = 4
SYNC_STATE, SYNC_BLOCK, SYNC_PRED, SYNC_SEG = range(4)
STORE_LANES = 256                     # lanes of one workgroup of mtmp_jpeg_store_entropy
# one build launch of to(device): at most this many stream bytes / sync rows / segments, so that every offset inside a launch is
# 32-bit and the temporary rows stay small
CHUNK_BYTES, CHUNK_SYNC_ROWS, CHUNK_SEGS = 64 << 20, 1 << 22, 1 << 20


def subseq_bits_of(max_seg_bytes: int, requested: Optional[int] = None) -> int:
    """What ``JpegPlan.subseq_bits`` chooses for an image whose largest segment has ``max_seg_bytes`` bytes: ``requested`` (None:
    the default), raised to the smallest multiple of 32 that cuts that segment into at most MAX_SUBSEQ subsequences."""
    s = DEFAULT_SUBSEQ_BITS if requested is None else int(requested)
    if s < 1:
        raise ValueError("CxrStore: subseq_bits must be positive (the store has one sync row per subsequence)")
    least = -(-int(max_seg_bytes) * 8 // MAX_SUBSEQ)
    return (max(s, least, 32) + 31) // 32 * 32


class CxrImage:
    """One image of a store: what a sample carries in place of the file's bytes."""
    __slots__ = ("store", "index", "h", "w")

    def __init__(self, store, index: int, h: int, w: int):
        self.store, self.index, self.h, self.w = store, int(index), int(h), int(w)

    def __repr__(self):
        return f"CxrImage({self.index}: {self.h} x {self.w})"


class CxrStoreBatch:
    """The stored images of one batch: ONE int32 buffer (pinned when a GPU is present) that holds, in this order,
    wide    int64 [n, 2]          stream offset and first sync row of every image, exactly as the store has them
    desc    int32 [n, JPG_WORDS]  the store's rows gathered by index, JPG_DST and JPG_COEF filled in
    prefix  int32 [n + 1]         exclusive prefix sum of the images' sync rows = decoder lanes
    plus the host's copies of what sizes the launches.  ``images``: per row the image's index among the batch's present images."""

    def __init__(self, store, indices, buf, images, total_blocks, max_blocks, lanes):
        self.store, self.indices, self.buf, self.images = store, indices, buf, list(images)
        self.total_blocks, self.max_blocks, self.lanes = int(total_blocks), int(max_blocks), int(lanes)
        n = len(indices)
        self.wide = buf[:4 * n].view(torch.int64).view(n, 2)
        self.desc = buf[4 * n:(4 + JPG_WORDS) * n].view(n, JPG_WORDS)
        self.prefix = buf[(4 + JPG_WORDS) * n:]

    @property
    def n(self) -> int:
        return len(self.indices)

    @property
    def nbytes(self) -> int:
        """bytes that go to the device for this batch"""
        return int(self.buf.numel() * 4)

    def to(self, device, non_blocking: bool = False) -> "CxrStoreBatch":
        return CxrStoreBatch(self.store, self.indices, self.buf.to(device, non_blocking=non_blocking), self.images,
                             self.total_blocks, self.max_blocks, self.lanes)


class CxrStore:
    def __init__(self, streams, rows, wide, segs, tables, names=None, file_bytes: int = 0):
        """From arrays (``from_files`` makes them).  ``streams`` may be None for a host mirror that only plans batches."""
        self.rows = np.ascontiguousarray(rows, np.int32).reshape(-1, JPG_WORDS)
        self.wide = np.ascontiguousarray(wide, np.int64).reshape(-1, 2)
        self.segs = np.ascontiguousarray(segs, np.int32).reshape(-1, TSEG_WORDS)
        self.tables = np.ascontiguousarray(tables, np.int32).ravel()
        self.streams = None if streams is None else np.ascontiguousarray(streams, np.uint8).ravel()
        n = self.rows.shape[0]
        if n < 1 or self.wide.shape[0] != n:
            raise ValueError(f"CxrStore: {n} image rows and {self.wide.shape[0]} offset rows")
        self.names = [str(i) for i in range(n)] if names is None else [str(v) for v in names]
        if len(self.names) != n:
            raise ValueError(f"CxrStore: {len(self.names)} names for {n} images")
        self.file_bytes = int(file_bytes)
        self.n_sync = int(self.wide[-1, WIDE_SYNC0] + self.rows[-1, JPG_NSYNC])
        self.n_stream_bytes = int(self.streams.size) if self.streams is not None else 0
        self.device = torch.device("cpu")
        self.d_streams = self.d_segs = self.d_tables = self.d_sync = None
        self.build_ms = None
        self._patients = None

    # ---------------------------------------------------------------------------------------------------------- the host half
    @classmethod
    def from_files(cls, files: Sequence, subseq_bits: Optional[int] = None, names: Optional[Sequence] = None) -> "CxrStore":
        """files: the ``bytes`` / ``bytearray`` / ``memoryview`` of baseline greyscale JPEG files.  A file ``parse_jpeg`` does not
        accept is refused here, by index and name; there is no fallback."""
        files = list(files)
        if not files:
            raise ValueError("CxrStore.from_files: no file")
        names = [str(i) for i in range(len(files))] if names is None else [str(v) for v in names]
        if len(names) != len(files):
            raise ValueError(f"CxrStore.from_files: {len(names)} names for {len(files)} files")
        rows = np.zeros((len(files), JPG_WORDS), np.int64)
        wide = np.zeros((len(files), 2), np.int64)
        seg_parts, parts, tab_parts = [], [], []
        tab_off, tab_words = {}, 0
        stream_off = n_seg = n_sync = file_bytes = 0

        def table(key, make):
            nonlocal tab_words
            if key not in tab_off:
                words = make()
                tab_off[key] = tab_words
                tab_parts.append(words.astype(np.int32))
                tab_words += words.size
            return tab_off[key]

        for i, f in enumerate(files):
            try:
                info = parse_jpeg(f)
            except (ValueError, NotImplementedError) as e:
                raise type(e)(f"CxrStore.from_files: file {i} ({names[i]}): {e}") from None
            bh, bw = info.blocks
            ss = info.stream_segments
            S = subseq_bits_of(int(ss[:, 1].max()), subseq_bits)
            nsub = np.maximum(-(-(ss[:, 1] * 8) // S), 1)
            sync0 = np.concatenate([[0], np.cumsum(nsub)])
            seg = np.zeros((len(ss), TSEG_WORDS), np.int64)
            seg[:, TSEG_OFF], seg[:, TSEG_BYTES] = ss[:, 0], ss[:, 1]
            seg[:, TSEG_BLOCK0] = np.arange(len(ss)) * info.restart_interval
            seg[:, TSEG_SYNC0] = sync0[:-1]
            d = rows[i]
            d[[JPG_SEG0, JPG_NSEG, JPG_H, JPG_W, JPG_BPR, JPG_NBLK]] = (n_seg, len(ss), info.h, info.w, bw, bh * bw)
            d[JPG_QT] = table(("q", info.qtable.tobytes()), lambda: info.qtable)
            d[JPG_DC] = table(("h", info.dc), lambda: huff_table_words(info.dc))
            d[JPG_AC] = table(("h", info.ac), lambda: huff_table_words(info.ac))
            d[[JPG_RI, JPG_SUBSEQ, JPG_NSYNC]] = (info.restart_interval, S, sync0[-1])
            wide[i] = (stream_off, n_sync)
            seg_parts.append(seg)
            parts.append(info.stream)
            stream_off += info.stream.size
            n_seg += len(ss)
            n_sync += int(sync0[-1])
            file_bytes += memoryview(f).nbytes
        if max(n_seg, tab_words, int(rows.max())) >= 2 ** 31:
            raise ValueError("CxrStore.from_files: the segment rows or the tables do not fit 32-bit offsets")
        streams = np.concatenate(parts) if stream_off else np.zeros(1, np.uint8)
        return cls(streams, rows.astype(np.int32), wide, np.concatenate(seg_parts).astype(np.int32), np.concatenate(tab_parts),
                   names, file_bytes)

    @property
    def n_images(self) -> int:
        return int(self.rows.shape[0])

    @property
    def nbytes_streams(self) -> int:
        return self.n_stream_bytes

    @property
    def nbytes_sync(self) -> int:
        return self.n_sync * SYNC_WORDS * 4

    @property
    def nbytes(self) -> int:
        """what the store holds on the device: streams, sync table, segment rows, tables"""
        return self.nbytes_streams + self.nbytes_sync + int(self.segs.size + self.tables.size) * 4

    def image(self, i: int) -> CxrImage:
        i = int(i)
        if not 0 <= i < self.n_images:
            raise IndexError(f"CxrStore.image: {i} is outside 0..{self.n_images - 1}")
        return CxrImage(self, i, self.rows[i, JPG_H], self.rows[i, JPG_W])

    # --------------------------------------------------------------------------------------------------------- the device half
    def _chunks(self):
        """[a, b) image ranges of the build launches (a single image always fits: everything inside one is 32-bit)"""
        n = self.n_images
        seg_end = self.rows[:, JPG_SEG0].astype(np.int64) + self.rows[:, JPG_NSEG]
        sync_end = self.wide[:, WIDE_SYNC0] + self.rows[:, JPG_NSYNC]
        byte_end = np.concatenate([self.wide[1:, WIDE_STREAM], [self.n_stream_bytes]])
        a = 0
        while a < n:
            b = min(int(np.searchsorted(byte_end, self.wide[a, WIDE_STREAM] + CHUNK_BYTES, "right")),
                    int(np.searchsorted(sync_end, self.wide[a, WIDE_SYNC0] + CHUNK_SYNC_ROWS, "right")),
                    int(np.searchsorted(seg_end, int(self.rows[a, JPG_SEG0]) + CHUNK_SEGS, "right")), n)
            b = max(b, a + 1)
            yield a, b
            a = b

    def to(self, device) -> "CxrStore":
        """Upload streams, segment rows and tables, build the sync table on the device (mtmp_jpeg_sync_points, chunk by chunk),
        read the status words back ONCE.  An image whose stream does not yield its blocks is refused by name, and the store stays
        on the host."""
        device = resolve_device(device)
        if device == self.device:
            return self
        if device.type != "cuda":
            raise RuntimeError(f"CxrStore.to: the sync table is built on an MI355X only (asked for {device}); there is no CPU fallback")
        if self.device.type != "cpu":
            raise RuntimeError(f"CxrStore.to: the store is already on {self.device}; build another one for another device")
        if self.streams is None:
            raise RuntimeError("CxrStore.to: this store is a host mirror without streams")
        import time
        from ... import _lib
        t0 = time.perf_counter()
        n = self.n_images
        p = lambda t, off=0: t.data_ptr() + off
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream().cuda_stream
            d_streams = torch.empty(self.n_stream_bytes, dtype=torch.uint8, device=device)
            d_sync = torch.empty((self.n_sync, SYNC_WORDS), dtype=torch.int32, device=device)
            d_tables = torch.from_numpy(self.tables).to(device)
            d_segs = torch.from_numpy(self.segs).to(device)
            status = torch.zeros(n, dtype=torch.int32, device=device)
            nseg = self.rows[:, JPG_NSEG].astype(np.int64)
            for a, b in self._chunks():
                s0 = int(self.wide[a, WIDE_STREAM])
                s1 = int(self.wide[b, WIDE_STREAM]) if b < n else self.n_stream_bytes
                y0 = int(self.wide[a, WIDE_SYNC0])
                y1 = int(self.wide[b, WIDE_SYNC0]) if b < n else self.n_sync
                m0 = int(self.rows[a, JPG_SEG0])
                m1 = m0 + int(nseg[a:b].sum())
                d_streams[s0:s1].copy_(torch.from_numpy(self.streams[s0:s1]))
                r = self.rows[a:b].astype(np.int64)
                r[:, JPG_STREAM] = self.wide[a:b, WIDE_STREAM] - s0
                r[:, JPG_SEG0] -= m0
                img = np.repeat(np.arange(b - a), nseg[a:b])
                t = self.segs[m0:m1].astype(np.int64)
                seg = np.stack([r[img, JPG_STREAM] + t[:, TSEG_OFF], t[:, TSEG_BYTES], img, t[:, TSEG_BLOCK0]], 1)
                sync0 = (self.wide[a:b, WIDE_SYNC0] - y0)[img] + t[:, TSEG_SYNC0]
                lanes = int(np.maximum(-(-(t[:, TSEG_BYTES] * 8) // r[img, JPG_SUBSEQ]), 1).max())
                if lanes > MAX_SUBSEQ or max(s1 - s0, y1 - y0) >= 2 ** 31:
                    raise ValueError(f"CxrStore.to: images {a}..{b - 1} do not fit one build launch")
                stage = (min(int(t[:, TSEG_BYTES].max()), MAX_STAGE_BYTES) + 15) // 16 * 16
                dev = [torch.from_numpy(np.ascontiguousarray(x.astype(np.int32))).to(device) for x in (r, seg, sync0)]
                _lib.call("mtmp_jpeg_sync_points", p(d_streams, s0), p(dev[0]), p(dev[1]), p(d_tables), p(dev[2]),
                          p(d_sync, y0 * SYNC_WORDS * 4), p(status, a * 4), m1 - m0, lanes, y1 - y0, stage, stream)
            st = status.cpu().numpy()                   # the one read-back; it also ends the launches that read `dev`
        bad = np.flatnonzero(st)
        if bad.size:
            raise ValueError("CxrStore.to: the JPEG stream of image(s) " +
                             ", ".join(f"{int(i)} ({self.names[int(i)]}, status {int(st[i])})" for i in bad[:8]) +
                             (" ..." if bad.size > 8 else "") + " is truncated or corrupt; the store holds no such image")
        self.d_streams, self.d_segs, self.d_tables, self.d_sync = d_streams, d_segs, d_tables, d_sync
        self.device = device
        self.streams = None                             # the bytes live on the device now; the mirror rows stay
        self.build_ms = (time.perf_counter() - t0) * 1e3
        return self

    # ----------------------------------------------------------------------------------------------------------------- batches
    def batch(self, indices, dst_offsets=None, images=None, pin: Optional[bool] = None) -> CxrStoreBatch:
        """The plan of decoding images ``indices`` (any order, repeats allowed), image k going to byte ``dst_offsets[k]`` of the
        batch's pixel buffer (None: back to back).  numpy on the mirror rows; nothing touches the device."""
        idx = np.asarray(indices, np.int64).ravel()
        n = idx.size
        if n < 1:
            raise ValueError("CxrStore.batch: no image")
        if idx.min() < 0 or idx.max() >= self.n_images:
            raise ValueError(f"CxrStore.batch: an index outside 0..{self.n_images - 1}")
        d = self.rows[idx].astype(np.int64)
        nblk = d[:, JPG_NBLK]
        coef = np.cumsum(nblk) - nblk
        if dst_offsets is None:
            px = d[:, JPG_H] * d[:, JPG_W]
            dst = np.cumsum(px) - px
        else:
            dst = np.asarray(dst_offsets, np.int64).ravel()
        d[:, JPG_DST], d[:, JPG_COEF] = dst, coef
        prefix = np.concatenate([[0], np.cumsum(d[:, JPG_NSYNC])])
        if max(int(prefix[-1]), int(nblk.sum()) * 64, int(dst.max()) + int((d[:, JPG_H] * d[:, JPG_W]).max())) >= 2 ** 31:
            raise ValueError("CxrStore.batch: the batch does not fit 32-bit offsets")
        words = np.concatenate([self.wide[idx].ravel().view(np.int32), d.astype(np.int32).ravel(), prefix.astype(np.int32)])
        if pin is None:
            pin = torch.cuda.is_available()
        buf = torch.empty(words.size, dtype=torch.int32, pin_memory=pin)
        buf.copy_(torch.from_numpy(words))
        return CxrStoreBatch(self, idx, buf, range(n) if images is None else images, nblk.sum(), nblk.max(), prefix[-1])

    # ------------------------------------------------------------------------------------------- which images a sample gets
    @classmethod
    def from_patients(cls, patients, subseq_bits: Optional[int] = None) -> "CxrStore":
        """patients: per patient a sequence of ``(time, name, file bytes)``: the reference's ``data_pkl['cxr_input']`` pairs
        ``(time, path)`` with the file behind each path.  The store holds every file once, in the order given, and a CSR
        (patient -> its images ordered as ``sorted()`` orders the ``(time, path)`` tuples) for ``select``."""
        files, names, times, ptr = [], [], [], [0]
        for pat in patients:
            for t, name, data in pat:
                files.append(data)
                names.append(str(name))
                times.append(float(t))
            ptr.append(len(files))
        store = cls.from_files(files, subseq_bits, names)
        store.set_patients(ptr, times)
        return store

    def set_patients(self, ptr, times):
        """ptr int [P + 1]: patient p owns images ptr[p] .. ptr[p + 1] - 1; times float [n_images]."""
        ptr, times = np.asarray(ptr, np.int64), np.asarray(times, np.float64)
        if ptr[0] != 0 or ptr[-1] != self.n_images or (np.diff(ptr) < 0).any() or times.shape != (self.n_images,):
            raise ValueError("CxrStore.set_patients: ptr must run from 0 to n_images, one time per image")
        order = np.empty(self.n_images, np.int64)
        for p in range(len(ptr) - 1):                   # once per store: sorted() on (time, path), as the reference's branch does
            a, b = int(ptr[p]), int(ptr[p + 1])
            order[a:b] = sorted(range(a, b), key=lambda i: (times[i], self.names[i]))
        self._patients = (ptr, order, times[order])

    def select(self, samples, n_images: int, realtime: int, train_full: bool = False):
        """samples: per sample ``(patient, selected_key, t0, wanted)`` -- ``selected_key`` after the ``late_nones`` correction,
        ``t0`` = ``selected_key`` or the window's ``min_time``, ``wanted`` = ``image_wanted(...)`` and the sample has images
        and its modality combination keeps them.  Returns ``(pairs, missing)``: ``pairs`` the ``(handles, times)`` list that
        ``collate_raw_cxr`` takes, ``missing`` bool [B].  n_images = 0: the last image with ``time <= selected_key``, its time
        minus ``selected_key`` (realtime 1) or minus ``t0``; n_images = K: the last K in ascending order, times minus
        ``selected_key`` (dataset_new.py:2114).  train_full: a wanted sample without an eligible image raises (the reference
        exits the process there, :2077-2079)."""
        if self._patients is None:
            raise RuntimeError("CxrStore.select: the store has no patient table (from_patients / set_patients)")
        ptr, order, stimes = self._patients
        K = int(n_images)
        pairs, missing = [], np.ones(len(samples), bool)
        for b, (pat, key, t0, wanted) in enumerate(samples):
            chosen = []
            if wanted:
                pat = int(pat)
                if not 0 <= pat < len(ptr) - 1:
                    raise ValueError(f"CxrStore.select: sample {b} names patient {pat}, the store holds 0..{len(ptr) - 2}")
                a, e = int(ptr[pat]), int(ptr[pat + 1])
                m = a + int(np.searchsorted(stimes[a:e], key, "right"))      # time <= selected_key
                if m == a and train_full:
                    raise ValueError(f"CxrStore.select: sample {b} (patient {pat}, selected_key {key}) has no image at or before "
                                     "its selected_key, which train-full requires")
                chosen = list(range(max(a, m - max(K, 1)), m))
            missing[b] = not chosen
            sub = key if (K or int(realtime) == 1) else t0
            pairs.append(([self.image(order[i]) for i in chosen], [stimes[i] - sub for i in chosen]))
        return pairs, missing


def image_wanted(args, type_id: int, missing_comb: int, has_cxr: bool) -> bool:
    """The reference's condition for reading a sample's images (dataset_new.py:2075 and the ``missing_comb`` half of :2080):
    ``has_cxr``: 'cxr_input' is in the sample and not None.  (With train-full the reference tests for an eligible image BEFORE it
    looks at ``missing_comb``, :2077; a train-full sample of combination 1 or 2 without one exits there and is simply absent here.)"""
    inputs, incl = args.input_types, args.modality_inclusion
    full = "img" in inputs and "img1" in args.fullmodal_definition and "train-full" in incl
    miss = "train-missing" in incl and int(type_id) in (0, 2, 3, 5) and "img" in inputs
    return bool((full or miss) and has_cxr and int(missing_comb) not in (1, 2))
