"""Times of the image store (builder/data/cxr_store.py; csrc/jpeg.hip: mtmp_jpeg_sync_points, mtmp_jpeg_store_entropy) on one
MI355X against the per-batch path it replaces (file bytes: parse_jpeg + plan_jpegs + mtmp_jpeg_entropy): the figures of
profiles/cxr_store.txt.  The method of tools/bench_jpeg.py, and its two batches.

    python tools/bench_cxr_store.py [--images 64] [--rounds 20] [--host-rounds 50] [--out FILE]
    python tools/bench_cxr_store.py --host-only       # the planning half alone, where there is no GPU

Per size (260 x 312 and 586 x 586, quality 75, PIL's defaults): every image decoded from the store is compared with PIL's first;
mtmp_jpeg_store_entropy against mtmp_jpeg_entropy at its defaults on the same files, alternating round by round, warm, median of
device-event times around 5 launches; the wall time from samples to a device-ready batch (collate_raw_cxr, .to(device), the
decoder's enqueue) on handles against the same on the files' bytes, same process, median; the bytes that cross the link per
batch; the size of the sync table against the streams; the one-off build time of store.to(device).  Needs PIL (it writes the
files); there is no fallback."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools._timing import Lines, median, wall_ms  # noqa: E402
from tools.bench_jpeg import images, median_pair, pil_decode  # noqa: E402


def median_wall(fa, fb, rounds, after=lambda: None):
    """median wall time of fa and fb in ms, alternating; ``after`` runs outside the timed part (it ends the device's work)"""
    for _ in range(3):
        fa(), after(), fb(), after()
    ts = ([], [])
    for _ in range(rounds):
        for i, fn in enumerate((fa, fb)):
            ts[i].append(wall_ms(fn, sync=False))
            after()
    return median(ts[0]), median(ts[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--host-rounds", type=int, default=50)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    gpu = not a.host_only
    if gpu and not torch.cuda.is_available():
        raise SystemExit("tools/bench_cxr_store.py measures on an MI355X; no GPU found (--host-only times the planning half)")
    from medical_tri_modal_pilot_amd.builder.data.cxr_store import CxrStore
    from medical_tri_modal_pilot_amd.builder.data.cxr_transform import CxrTransform, collate_raw_cxr
    from medical_tri_modal_pilot_amd.synthetic import jpeg_encode
    import PIL
    where = torch.cuda.get_device_name(0) if gpu else "no GPU: planning half only"
    say = Lines()
    say(f"torch {torch.__version__}, {where}, PIL {PIL.__version__}; {a.images} images, quality 75; kernels: median of "
        f"{a.rounds} rounds of 5 launches, device events; host: median of {a.host_rounds} wall times; the two forms alternate")
    tr = CxrTransform(224, "resize_crop", True)
    dev = torch.device("cuda", 0) if gpu else None
    for h, w in ((260, 312), (586, 586)):
        files = [jpeg_encode(im) for im in images(a.images, h, w)]
        t0 = time.perf_counter()
        store = CxrStore.from_files(files)
        t_parse = (time.perf_counter() - t0) * 1e3
        handles = [store.image(i) for i in range(a.images)]
        s_handles = [([hd], [-1.0]) for hd in handles]
        s_bytes = [([f], [-1.0]) for f in files]
        plan_st, plan_by = median_wall(lambda: collate_raw_cxr(s_handles, tr, 0), lambda: collate_raw_cxr(s_bytes, tr, 0), a.host_rounds)
        raw_st, raw_by = collate_raw_cxr(s_handles, tr, 0), collate_raw_cxr(s_bytes, tr, 0)
        nb = lambda *ts: sum(t.numel() * t.element_size() for t in ts if t is not None)
        common = lambda r: nb(r.desc, r.tables, r.slot_map, r.aug)
        sent_st = common(raw_st) + raw_st.stored.nbytes
        jp = raw_by.jpeg
        sent_by = common(raw_by) + nb(raw_by.pixels, jp.streams, jp.desc, jp.segs, jp.tables)
        for s in [f"{a.images} x {h} x {w}: files {sum(len(f) for f in files)} bytes; store: streams {store.nbytes_streams}, sync table "
                  f"{store.nbytes_sync} ({store.nbytes_sync / store.nbytes_streams:.3f} of the streams), all {store.nbytes} bytes against "
                  f"{a.images * h * w} bytes of uint8 pixels ({store.nbytes / (a.images * h * w):.3f}); from_files (parse, once) {t_parse:.1f} ms",
                  f"  planning half (collate_raw_cxr alone): handles {plan_st:8.3f} ms, file bytes {plan_by:8.3f} ms",
                  f"  bytes over the link per batch: handles {sent_st} (store rows and prefix {raw_st.stored.nbytes}), file bytes {sent_by} "
                  f"(zero pixel buffer {raw_by.pixels.numel()}, streams {jp.streams.numel()})"]:
            say(s)
        if not gpu:
            continue
        from medical_tri_modal_pilot_amd import ops
        from medical_tri_modal_pilot_amd._lib import call
        from medical_tri_modal_pilot_amd.ops import _p, _stream
        store.to(dev)
        torch.cuda.synchronize()
        want = [np.asarray(pil_decode(f)) for f in files]
        pixels, sizes = ops.cxr_store_decode(store, list(range(a.images)))
        got = pixels.cpu().numpy().reshape(a.images, h, w)
        bad = sum(int(not np.array_equal(g, w_)) for g, w_ in zip(got, want))
        if bad:
            raise SystemExit(f"{h} x {w}: {bad} images decoded from the store differ from PIL's decode")
        sb = raw_st.stored.to(dev)
        p = jp.to(dev)
        coef = torch.zeros(p.total_blocks * 64, dtype=torch.int16, device=dev)
        status = torch.zeros(p.n, dtype=torch.int32, device=dev)
        S = p.subseq_bits(None)

        def parent():
            call("mtmp_jpeg_entropy", _p(p.streams), _p(p.desc), _p(p.segs), _p(p.tables), _p(coef), _p(status), None, p.segs.shape[0],
                 p.max_seg_bytes, S, p.stage_bytes(), _stream())

        def stored():
            call("mtmp_jpeg_store_entropy", _p(store.d_streams), _p(store.d_segs), _p(store.d_sync), _p(store.d_tables), _p(sb.desc),
                 _p(sb.wide), _p(sb.prefix), _p(coef), sb.n, sb.lanes, store.d_streams.numel(), store.d_segs.shape[0],
                 store.d_sync.shape[0], store.d_tables.numel(), _stream())
        t_st, t_par = median_pair(stored, parent, a.rounds)

        def batch(samples):
            raw = collate_raw_cxr(samples, tr, 0).to(dev, non_blocking=True)
            ops.jpeg_decode(raw)
        w_st, w_by = median_wall(lambda: batch(s_handles), lambda: batch(s_bytes), a.host_rounds, torch.cuda.synchronize)
        for s in [f"  mtmp_jpeg_store_entropy ({sb.lanes} lanes, {-(-sb.lanes // 256)} workgroups of 256): {t_st * 1e3:9.1f} us;  mtmp_jpeg_entropy "
                  f"(subseq_bits {S}, {p.segs.shape[0]} workgroups, its defaults): {t_par * 1e3:9.1f} us;  ratio {t_par / t_st:.2f}",
                  f"  samples -> device-ready batch (collate_raw_cxr, .to(device), the decoder's enqueue): handles {w_st:8.3f} ms, file bytes "
                  f"{w_by:8.3f} ms",
                  f"  store.to(device), once (upload, sync table, status read-back): {store.build_ms:8.2f} ms"]:
            say(s)
    say.write(a.out)


if __name__ == "__main__":
    main()
