"""Times of the JPEG decoder (csrc/jpeg.hip) on one MI355X, against PIL on the same box's CPU: the figures of
profiles/jpeg_decode.txt.

    python tools/bench_jpeg.py [--images 64] [--rounds 20] [--out FILE]

Per size (260 x 312 and 586 x 586, quality 75, PIL's defaults; synthetic.make_raw_cxr's content): mtmp_jpeg_entropy with the
host's choice of subseq_bits and with 0 (one lane per segment), alternating, warm, median of device-event times around `inner`
launches; mtmp_jpeg_idct; the synchronisation rounds; ops.jpeg_decode_images with its allocations and zero-fills; the bytes that
go to the device against the uint8 pixels; PIL's Image.open + load of the same files with one thread and with 16.  Every decoded
image is compared with PIL's first.  Needs PIL (it writes the files) and a GPU; there is no fallback."""
import argparse
import io
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def images(n, h, w, seed=5):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        y, x = np.mgrid[0:h, 0:w]
        a = (70 + 90 * rng.random() + 60 * np.sin(x / (20 + 40 * rng.random())) * np.cos(y / (15 + 30 * rng.random()))
             + 40 * (x / w) + rng.normal(0, 10, (h, w)))
        out.append(np.clip(a, 0, 255).astype(np.uint8))
    return out


def median_pair(fa, fb, rounds, inner=5):
    for _ in range(2):
        fa()
        fb()
    ts = ([], [])
    for _ in range(rounds):
        for i, fn in enumerate((fa, fb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts[i].append(e0.elapsed_time(e1) / inner)
    return sorted(ts[0])[rounds // 2], sorted(ts[1])[rounds // 2]


def pil_decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_jpeg.py measures on an MI355X; no GPU found")
    from medical_tri_modal_pilot_amd import ops
    from medical_tri_modal_pilot_amd._lib import call
    from medical_tri_modal_pilot_amd.builder.data.jpeg import plan_files
    from medical_tri_modal_pilot_amd.ops import _p, _stream
    from medical_tri_modal_pilot_amd.synthetic import jpeg_encode
    import PIL
    lines = [f"torch {torch.__version__}, {torch.cuda.get_device_name(0)}, PIL {PIL.__version__}; {a.images} images, quality 75, "
             f"median of {a.rounds} rounds of 5 launches, device events"]
    dev = torch.device("cuda", 0)
    for h, w in ((260, 312), (586, 586)):
        files = [jpeg_encode(im) for im in images(a.images, h, w)]
        want = [np.asarray(pil_decode(f)) for f in files]
        t0 = time.perf_counter()
        plan, sizes = plan_files(files)
        t_plan = time.perf_counter() - t0
        for bits in (None, 0):
            got = ops.jpeg_decode_images(files, dev, subseq_bits=bits)
            bad = sum(int(not np.array_equal(g.cpu().numpy(), w_)) for g, w_ in zip(got, want))
            if bad:
                raise SystemExit(f"{h} x {w}, subseq_bits {bits}: {bad} images differ from PIL's decode")
        p = plan.to(dev)
        nseg = p.segs.shape[0]
        coef = torch.zeros(p.total_blocks * 64, dtype=torch.int16, device=dev)
        status = torch.zeros(p.n, dtype=torch.int32, device=dev)
        rounds = torch.zeros(nseg, dtype=torch.int32, device=dev)
        pixels = torch.empty(a.images * h * w, dtype=torch.uint8, device=dev)
        S = p.subseq_bits(None)

        def entropy(bits):
            call("mtmp_jpeg_entropy", _p(p.streams), _p(p.desc), _p(p.segs), _p(p.tables), _p(coef), _p(status), _p(rounds), nseg,
                 p.max_seg_bytes, bits, p.stage_bytes(), _stream())

        def idct():
            call("mtmp_jpeg_idct", _p(coef), _p(p.desc), _p(p.tables), _p(status), _p(pixels), p.n, p.max_blocks, _stream())
        entropy(S)
        torch.cuda.synchronize()
        r = rounds.cpu()
        t_par, t_one = median_pair(lambda: entropy(S), lambda: entropy(0), a.rounds)
        t_idct, t_all = median_pair(idct, lambda: ops.jpeg_decode_images(files, dev), a.rounds)
        sent = sum(t.numel() * t.element_size() for t in (plan.streams, plan.desc, plan.segs, plan.tables))
        t0 = time.perf_counter()
        for f in files:
            pil_decode(f)
        t_pil1 = time.perf_counter() - t0
        with ThreadPoolExecutor(16) as ex:
            list(ex.map(pil_decode, files))
            t0 = time.perf_counter()
            list(ex.map(pil_decode, files))
            t_pil16 = time.perf_counter() - t0
        lines += [
            f"{a.images} x {h} x {w}: files {sum(len(f) for f in files)} bytes, sent to the device {sent} bytes (streams {plan.streams.numel()}, "
            f"rows and tables {sent - plan.streams.numel()}) against {a.images * h * w} bytes of uint8 pixels ({sent / (a.images * h * w):.3f})",
            f"  mtmp_jpeg_entropy  subseq_bits {S} (host's choice): {t_par * 1e3:9.1f} us, rounds max {int(r.max())} mean {float(r.float().mean()):.2f}, "
            f"lanes of the largest segment {-(-p.max_seg_bytes * 8 // S)}",
            f"  mtmp_jpeg_entropy  subseq_bits 0 (one lane per segment): {t_one * 1e3:9.1f} us",
            f"  mtmp_jpeg_idct: {t_idct * 1e3:9.1f} us;  entropy + idct {(t_par + t_idct) * 1e3:9.1f} us = {a.images / (t_par + t_idct) * 1e3:10.0f} images/s",
            f"  ops.jpeg_decode_images (host parse and plan, H2D, zero-fills, both kernels, status copy): {t_all:9.3f} ms; host parse "
            f"and plan alone {t_plan * 1e3:9.3f} ms",
            f"  PIL Image.open + load on this box: 1 thread {t_pil1 / a.images * 1e3:7.3f} ms per image ({a.images / t_pil1:8.0f} images/s), 16 threads "
            f"{t_pil16 * 1e3:7.3f} ms for the {a.images} ({a.images / t_pil16:8.0f} images/s)",
        ]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
