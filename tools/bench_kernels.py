"""Per-kernel micro-benchmarks at the config-2 shapes (B=64, N_v=1005): TF/s or GB/s of every
libmtmp_hip.so kernel next to the library GEMM (torch.matmul -> hipBLASLt) on the same random
data, measured with HIP events on the launch stream (interleaved rounds, median).

    python tools/bench_kernels.py [--rounds 7] [--only gemm_nt,attn]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from medical_tri_modal_pilot_amd import ops  # noqa: E402

DEV = "cuda:0"
BF = torch.bfloat16


def timeit(fn, rounds, inner=5):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    ts.sort()
    return ts[len(ts) // 2]


def timeit_pair(fa, fb, rounds, inner=5):
    """two forms of one product, alternating round by round in this process: (min ms of fa, min ms of fb)"""
    for _ in range(2):
        fa()
        fb()
    best = [float("inf"), float("inf")]
    for _ in range(rounds):
        for i, fn in enumerate((fa, fb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            best[i] = min(best[i], e0.elapsed_time(e1) / inner)
    return best[0], best[1]


def timeit_pair_median(fa, fb, rounds, inner=5):
    """two forms of one product, warm, alternating round by round in this process: (median ms of fa, median ms of fb)"""
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


# (tokens a side, C, heads) of the four stages of the image encoder at --image-size 512: no side is a multiple of the 7x7 window
SWIN_512 = ((128, 96, 3), (64, 192, 6), (32, 384, 12), (16, 768, 24))


# (N = dY width, K = X width, rows at 64 images) of the weight gradients of the trainable image encoder whose widths are not
# multiples of 128: stem, stage 1 qkv / proj / fc1 / fc2, patch merging 1, stage 2 qkv / proj / fc1 / fc2
ENCODER_TN = ((96, 16, 200704), (288, 96, 200704), (96, 96, 200704), (384, 96, 200704), (96, 384, 200704), (192, 384, 50176),
              (576, 192, 50176), (192, 192, 50176), (768, 192, 50176), (192, 768, 50176))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    only = [s for s in a.only.split(",") if s]
    g = torch.Generator(device=DEV).manual_seed(0)
    R = lambda *s: torch.randn(*s, generator=g, device=DEV, dtype=torch.float32).to(BF)
    M = 64 * 1005
    out = {}
    table = ""

    def rec(name, ms, flops=None, bytes_=None):
        d = {"ms": round(ms, 4)}
        if flops:
            d["TFLOPs"] = round(flops / ms / 1e9, 1)
        if bytes_:
            d["GBs"] = round(bytes_ / ms / 1e6, 1)
        out[name] = d
        print(name, d, flush=True)

    def want(k):
        return not only or any(k.startswith(o) or o.startswith(k) for o in only)

    # ---- NT GEMMs
    for name, (m, n, k) in {"gemm_nt.ffn2[M,256,1024]": (M, 256, 1024), "gemm_nt.dH[M,1024,256]": (M, 1024, 256),
                            "gemm_nt.dxn2[M,256,1024]": (M, 256, 1024), "gemm_nt.swin_qkv1[200704,288,96]": (200704, 288, 96),
                            "gemm_nt.swin_fc1_1[200704,384,96]": (200704, 384, 96),
                            "gemm_nt.swin_fc2_1[200704,96,384]": (200704, 96, 384),
                            "gemm_nt.swin_fc1_3[12544,1536,384]": (12544, 1536, 384),
                            "gemm_nt.swin_fc2_3[12544,384,1536]": (12544, 384, 1536)}.items():
        if not want("gemm_nt"):
            break
        x, w = R(m, k), R(n, k) * 0.05
        b = torch.zeros(n, device=DEV)
        r = R(m, n)
        rec(name, timeit(lambda: ops.gemm_nt(x, w, b, res2d=r), a.rounds), 2.0 * m * n * k)
        rec(name + ".blas", timeit(lambda: torch.addmm(r, x, w.t()), a.rounds), 2.0 * m * n * k)
    if want("gemm_nt"):             # dH = dY W2 gated by the saved hidden activation (FFN backward)
        dy, w2t, h = R(M, 256), R(1024, 256) * 0.05, R(M, 1024)
        rec("gemm_nt.dH_gated[M,1024,256]", timeit(lambda: ops.gemm_nt(dy, w2t, gate=h, gate_scale=1.0 / 0.9), a.rounds), 2.0 * M * 1024 * 256)
    if want("gemm_nt"):             # the same product gated by the forward's sign bits
        x0, w1 = R(M, 256), R(1024, 256) * 0.05
        _, _, _, sg = ops.ln_gemm(x0, torch.ones(256, device=DEV), torch.zeros(256, device=DEV), w1, None, 1024, relu=True, drop_p=0.1,
                                  seed=3, want_signs=True)
        rec("gemm_nt.dH_signs[M,1024,256]", timeit(lambda: ops.gemm_nt_signs(dy, w2t, sg, 1.0 / 0.9), a.rounds), 2.0 * M * 1024 * 256,
            2.0 * M * (256 + 1024) + M * 128)
    # ---- LN-fused GEMMs
    if want("ln_gemm"):
        x = R(M, 256)
        gm, bt = torch.ones(256, device=DEV), torch.zeros(256, device=DEV)
        for n, relu in ((768, False), (1024, True)):
            w = R(n, 256) * 0.05
            b = torch.zeros(n, device=DEV)
            rec(f"ln_gemm[M,{n},256]", timeit(lambda: ops.ln_gemm(x, gm, bt, w, b, n, relu=relu), a.rounds), 2.0 * M * n * 256,
                2.0 * M * (256 + n + 256))
            if relu:
                rec(f"ln_gemm[M,{n},256].drop.signs", timeit(lambda: ops.ln_gemm(x, gm, bt, w, b, n, relu=True, drop_p=0.1, seed=7,
                                                                                   want_signs=True), a.rounds),
                    2.0 * M * n * 256, 2.0 * M * (256 + n + 256))
                rec(f"ln_gemm[M,{n},256].drop", timeit(lambda: ops.ln_gemm(x, gm, bt, w, b, n, relu=True, drop_p=0.1, seed=7), a.rounds),
                    2.0 * M * n * 256, 2.0 * M * (256 + n + 256))
            rec(f"ln_gemm[M,{n},256].blas_nolN", timeit(lambda: torch.addmm(b.to(BF), x, w.t()), a.rounds), 2.0 * M * n * 256)
    # ---- TN (weight gradient) GEMMs
    if want("gemm_tn"):
        for n, k in ((768, 256), (1024, 256), (256, 1024)):
            dy, x = R(M, n), R(M, k)
            rec(f"gemm_tn[{n},{k},M]", timeit(lambda: ops.gemm_tn(dy, x), a.rounds), 2.0 * M * n * k)
            rec(f"gemm_tn[{n},{k},M].blas", timeit(lambda: dy.t() @ x, a.rounds), 2.0 * M * n * k)
    # ---- the same for the encoder's widths (mtmp_gemm_tn's masked-tile kernel + reduction), each next to the path these
    #      products took before: fp32 copies of both operands, a library product and a separate column sum
    if want("gemm_tn"):
        lines, tot = [], [0.0, 0.0]
        for n, k, m in ENCODER_TN:
            dy, x = R(m, n), R(m, k)

            def lib_form():
                dyf = dy.float()
                return dyf.t() @ x.float(), dyf.sum(0)

            t_new, t_lib = timeit_pair(lambda: ops.gemm_tn(dy, x), lib_form, a.rounds)
            rec(f"gemm_tn[{n},{k},{m}]", t_new, 2.0 * m * n * k, 2.0 * (n + k) * m)
            rec(f"gemm_tn[{n},{k},{m}].cast_blas_sum", t_lib, 2.0 * m * n * k, 2.0 * (n + k) * m)
            tot[0] += t_new
            tot[1] += t_lib
            lines.append(f"{n:4d} x {k:4d}  {m:7d}  {t_new * 1e3:9.1f}  {t_lib * 1e3:9.1f}  {2.0 * (n + k) * m / t_new / 1e9:6.2f}")
            del dy, x
        lines.append(f"sum                   {tot[0] * 1e3:9.1f}  {tot[1] * 1e3:9.1f}")
        table = ("# dW = dY^T X, db = colsum(dY), bf16 operands, one process, forms alternating, min over %d rounds of 5 calls\n"
                 "# new: ops.gemm_tn (product + reduction); before: dy.float().t() @ x.float() and dy.float().sum(0)\n"
                 "# TB/s: 2 (N + K) M bytes / new time\n"
                 "#  N      K        M     new us  before us    TB/s\n" % a.rounds + "\n".join(lines) + "\n")
        print(table, end="", flush=True)
    # ---- shifted-window attention on the 512-pixel maps: mtmp_swin_window_attn_pad(_bwd) on the un-padded map next to the recipe
    #      it replaces -- the qkv map copied into a bias-filled map of the padded size, the window-multiple kernels on that map,
    #      crop (backward: dout zero-padded the same way, dqkv cropped, the pad tokens' dk / dv summed into the bias gradient)
    pad_table = ""
    if want("swin_pad"):
        lines, tot = [], [0.0, 0.0, 0.0, 0.0]
        n, shift = 64, 3
        for H, C, heads in SWIN_512:
            Hp = -(-H // 7) * 7
            qkv, dout = R(n, H, H, 3 * C), R(n, H, H, C)
            bias = torch.randn(3 * C, generator=g, device=DEV) * 0.3
            tab = (torch.randn(4, heads, 64, 64, generator=g, device=DEV) * 0.02)
            tab[..., 49:] = -30000.0
            tab = tab.to(BF)

            def copy_fwd():
                padded = bias.to(BF).expand(n, Hp, Hp, 3 * C).contiguous()
                padded[:, :H, :H] = qkv
                return ops.swin_window_attn(padded, tab, heads, shift)[:, :H, :H].contiguous()

            def copy_bwd():
                padded = bias.to(BF).expand(n, Hp, Hp, 3 * C).contiguous()
                padded[:, :H, :H] = qkv
                dpad = torch.zeros(n, Hp, Hp, C, dtype=BF, device=DEV)
                dpad[:, :H, :H] = dout
                dq, dtab = ops.swin_window_attn_bwd(padded, tab, dpad, heads, shift)
                db = dq.sum((0, 1, 2), dtype=torch.float32) - dq[:, :H, :H].sum((0, 1, 2), dtype=torch.float32)
                return dq[:, :H, :H].contiguous(), dtab, db

            f_new, f_old = timeit_pair_median(lambda: ops.swin_window_attn_pad(qkv, bias, tab, heads, shift), copy_fwd, a.rounds)
            b_new, b_old = timeit_pair_median(lambda: ops.swin_window_attn_pad_bwd(qkv, bias, tab, dout, heads, shift), copy_bwd, a.rounds)
            tag = f"[{n},{H},{H},{C}]"
            rec("swin_pad.fwd" + tag, f_new, bytes_=2.0 * n * H * H * 4 * C)
            rec("swin_pad.fwd" + tag + ".copy_kernel_crop", f_old)
            rec("swin_pad.bwd" + tag, b_new, bytes_=2.0 * n * H * H * 8 * C)
            rec("swin_pad.bwd" + tag + ".copy_kernel_crop", b_old)
            for i, v in enumerate((f_new, f_old, b_new, b_old)):
                tot[i] += v
            lines.append(f"{H:4d} x {H:4d} x {C:4d}  {f_new * 1e3:9.1f}  {f_old * 1e3:9.1f}  {b_new * 1e3:9.1f}  {b_old * 1e3:9.1f}")
            del qkv, dout
        lines.append("sum                 " + "".join(f"  {v * 1e3:9.1f}" for v in tot))
        pad_table = ("# shifted-window attention (shift 3) of 64 images at the four stage shapes of --image-size 512, bf16, one process, warm,\n"
                     "# forms alternating, median over %d rounds of 5 calls\n"
                     "# new: mtmp_swin_window_attn_pad / _pad_bwd on the un-padded map; copy: bias-filled padded copy + window-multiple kernel + crop\n"
                     "#   H      W      C     fwd new us  fwd copy us  bwd new us  bwd copy us\n" % a.rounds + "\n".join(lines) + "\n")
        print(pad_table, end="", flush=True)
    # ---- chest X-ray input chain (csrc/image_prep.hip): uint8 images -> float batch, three launches
    cxr_table = ""
    if want("cxr"):
        import time
        import numpy as np
        from medical_tri_modal_pilot_amd import _lib
        from medical_tri_modal_pilot_amd.builder.data.cxr_transform import CxrTransform, collate_raw_cxr
        from medical_tri_modal_pilot_amd.ops import _p, _stream
        rng = np.random.default_rng(0)

        def source(h, w):
            y, x = np.mgrid[0:h, 0:w]
            return np.clip(90 + 60 * np.sin(x / 37.0) * np.cos(y / 23.0) + 40 * (x / w) + rng.normal(0, 12, (h, w)), 0, 255).astype(np.uint8)

        def pil_ms(src, S):
            """the reference loader's chain on this box's CPU, one core, decode not included; None without PIL"""
            try:
                from PIL import Image, ImageOps
            except ImportError:
                return None
            from medical_tri_modal_pilot_amd.builder.data.cxr_transform import affine_matrix
            tr, im = CxrTransform(S, "resize_affine_crop", True), Image.fromarray(src)
            rh, rw = tr.resized(*src.shape)
            top, left = tr.crop(rh, rw)
            reps = 20
            t0 = time.perf_counter()
            for _ in range(reps):
                r = ImageOps.equalize(im).resize((rw, rh), Image.BILINEAR)
                r = r.transform((rw, rh), Image.AFFINE, affine_matrix(rw, rh, 3.0, 10, -7, 1.05), Image.NEAREST, fillcolor=0)
                np.asarray(r.crop((left, top, left + S, top + S)), dtype=np.float32) / 255
            return (time.perf_counter() - t0) / reps * 1e3

        lines = []
        for (h, w), S in (((256, 311), 224), ((585, 711), 512)):
            cpu = pil_ms(source(h, w), S)
            for n in (64, 192):
                srcs = [source(h, w) for _ in range(8)]
                raw = collate_raw_cxr([([srcs[i % 8]], [-1.0]) for i in range(n)], CxrTransform(S, "resize_affine_crop", True), 0,
                                      generator=torch.Generator().manual_seed(1)).to(DEV)
                hist = torch.zeros(n, 256, dtype=torch.int32, device=DEV)
                scratch = torch.empty(raw.scratch_bytes, dtype=torch.uint8, device=DEV)
                dst = torch.empty(raw.out_shape, device=DEV)
                t_h = timeit(lambda: _lib.call("mtmp_cxr_hist", _p(raw.pixels), _p(raw.desc), _p(hist), n, raw.max_pixels, _stream()), a.rounds)
                hist = ops.cxr_hist(raw.pixels, raw.desc, raw.max_pixels)
                t_r = timeit(lambda: _lib.call("mtmp_cxr_resize", _p(raw.pixels), _p(raw.desc), _p(raw.tables), _p(hist), _p(scratch), n,
                                               raw.max_rh, raw.max_rw, raw.lds_rows, _stream()), a.rounds)
                t_a = timeit(lambda: _lib.call("mtmp_cxr_affine_crop", _p(scratch), _p(raw.desc), _p(raw.slot_map), _p(dst), n, S, _stream()), a.rounds)
                t_all = timeit(lambda: ops.cxr_prepare(raw), a.rounds)
                tag = f"[{n}x{h}x{w}->{S}]"
                rec("cxr.hist" + tag, t_h, bytes_=float(n * h * w))
                rec("cxr.resize" + tag, t_r, bytes_=float(n * h * w + raw.scratch_bytes))
                rec("cxr.affine_crop" + tag, t_a, bytes_=float(n * S * S * 5))
                rec("cxr.prepare" + tag, t_all)
                tot = t_h + t_r + t_a
                cpu_s = "PIL not installed; 0.39 ms per 256x311 image per core was measured on a CPU-only machine" if cpu is None \
                    else f"{cpu:7.3f} ms/image/core = {1e3 / cpu:8.0f} images/s/core (PIL {__import__('PIL').__version__}, this box's CPU)"
                lines.append(f"{n:4d} x {h} x {w} -> {S}: hist {t_h * 1e3:7.1f}  resize {t_r * 1e3:7.1f}  affine_crop {t_a * 1e3:7.1f}  sum {tot * 1e3:8.1f} us"
                             f"  ({n / tot * 1e3:10.0f} images/s; ops.cxr_prepare with its allocations and zero-fill {t_all * 1e3:8.1f} us); CPU chain: {cpu_s}")
        cxr_table = ("# chest X-ray input chain, resize_affine_crop, uint8 sources already on the device, one process, warm, median over %d rounds of 5 calls\n"
                     % a.rounds + "\n".join(lines) + "\n")
        # the random chains (csrc/image_aug.hip): launches and us per batch of 64 images of 256 x 311 -> 224, ops and boxes drawn
        from medical_tri_modal_pilot_amd.builder.data.cxr_transform import CxrRandomTransform, draw_randaug, draw_resized_crop

        def pil_random_ms(src, S, randaug):
            """RandAugment (when asked for) + RandomResizedCrop by the PIL calls they are on an L image, one core, drawn per repetition"""
            try:
                from PIL import Image, ImageOps
            except ImportError:
                return None
            spec = importlib.util.spec_from_file_location("make_golden_cxr_aug", os.path.join(ROOT, "tests", "golden", "gen", "make_golden_cxr_aug.py"))
            gen = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(gen)
            im, g, reps = Image.fromarray(src), torch.Generator().manual_seed(2), 40
            plans = [(draw_randaug(*src.shape, g) if randaug else [], draw_resized_crop(*src.shape, g)) for _ in range(reps)]
            t0 = time.perf_counter()
            for ops_, (bi, bj, bh, bw) in plans:
                r = ImageOps.equalize(im)
                for op, m in ops_:
                    r = gen.apply_op(r, op, m)
                np.asarray(r.crop((bj, bi, bj + bw, bi + bh)).resize((S, S), Image.BILINEAR), dtype=np.float32) / 255
            return (time.perf_counter() - t0) / reps * 1e3

        import importlib.util
        lines, (h, w), S, n = [], (256, 311), 224, 64
        srcs = [source(h, w) for _ in range(8)]
        for kind in ("random", "randaug"):
            raw = collate_raw_cxr([([srcs[i % 8]], [-1.0]) for i in range(n)], CxrRandomTransform(S, kind), 0,
                                  generator=torch.Generator().manual_seed(1)).to(DEV)
            launches = 2 + bin(raw.stages).count("1")
            t_all = timeit(lambda: ops.cxr_prepare(raw), a.rounds)
            rec(f"cxr.prepare.{kind}[{n}x{h}x{w}->{S}]", t_all)
            cpu = pil_random_ms(srcs[0], S, kind == "randaug")
            cpu_s = "PIL not installed" if cpu is None else f"{cpu:7.3f} ms/image/core (PIL {__import__('PIL').__version__}, this box's CPU)"
            lines.append(f"{kind:8s} {n:4d} x {h} x {w} -> {S}: {launches} launches, ops.cxr_prepare with its allocations and zero-fill "
                         f"{t_all * 1e3:8.1f} us  ({n / t_all * 1e3:10.0f} images/s); CPU chain: {cpu_s}")
        cxr_table += ("# random chains (RandomResizedCrop; RandAugment in front of it), ops and boxes drawn with seed 1, same conditions\n"
                      + "\n".join(lines) + "\n")
        print(cxr_table, end="", flush=True)
    # ---- attention
    if want("attn"):
        B, N = 64, 1005
        qkv = R(B, N, 768)
        res, do = R(B, N, 256), R(B, N, 256)
        kv = torch.full((B,), N, dtype=torch.int32, device=DEV)
        f = 4.0 * B * 4 * N * N * 64
        rec("attn_fwd[64,1005].online", timeit(lambda: ops.attn_fwd(qkv, kv, res=res), a.rounds), f)
        kn = ops.key_norms(qkv)
        rec("key_norms[64,1005]", timeit(lambda: ops.key_norms(qkv), a.rounds), bytes_=2.0 * B * N * 256)
        rec("attn_fwd[64,1005].bounded", timeit(lambda: ops.attn_fwd(qkv, kv, res=res, knorm=kn), a.rounds), f)
        qs = qkv * 0.35                # scores of the size a LayerNorm-fed projection produces
        kn2 = ops.key_norms(qs)
        rec("attn_fwd[64,1005].bounded.smallscores", timeit(lambda: ops.attn_fwd(qs, kv, res=res, knorm=kn2), a.rounds), f)
        o, _, lse = ops.attn_fwd(qkv, kv, res=res)
        rec("attn_bwd[64,1005]", timeit(lambda: ops.attn_bwd(qkv, o, do, lse, kv), a.rounds), 2.5 * f)
    # ---- streaming kernels
    if want("stream"):
        z, dy = R(M, 256), R(M, 256)
        st = torch.stack([z.float().mean(-1), 1 / (z.float().std(-1) + 1e-6)], 1).contiguous()
        gm = torch.ones(256, device=DEV)
        rec("ln_bwd[M,256]", timeit(lambda: ops.ln_bwd(z, st, gm, dy, dy), a.rounds), bytes_=4.0 * M * 256 * 2)
        x = R(64, 56, 56, 96)
        w, b = torch.ones(96, device=DEV), torch.zeros(96, device=DEV)
        rec("ln_rows[200704,96]", timeit(lambda: ops.layernorm_rows(x, w, b), a.rounds), bytes_=2.0 * x.numel() * 2)
    # ---- the fused FFN block of the inference forward against the training forward's chain (ln_gemm_signs + gemm_nt): both forms
    # in this process, warm, alternating window by window; median with min and max.  Small row counts get more calls per window
    ffn_table = ""
    if want("ffn_block"):
        gm, bt = torch.ones(256, device=DEV), torch.zeros(256, device=DEV)
        w1, w2 = R(1024, 256) * 0.08, R(256, 1024) * 0.03
        c1, c2 = torch.randn(1024, generator=g, device=DEV) * 0.3, torch.randn(256, generator=g, device=DEV) * 0.3
        ffn_table = ("# mtmp_ffn_block against mtmp_ln_gemm_signs + mtmp_gemm_nt, bf16, us per call, one process, warm, forms alternating,\n"
                     "# median (min .. max) over %d windows\n# M        fused                      chain                      chain / fused\n"
                     % max(a.rounds, 7))
        for m in (64 * 1010, 64 * 137, 64 * 58, 1024, 512, 256, 64):
            x = (R(m, 256) + 0.3) * 2
            inner = 5 if m > 4096 else 40

            def chain():
                h = ops.ln_gemm_signs_grouped([x], [gm], [bt], [w1], [c1], 1024, 0.0, [0])[0]
                return ops.gemm_nt_grouped(h, [w2], [c2], [x], 0.0, [0])

            def fused():
                return ops.ffn_block_grouped([x], [gm], [bt], [w1], [c1], [w2], [c2])

            for _ in range(3):
                fused()
                chain()
            ts = ([], [])
            for _ in range(max(a.rounds, 7)):
                for i, fn in enumerate((fused, chain)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(inner):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    ts[i].append(1e3 * e0.elapsed_time(e1) / inner)
            med = [sorted(t)[len(t) // 2] for t in ts]
            rec(f"ffn_block[{m}].fused", med[0] / 1e3, 2.0 * m * 2 * 256 * 1024)
            rec(f"ffn_block[{m}].chain", med[1] / 1e3, 2.0 * m * 2 * 256 * 1024)
            ffn_table += "%-8d %8.1f (%6.1f .. %6.1f)  %8.1f (%6.1f .. %6.1f)  %.2f\n" % (
                m, med[0], min(ts[0]), max(ts[0]), med[1], min(ts[1]), max(ts[1]), med[1] / med[0])
        print(ffn_table, flush=True)
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(ROOT, "gpurun_out", "bench_kernels.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    if pad_table:                    # the padded-window table, next to the JSON
        with open(os.path.join(os.path.dirname(fh.name), "swin_padded_windows.txt"), "w") as ft:
            ft.write(pad_table)
    if cxr_table:
        with open(os.path.join(os.path.dirname(fh.name), "cxr_input_pipeline_table.txt"), "w") as ft:
            ft.write(cxr_table)
    if ffn_table:
        with open(os.path.join(os.path.dirname(fh.name), "ffn_block_table.txt"), "w") as ft:
            ft.write(ffn_table)
    if table:                        # the encoder-width table, next to the JSON
        with open(os.path.join(os.path.dirname(fh.name), "gemm_tn_encoder_widths.txt"), "w") as ft:
            ft.write(table)


if __name__ == "__main__":
    main()
