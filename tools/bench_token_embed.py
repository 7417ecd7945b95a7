"""Times of the token-id report path (builder/data/report_store.TokenReportStore, csrc/token_embed.hip) on one MI355X against
the torch path it replaces: the figures of profiles/token_embed.txt.

    python tools/bench_token_embed.py [--batches 64,128] [--rounds 30] [--inner 20] [--out FILE]

Per batch size B (L 128, V 30000, D 256; report lengths drawn as ``synthetic.make_token_report_store`` draws them, uniform on
0..160, 40 % of the samples missing) and per compute type:
(a) the parent's path: the float32 [B, L] host tensor of the loader ``.to(device)`` + ``.long()`` + ``F.embedding`` + ``.to(dt)``
    forward; ``embedding_dense_backward`` (behind the cast's backward, ``dy.float()``, in the bf16 build) plus the ``add_`` into
    the table's slice of a flat gradient buffer, which is what AccumulateGrad does, backward;
(b) the new path: ``ops.report_token_ids`` + ``ops.token_embed_fwd`` forward, ``ops.token_embed_bwd`` into the (zeroed) slice
    backward.
Device events around ``inner`` calls back to back; every round times every variant once (alternating rounds), medians with
extremes over the rounds.  For the kernels' own times run the tool under ``rocprofv3 --kernel-trace --stats``, in a run of its
own.  Results are compared first: forward bits equal, the gradient inside the float32 summation bound.  Needs a GPU; no fallback."""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools._timing import Lines, device_ms, median as med  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,128")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--reports", type=int, default=2048)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_token_embed: needs an MI355X (no CPU fallback)")
    from medical_tri_modal_pilot_amd import ops, synthetic
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    F32, BF16 = torch.float32, torch.bfloat16
    L, V, D = 128, 30000, 256
    C = ops.token_embed_chunk()
    say = Lines()
    dev_time = lambda fn: device_ms(fn, a.inner)
    say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; L {L}, V {V}, D {D}, chunk {C}; {a.rounds} alternating "
        f"rounds, device-event figures over {a.inner} calls back to back")
    host = synthetic.make_token_report_store(5011, n_reports=a.reports)
    host_ids = host.ids.numpy().copy()
    store = synthetic.make_token_report_store(5011, n_reports=a.reports).to(dev)
    say(f"token store: {store.n_reports} reports, {store.n_tokens} ids, {store.nbytes} bytes on the device")
    g = torch.Generator().manual_seed(17)
    w32 = torch.randn(V, D, generator=g).to(dev)
    tables = {F32: w32, BF16: w32.to(BF16)}                   # (the optimizer's bf16 shadow of the table)
    flat = torch.zeros(V * D + 4096, device=dev)              # a flat gradient buffer; the table's slice begins 16 bytes in
    dslice = flat[4:4 + V * D].view(V, D)
    rng = np.random.default_rng(7)
    for B in [int(b) for b in a.batches.split(",")]:
        T = B * L
        idx = rng.integers(0, store.n_reports, B).astype(np.int64)
        idx[rng.random(B) < 0.4] = -1                         # 40 % missing
        plan = store.plan(idx)
        x_host = torch.stack([torch.cat([torch.tensor([2.0] + [float(v) for v in host_ids[f:f + min(n, L - 2)]] + [3.0]),
                                         torch.zeros(L - 2 - min(n, L - 2))]) if n else torch.zeros(L)
                              for f, n in zip(plan.first_token.tolist(), plan.n_tokens.tolist())])
        x_host[x_host == 1] = 0
        ids = ops.report_token_ids(plan, dev)
        assert torch.equal(ids.cpu().float(), x_host)
        cnt = torch.bincount(ids.flatten().long(), minlength=V).cpu()
        top = torch.topk(cnt, 4)
        say(f"[B {B}] T {T}: report lengths {int(plan.txt_lengths.min())}..{int(plan.txt_lengths.max())}, {int((plan.txt_lengths == 0).sum())} "
            f"of {B} missing; {int((cnt > 0).sum())} ids have a token; longest position lists "
            f"{[(int(i), int(n)) for n, i in zip(top.values, top.indices)]} (id, rows); {int((cnt > C).sum())} lists longer than a chunk of "
            f"{C}, {int((cnt == 1).sum())} of one row")
        for dt in (BF16, F32):
            tag = str(dt)[6:]
            dy = torch.randn(T, D, generator=g).to(dt).to(dev)
            ids_long = ids.long()
            # results first
            want = F.embedding(ids_long, w32).to(dt)
            got = ops.token_embed_fwd(ids, tables[dt], dt)
            assert torch.equal(got.view(torch.int16 if dt == BF16 else torch.int32), want.view(torch.int16 if dt == BF16 else torch.int32))
            ref = torch.zeros(V, D, dtype=torch.float64, device=dev).index_add_(0, ids_long.flatten(), dy.double())
            mag = torch.zeros(V, D, dtype=torch.float64, device=dev).index_add_(0, ids_long.flatten(), dy.double().abs())
            flat.zero_()
            ops.token_embed_bwd(ids, dy, dslice)
            err = (dslice.double() - ref).abs()
            assert bool((err <= cnt.to(dev).double().unsqueeze(1) * 2.0 ** -24 * mag).all())
            dense = torch.ops.aten.embedding_dense_backward(dy.float(), ids_long, V, -1, False)
            say(f"[B {B} {tag}] forward bits equal F.embedding(...).to({tag}); gradient: max |new - float64| {float(err.max()):.3g}, "
                f"max |embedding_dense_backward - float64| {float((dense.double() - ref).abs().max()):.3g}")
            x_pin = x_host.pin_memory()

            def parent_fwd():
                return F.embedding(x_pin.to(dev, non_blocking=True).long(), w32).to(dt)

            def parent_bwd():
                dslice.add_(torch.ops.aten.embedding_dense_backward(dy.float() if dt == BF16 else dy, ids_long, V, -1, False))

            def new_fwd():
                return ops.token_embed_fwd(ops.report_token_ids(plan, dev), tables[dt], dt)

            def new_bwd():
                ops.token_embed_bwd(ids, dy, dslice)
            variants = {"(a) parent forward: .to(device) + .long() + F.embedding + .to(dt)": parent_fwd,
                        "(b) new forward: report_token_ids + token_embed_fwd": new_fwd,
                        "(a) parent backward: embedding_dense_backward + add_ into the flat slice": parent_bwd,
                        "(b) new backward: token_embed_bwd into the flat slice": new_bwd}
            touched = int((cnt > 0).sum())
            esz = 2 if dt == BF16 else 4
            moved = {"(a) parent forward: .to(device) + .long() + F.embedding + .to(dt)":
                         T * 4 + T * 12 + T * D * 8 + (T * D * 6 if dt == BF16 else 0),
                     "(b) new forward: report_token_ids + token_embed_fwd": T * 8 + T * D * 2 * esz,
                     "(a) parent backward: embedding_dense_backward + add_ into the flat slice":
                         (T * D * 6 if dt == BF16 else 0) + V * D * 4 + T * D * 4 + touched * D * 8 + 3 * V * D * 4,
                     "(b) new backward: token_embed_bwd into the flat slice": T * D * esz + touched * D * 4 + 5 * T * 4}
            for fn in variants.values():
                fn()
            torch.cuda.synchronize()
            times = {k: [] for k in variants}
            for _ in range(a.rounds):
                for k, fn in variants.items():
                    times[k].append(dev_time(fn))
            for k in variants:
                say(f"[B {B} {tag}] {k}: {1e3 * med(times[k]):.1f} us per call (min {1e3 * min(times[k]):.1f}, max "
                    f"{1e3 * max(times[k]):.1f}); about {moved[k] / 1e6:.2f} MB of device traffic by the shapes")
    say.write(a.out)


if __name__ == "__main__":
    main()
