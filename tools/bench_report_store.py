"""Times of the report path (builder/data/report_store.py, csrc/report_store.hip) on one MI355X against the host path it
replaces: the figures of profiles/report_store.txt.

    python tools/bench_report_store.py [--batch 64] [--rounds 30] [--inner 20] [--workloads full,ragged] [--out FILE]

(a) the parent's path of one batch: the float32 [B, 128, 768] tensor the reference's loader and collate hand over, from pageable
    and from pinned host memory, ``.to(device)`` as the trainer does it, alone and followed by the bf16 build's ``.to(bfloat16)``
    launch -- device events around ``inner`` repetitions, and the host clock around one call that ends in a synchronise;
(b) ``ops.report_tokens`` from a float32 and from a bfloat16 store of seeded synthetic reports, into float32 and bfloat16,
    on two workloads: `full` (B distinct reports of 128 tokens) and `ragged` (``make_batch``'s lengths, 40 % of the samples missing):
    launches back to back with the descriptor already on the device by device events (an upper bound on the kernel: for
    its own time run the tool under ``rocprofv3 --kernel-trace --stats``, in a run of its own), the whole call with its descriptor copy and a
    synchronise by the host clock, and ``store.plan`` on the host.
Alternating rounds: every round times every variant once, the medians are over the rounds.  The bytes a variant moves are
computed from the shapes.  Every gathered batch is compared with the parent path's tensor first.  Needs a GPU; no fallback."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools._timing import Lines, device_ms, median as med, wall_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--reports", type=int, default=2048)
    ap.add_argument("--workloads", default="full,ragged")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_report_store: needs an MI355X (no CPU fallback)")
    from medical_tri_modal_pilot_amd import ops, synthetic
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    F32, BF16 = torch.float32, torch.bfloat16
    B, L, W = a.batch, 128, 768
    say, wall_time = Lines(), wall_ms
    dev_time = lambda fn: device_ms(fn, a.inner)
    say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; B {B}, L {L}, W {W}; {a.rounds} alternating rounds, "
        f"device-event figures over {a.inner} calls back to back")
    # the store: B distinct reports of L tokens (the `full` workload reads every one of them once: no report is served from a
    # cache because another sample has just read it), then reports with make_batch's lengths, uniform on 1..L - 2
    from medical_tri_modal_pilot_amd.builder.data import ReportStore
    g = torch.Generator().manual_seed(5003)
    n_each = [L] * B + torch.randint(1, L - 1, (a.reports - B,), generator=g).tolist()
    mapping = {f"report {i}": {"embedding": torch.randn(n, W, generator=g).numpy()} for i, n in enumerate(n_each)}
    host = ReportStore.from_mapping(mapping)
    emb32 = host.emb.clone()
    stores = {F32: ReportStore.from_mapping(mapping).to(dev, F32), BF16: ReportStore.from_mapping(mapping).to(dev, BF16)}
    del mapping
    for dt, st in stores.items():
        say(f"store[{dt}]: {st.n_reports} reports, {st.n_tokens} tokens, {st.nbytes} bytes on the device = {st.nbytes // st.n_tokens} per token")

    rng = np.random.default_rng(7)
    n_tok = np.diff(host.tok_ptr)
    full_idx = np.arange(B, dtype=np.int64)                                   # B distinct 128-token reports: every row is read
    mb = synthetic.make_batch(99, B, 8, missing_mode="none")                  # its txt_lengths: uniform on 1..126
    want_len = mb["txt_lengths"].numpy().copy()
    want_len[rng.random(B) < 0.4] = 0                                         # 40 % missing
    order = np.argsort(n_tok, kind="stable")
    ragged_idx = np.asarray([-1 if n == 0 else int(order[np.searchsorted(n_tok[order], n)]) for n in want_len], np.int64)
    for kind, idx in [w for w in (("full", full_idx), ("ragged", ragged_idx)) if w[0] in a.workloads.split(",")]:
        plans = {dt: st.plan(idx) for dt, st in stores.items()}
        lens = plans[F32].txt_lengths
        x_page = torch.stack([torch.cat([emb32[f:f + n], torch.zeros([L - n, W])], dim=0)      # the loader's padding, the collate's stack
                              for f, n in zip(plans[F32].first_token.tolist(), plans[F32].n_tokens.tolist())])
        x_pin = x_page.pin_memory()
        live = int(lens.sum())
        say(f"[{kind}] lengths {int(lens.min())}..{int(lens.max())}, mean {float(lens.float().mean()):.1f}, {int((lens == 0).sum())} of {B} "
            f"missing; token rows in the batch {live} of {B * L}")
        # results first
        ref = x_page.to(dev)
        for src in (F32, BF16):
            for dst in (F32, BF16):
                got = ops.report_tokens(plans[src], dev, dst)
                exp = (ref if src == F32 else ref.to(BF16)).to(dst)
                assert torch.equal(got, exp), (kind, src, dst)
        say(f"[{kind}] gather == parent path in all four type pairs")
        variants = {
            "parent pageable .to(device)": lambda: x_page.to(dev, non_blocking=True),
            "parent pageable .to(device) + .to(bf16)": lambda: x_page.to(dev, non_blocking=True).to(BF16),
            "parent pinned .to(device)": lambda: x_pin.to(dev, non_blocking=True),
            "parent pinned .to(device) + .to(bf16)": lambda: x_pin.to(dev, non_blocking=True).to(BF16),
        }
        moved = {"parent pageable .to(device)": (B * L * W * 4, 0), "parent pinned .to(device)": (B * L * W * 4, 0),
                 "parent pageable .to(device) + .to(bf16)": (B * L * W * 4, B * L * W * 6),
                 "parent pinned .to(device) + .to(bf16)": (B * L * W * 4, B * L * W * 6)}
        launch = {}
        for src in (F32, BF16):
            for dst in (F32, BF16):
                name = f"report_tokens {str(src)[6:]} store -> {str(dst)[6:]}"
                desc = plans[src].descriptor().to(dev)
                out = torch.empty(B, L, W, dtype=dst, device=dev)
                variants[name] = (lambda p=plans[src], d=dst: ops.report_tokens(p, dev, d))
                launch[name] = (lambda p=plans[src], d=dst, o=out, t=desc: ops.report_tokens(p, dev, d, out=o, tables=t))
                moved[name] = (B * 16, live * W * (4 if src == F32 else 2) + B * L * W * (4 if dst == F32 else 2))
        for fn in list(variants.values()) + list(launch.values()):           # warm every shape
            fn()
        torch.cuda.synchronize()
        t_dev, t_wall, t_launch = ({k: [] for k in variants} for _ in range(3))
        for _ in range(a.rounds):
            for k, fn in variants.items():
                t_dev[k].append(dev_time(fn))
                t_wall[k].append(wall_time(fn))
                if k in launch:
                    t_launch[k].append(dev_time(launch[k]))
        for k in variants:
            h2d, onchip = moved[k]
            s = (f"[{kind}] {k}: {1e3 * med(t_dev[k]):.1f} us per call by device events (min {1e3 * min(t_dev[k]):.1f}, max "
                 f"{1e3 * max(t_dev[k]):.1f}), {1e3 * med(t_wall[k]):.1f} us by the host clock with a synchronise; host-to-device "
                 f"{h2d} bytes, device reads + writes {onchip} bytes")
            if k in launch:
                s += (f"; with the descriptor already on the device {1e3 * med(t_launch[k]):.1f} us per launch back to back (min "
                      f"{1e3 * min(t_launch[k]):.1f}, max {1e3 * max(t_launch[k]):.1f}: an upper bound on the kernel, the window holds the "
                      f"host's enqueue of every launch)")
            say(s)
        tp = [wall_ms(lambda: stores[F32].plan(idx), sync=False) for _ in range(a.rounds)]
        say(f"[{kind}] store.plan on the host: {1e3 * med(tp):.0f} us per batch")
    say.write(a.out)


if __name__ == "__main__":
    main()
