"""Times of the event-window path (builder/data/tie_store.py, csrc/tie_store.hip) on one MI355X against the host path it
replaces: the figures of profiles/tie_store.txt.

    python tools/bench_tie_store.py [--batch 64] [--rounds 20] [--steps 8] [--out FILE]

Two workloads on synthetic.make_tie_store: `full` (B windows of 24 dense hours, 1218 rows cut at TIE-len 1000) and `ragged`
(windows of 1..24 hours over dense and sparse patients: row counts spread over about 20..1000 -- an approximation of the ragged
benchmark workload, whose lengths are uniform on 3..1000, not the same distribution).  Per workload: the host path of one batch --
tie_window x B, collate_packed, PackedTieBatch.on_device with the 4096 bucket -- as wall time on ONE core of this box
(torch.set_num_threads(1)); store.plan; mtmp_tie_window_gather alone (device events, warm, median) and between the replayed
hipGraph steps of a 6-layer model (the mtmp_timestamp marks DESIGN section 7 uses); the store's bytes.  Every gathered batch is compared with
the host path's first.  Needs a GPU; there is no fallback."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools._timing import Lines, device_ms, median, wall_ms  # noqa: E402


def pick_windows(store, patients, B, kind, rng):
    """full: 24-hour windows of the dense patients; ragged: windows over every patient whose event counts spread over 0..1200"""
    dense = [p for p in range(store.n_patients) if p % 4 == 0]
    w = []
    while len(w) < B:
        p = dense[len(w) % len(dense)] if kind == "full" or rng.random() < 0.6 else int(rng.integers(store.n_patients))
        H = int(store.hour_ptr[p + 1] - store.hour_ptr[p])
        key = int(rng.integers(23, H))
        L = 24 if kind == "full" else int(rng.integers(1, 25))
        if any(a is not None for a in patients[p]["data_in_time"][key - L + 1:key + 1]):
            w.append((p, key, L))
    return np.asarray(w, np.int64)


def host_ms(fn, rounds):
    """median ms of ``fn`` by the host clock alone (host work, or a call that synchronises by itself)"""
    return median([wall_ms(fn, sync=False) for _ in range(rounds)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from medical_tri_modal_pilot_amd import ops, synthetic
    from medical_tri_modal_pilot_amd.builder.data import TieEventStore, collate_packed, tie_window
    from medical_tri_modal_pilot_amd.builder.trainer import get_trainer
    from medical_tri_modal_pilot_amd.builder.utils.cosine_annealing_with_warmup_v2 import CosineAnnealingWarmupRestarts
    from medical_tri_modal_pilot_amd.control.config import build_parser
    from medical_tri_modal_pilot_amd.train import _Logger, build_training
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.set_num_threads(1)
    say = Lines()
    patients, fmin, fmax = synthetic.make_tie_patients(4099, 64)
    store = TieEventStore.from_patients(patients, fmin, fmax).to(dev)
    say(f"store: {store.n_patients} patients, {store.n_hours} patient-hours, {store.n_events} events, {store.nbytes} bytes on the device = "
        f"{store.nbytes_hours / store.n_hours:.1f} bytes per patient-hour + {store.nbytes_events / max(store.n_events, 1):.1f} per event")
    T, B = 1000, a.batch
    args = build_parser().parse_args(
        ["--input-types", "vslt_img_txt", "--model", "tri_mbt_vsltcls", "--modality-inclusion", "train-missing_test-missing",
         "--batch-size", str(B), "--transformer-num-layers", "6", "--vslt-type", "TIE", "--imgtxt-time", "1", "--mbt-only-vslt", "1",
         "--TIE-len", str(T), "--compute-dtype", "bf16", "--hip-graph", "1", "--synthetic", "1"])
    model, opt, crit = build_training(args, dev, False)
    model.train()
    sched = CosineAnnealingWarmupRestarts(opt, first_cycle_steps=args.t_0 * 100, cycle_mult=args.t_mult, max_lr=args.lr_init * 8,
                                          min_lr=1e-6, warmup_steps=args.t_up * 100, gamma=args.gamma)
    rng = np.random.default_rng(3)
    it = 0
    for kind in ("full", "ragged"):
        wins = pick_windows(store, patients, B, kind, rng)

        def host_rows():
            out = []
            for p, key, L in wins.tolist():
                q = patients[p]
                ev, _, key2 = tie_window(q["data"], q["delta"], q["data_in_time"], key, L, fmin, fmax, 24, T, 1, True)
                out.append((ev, np.asarray([1.0 if q["gender"] == "M" else 0.0, q["age"]], np.float32), float(-key2)))
            return out

        def host_path():
            pb = collate_packed(host_rows())
            pk = pb.on_device(dev, 1000, 4096)
            torch.cuda.synchronize()
            return pk
        batch = store.plan(wins, T, 1)
        want, got = host_path(), ops.tie_windows(batch, dev, 1000, bucket=4096)
        assert torch.equal(want.events, got.events) and torch.equal(want.cu_seqlens, got.cu_seqlens)
        lens = batch.input_lengths
        say(f"[{kind}] B {B}, TIE-len {T}: rows {int(lens.min())}..{int(lens.max())}, mean {float(lens.float().mean()):.0f}, "
            f"{batch.total_rows} in the batch; gather == host path")
        t_rows, t_host = host_ms(host_rows, a.rounds), host_ms(host_path, a.rounds)
        say(f"[{kind}] host path, one core: tie_window x {B} {t_rows:.2f} ms, with collate_packed + on_device(bucket 4096) "
            f"{t_host:.2f} ms per batch = {t_host / B:.3f} ms per sample")
        say(f"[{kind}] store.plan: {1e3 * host_ms(lambda: store.plan(wins, T, 1), a.rounds):.0f} us per batch")
        t_call = host_ms(lambda: (ops.tie_windows(batch, dev, 1000, bucket=4096), torch.cuda.synchronize()), a.rounds)
        desc, cu = batch.descriptor().to(dev), batch.cu_seqlens.to(dev)
        launch = lambda: ops.tie_windows(batch, dev, 1000, bucket=4096, out=got.events, tables=(desc, cu))
        ts = [device_ms(launch, 5) for _ in range(a.rounds + 2)]
        say(f"[{kind}] mtmp_tie_window_gather alone: {1e3 * median(ts[2:]):.1f} us per launch (device events, 5 launches back "
            f"to back); ops.tie_windows with its two small copies and a synchronise: {1e3 * t_call:.0f} us wall")
        # between replayed steps: the trainer gathers in front of every step; the marks bracket the launch on the stream
        bt = synthetic.make_batch(99, B, T, missing_mode="none")
        ops.marks_enable(dev, only=("k.tie_window_gather",))
        in_step = []
        for _ in range(5):                               # the stamps of the last of `steps` steps enqueued without a host wait
            for _ in range(a.steps):
                it += 1
                ops.marks_new_step()
                get_trainer(args=args, iteration=it, x=batch, static=batch.static, input_lengths=batch.input_lengths, y=bt["y"],
                            output_lengths=None, model=model, logger=_Logger(), device=dev, scheduler=sched, optimizer=opt,
                            criterion=crit, x_txt=bt["txt"], x_img=bt["img"], txt_lengths=bt["txt_lengths"],
                            imgtxt_time=(bt["img_time"], batch.txt_time), scaler=None, missing=bt["missing"], flow_type="train",
                            reports_tokens=None, reports_lengths=None, criterion_aux=(None, None))
            torch.cuda.synchronize()
            m = ops.marks_read()
            in_step.append(m[f"k.tie_window_gather.N{B}.0.e"] - m[f"k.tie_window_gather.N{B}.0.s"])
        ops.marks_disable()
        say(f"[{kind}] mtmp_tie_window_gather in front of replayed hipGraph steps (6 layers, bf16): median {median(in_step):.1f} us "
            f"between its stamps (the last of {a.steps} steps, five times: {', '.join(f'{v:.1f}' for v in in_step)}; the first group "
            f"holds the capture)")
    say.write(a.out)


if __name__ == "__main__":
    main()
