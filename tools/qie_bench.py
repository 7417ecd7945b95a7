"""Times of a ``--vslt-type QIE`` training step on one MI355X: the figures of profiles/qie.txt.

    python tools/qie_bench.py [--batch 64] [--tie-len 1000] [--layers 6] [--rounds 8] [--steps 20] [--out FILE]

train.py-style steps of tri_mbt_vsltcls --vslt-type QIE at the benchmark's shape (B 64, TIE-len 1000, 6 layers, bf16), replayed from a
hipGraph, with tuning.HIP_QIE on (ops.QieAddsFn, ops.StreamInputsQieFn, ops.QieHeadFn: csrc/qie.hip, csrc/head.hip) and off (the
torch chain: the launch sequence this model had before the switch existed).  Two models in ONE process, one per setting -- the switch is
read by forward() and frozen into the graph at its capture --, ``--rounds`` alternating windows of ``--steps`` replayed steps each, every
window by the host clock around a window that ends in a device synchronise.  Reported: median and min .. max over the windows, and the
first losses of both (the same synthetic batch and seed).  Needs a GPU; no fallback."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools._timing import Lines, median, wall_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--tie-len", type=int, default=1000)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qie_bench: needs an MI355X (no CPU fallback)")
    from medical_tri_modal_pilot_amd import synthetic, tuning
    from medical_tri_modal_pilot_amd.builder.trainer import get_trainer
    from medical_tri_modal_pilot_amd.builder.utils.cosine_annealing_with_warmup_v2 import CosineAnnealingWarmupRestarts
    from medical_tri_modal_pilot_amd.control.config import build_parser
    from medical_tri_modal_pilot_amd.train import _Logger, build_training
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    say = Lines()
    B, T = a.batch, a.tie_len
    argv = ["--input-types", "vslt_img_txt", "--model", "tri_mbt_vsltcls", "--modality-inclusion", "train-missing_test-missing",
            "--batch-size", str(B), "--transformer-num-layers", str(a.layers), "--vslt-type", "QIE", "--imgtxt-time", "1",
            "--mbt-only-vslt", "1", "--compute-dtype", "bf16", "--hip-graph", "1", "--synthetic", "1", "--TIE-len", str(T)]
    bt = synthetic.make_batch(99, B, T, ragged=False, missing_mode="none")
    static = torch.stack([bt["gen"], bt["age"]], 1)
    runs = {}
    for on in (True, False):
        torch.manual_seed(0)
        args = build_parser().parse_args(argv)
        model, opt, crit = build_training(args, dev, False)
        model.train()
        sched = CosineAnnealingWarmupRestarts(opt, first_cycle_steps=args.t_0 * 100, cycle_mult=args.t_mult, max_lr=args.lr_init * 8,
                                              min_lr=1e-6, warmup_steps=args.t_up * 100, gamma=args.gamma)
        runs[on] = dict(args=args, model=model, opt=opt, crit=crit, sched=sched, it=0, loss=None, first=None)

    def steps(on, n):
        r = runs[on]
        tuning.HIP_QIE = on                              # read by forward(): frozen into the graph at its capture
        for _ in range(n):
            r["it"] += 1
            _, r["loss"] = get_trainer(args=r["args"], iteration=r["it"], x=bt["x"], static=static, input_lengths=bt["input_lengths"],
                                       y=bt["y"], output_lengths=None, model=r["model"], logger=_Logger(), device=dev,
                                       scheduler=r["sched"], optimizer=r["opt"], criterion=r["crit"], x_txt=bt["txt"], x_img=bt["img"],
                                       txt_lengths=bt["txt_lengths"], imgtxt_time=(bt["img_time"], bt["txt_time"]), scaler=None,
                                       missing=bt["missing"], flow_type="train", reports_tokens=None, reports_lengths=None,
                                       criterion_aux=(None, None))
            if r["first"] is None:
                r["first"] = r["loss"]
    for on in (True, False):                             # capture and warm both before the first window
        steps(on, 5)
    times = {True: [], False: []}
    for _ in range(a.rounds):
        for on in (True, False):
            times[on].append(wall_ms(lambda: steps(on, a.steps)) / a.steps)
    tuning.HIP_QIE = True
    say(f"tri_mbt_vsltcls --vslt-type QIE on {torch.cuda.get_device_name(0)}: B {B}, TIE-len {T}, {a.layers} layers, bf16, hipGraph; "
        f"{a.rounds} alternating windows of {a.steps} steps per setting (wall / steps)")
    for on in (True, False):
        st = runs[on]["model"]._mtmp_graph_step.stats()
        ts = times[on]
        say(f"training step, HIP_QIE {'on ' if on else 'off'}: median {median(ts):.3f} ms (min {min(ts):.3f}, max {max(ts):.3f}); "
            f"{st['captures']} capture, {st['replays']} replays; first loss {runs[on]['first']:.5f}, last {runs[on]['loss']:.5f}")
    say.write(a.out)


if __name__ == "__main__":
    main()
