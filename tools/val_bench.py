"""Times of the validation pass on one MI355X: the figures of profiles/validation_pass.txt.

    python tools/val_bench.py [--windows 7] [--window-s 1.0] [--workloads full,ragged] [--out FILE]
    python tools/val_bench.py --infer-forward 0,1 [...]      validate() replayed under --infer-forward 0 and 1 (below)

At the benchmark's shape (bench.py WORKLOADS: batch 64, TIE-len 1000, 6 layers, bf16; `full` and `ragged`), in ONE process and
alternating, (a) the existing loop -- ``get_trainer(flow_type="test")`` per batch (eager launches, ``loss.item()`` per batch)
with ``Evaluator`` -- and (b) ``validate()`` with ``--hip-graph 1`` and ``DeviceEvaluator``.  Every shape is warmed first (for
(b): the warm-up step and the capture).  A timed window is one pass over K copies of the batch, K sized so that the window
lasts at least ``--window-s``; it ends with the pass's metrics (``performance_metric()`` / ``validate``'s own 64-byte copy) and a
device synchronise, so the ms per batch include 1/K of that.  Reported: median and min .. max over the windows.
Then ``performance_metric()`` alone at 1e5 and 1e6 stored predictions for both evaluators (Evaluator: a list of batches of 64,
as the loop leaves it; DeviceEvaluator: the same values in its buffers).

``--infer-forward 0,1`` replaces all of that by ONE comparison: ``validate()`` with ``--hip-graph 1`` under each listed setting of
``--infer-forward``, in one process on one box, windows alternating between the settings (a model of its own per setting: a flip
on one model would capture afresh every window).  Reported per workload and setting: ms per validation batch, replayed (median,
min .. max), and ``torch.cuda.max_memory_allocated`` of one pass of 4 batches above what was allocated before it.
Needs a GPU; no fallback."""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools._timing import Lines, median, wall_ms  # noqa: E402


def stats(xs):
    return median(xs), min(xs), max(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-s", type=float, default=1.0)
    ap.add_argument("--workloads", default="full,ragged")
    ap.add_argument("--metric-reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--infer-forward", default=None, help="e.g. 0,1: compare validate() under these settings instead")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("val_bench: needs an MI355X (no CPU fallback)")
    import bench
    from medical_tri_modal_pilot_amd import synthetic
    from medical_tri_modal_pilot_amd.builder.trainer import get_trainer, validate
    from medical_tri_modal_pilot_amd.builder.utils.device_evaluator import DeviceEvaluator
    from medical_tri_modal_pilot_amd.builder.utils.metrics import Evaluator
    from medical_tri_modal_pilot_amd.train import _Logger, build_training
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    say = Lines()

    say(f"validation pass on {torch.cuda.get_device_name(0)}: windows of >= {a.window_s} s, {a.windows} per variant, alternating")
    if a.infer_forward is not None:
        infer_compare(a, say, dev)
        say.write(a.out)
        return
    for wl in a.workloads.split(","):
        B, T, L, multi, n_img, ragged, miss_mode, _ = bench.WORKLOADS[wl]
        args = bench.make_args(wl, "bf16", 0.1, 1, 0, False)
        torch.manual_seed(412)
        model, _opt, crit = build_training(args, dev, False)
        model.train()
        bt = synthetic.make_batch(1234, B, T, ragged=ragged, missing_mode=miss_mode, multiimages=multi, n_images=n_img)
        d = {k: v.to(dev) for k, v in bt.items() if k != "missing"}
        static = torch.stack([d["gen"], d["age"]], 1)
        batch = (d["x"], static, d["y"], bt["input_lengths"], d["img"], d["img_time"], d["txt"], d["txt_lengths"], d["txt_time"],
                 bt["missing"], None, None)
        lg = _Logger(Evaluator(args))

        def eager_pass(k):
            model.eval()
            lg.evaluator.reset()
            total = 0.0
            for _ in range(k):
                x, st, y, il, img, it_, txt, tl, tt, miss, _f, _y2 = batch
                _, loss = get_trainer(args=args, iteration=1, x=x, static=st, input_lengths=il, y=y, output_lengths=None,
                                      model=model, logger=lg, device=dev, scheduler=None, optimizer=None, criterion=crit,
                                      x_txt=txt, x_img=img, txt_lengths=tl, imgtxt_time=(it_, tt), scaler=None, missing=miss,
                                      flow_type="test", reports_tokens=None, reports_lengths=None, criterion_aux=(None, None))
                total += loss
            res = lg.evaluator.performance_metric()
            model.train()
            return total / k, res

        dev_ev = {}

        def graph_pass(k):
            ev = dev_ev.get("ev")
            if ev is None or ev.capacity < k * B:
                ev = dev_ev["ev"] = DeviceEvaluator(args, dev, max(k * B, 4096 * B))
            r = validate(args, model, (batch for _ in range(k)), dev, crit, ev)
            return r["loss"], r["performance_metric"]

        def timed(fn, k):
            out = []
            return wall_ms(lambda: out.append(fn(k))) / k, out[0]

        # warm every shape (lazy initialisation, the eval graph's warm-up step and capture), then size K per variant
        eager_pass(3)
        graph_pass(4)
        ks = {}
        for name, fn in (("eager", eager_pass), ("graph", graph_pass)):
            ms, _ = timed(fn, 8)
            ks[name] = max(8, math.ceil(a.window_s * 1e3 * 1.15 / ms))
        times = {"eager": [], "graph": []}
        outs = {}
        for _ in range(a.windows):
            for name, fn in (("eager", eager_pass), ("graph", graph_pass)):
                ms, outs[name] = timed(fn, ks[name])
                times[name].append(ms)
        gs = model._mtmp_graph_eval.stats()
        say(f"[{wl}] batch {B}, TIE-len {T}, {L} layers, bf16, lengths {'ragged' if ragged else 'full'}, missing {miss_mode}")
        for name, what in (("eager", "get_trainer(flow_type='test') + Evaluator, eager launches"),
                           ("graph", "validate() --hip-graph 1 + DeviceEvaluator           ")):
            m, lo, hi = stats(times[name])
            say(f"  {what}: {m:8.3f} ms / batch (min {lo:.3f} .. max {hi:.3f}, {ks[name]} batches a window, "
                f"{ks[name] * m / 1e3:.2f} s a window)")
        me, mg = stats(times["eager"])[0], stats(times["graph"])[0]
        say(f"  ratio eager / graph {me / mg:.2f}; mean loss eager {outs['eager'][0]:.6f} graph {outs['graph'][0]:.6f}; metrics "
            f"eager {[float(v) for v in outs['eager'][1]]} graph {[float(v) for v in outs['graph'][1]]}")
        say(f"  eval graph: {gs['captures']} captures, {gs['replays']} replays, {gs['eager_over_budget']} eager steps past the budget")
        del model, lg, dev_ev
        torch.cuda.empty_cache()

    args = bench.make_args("full", "bf16", 0.1, 1, 0, False)
    g = torch.Generator().manual_seed(7)
    for n in (100000, 1000000):
        p = torch.sigmoid(2.0 * torch.randn(n, generator=g)).to(dev)
        t = (torch.rand(n, generator=g) < 0.3).float().to(dev)
        old = Evaluator(args)
        for lo in range(0, n, 64):
            old.add_batch(t[lo:lo + 64], p[lo:lo + 64])
        new = DeviceEvaluator(args, dev, n)
        new.pred.copy_(p)
        new.tgt.copy_(t.to(torch.uint8))
        new.ctr[0] = n
        new.appended = n
        res = {}
        tm = {"Evaluator": [], "DeviceEvaluator": []}
        for rep in range(a.metric_reps + 1):
            for name, ev in (("Evaluator", old), ("DeviceEvaluator", new)):
                new._metrics = None
                ms = wall_ms(lambda: res.update({name: ev.performance_metric()}))
                if rep:                                  # the first repetition warms
                    tm[name].append(ms)
        say(f"performance_metric() at {n} stored predictions ({a.metric_reps} repetitions after one warm-up):")
        for name in tm:
            m, lo, hi = stats(tm[name])
            say(f"  {name:16s}: {m:9.3f} ms (min {lo:.3f} .. max {hi:.3f}) -> {[float(v) for v in res[name]]}")
    say.write(a.out)


def infer_compare(a, say, dev):
    import copy
    import bench
    from medical_tri_modal_pilot_amd import synthetic
    from medical_tri_modal_pilot_amd.builder.trainer import validate
    from medical_tri_modal_pilot_amd.builder.utils.device_evaluator import DeviceEvaluator
    from medical_tri_modal_pilot_amd.train import build_training
    settings = [int(v) for v in a.infer_forward.split(",")]
    for wl in a.workloads.split(","):
        B, T, L, multi, n_img, ragged, miss_mode, _ = bench.WORKLOADS[wl]
        bt = synthetic.make_batch(1234, B, T, ragged=ragged, missing_mode=miss_mode, multiimages=multi, n_images=n_img)
        d = {k: v.to(dev) for k, v in bt.items() if k != "missing"}
        static = torch.stack([d["gen"], d["age"]], 1)
        batch = (d["x"], static, d["y"], bt["input_lengths"], d["img"], d["img_time"], d["txt"], d["txt_lengths"], d["txt_time"],
                 bt["missing"], None, None)
        runs = {}
        for s in settings:
            args = copy.copy(bench.make_args(wl, "bf16", 0.1, 1, 0, False))
            args.infer_forward = s
            torch.manual_seed(412)
            model, _opt, crit = build_training(args, dev, False)
            model.train()
            runs[s] = (args, model, crit, DeviceEvaluator(args, dev, 4096 * B))

        def run_pass(s, k):
            args, model, crit, ev = runs[s]
            return validate(args, model, (batch for _ in range(k)), dev, crit, ev)["loss"]

        peak, ks, loss = {}, {}, {}
        for s in settings:
            run_pass(s, 4)                                   # warm-up step and capture
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            run_pass(s, 4)
            torch.cuda.synchronize()
            peak[s] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
            ms = wall_ms(lambda: run_pass(s, 8)) / 8
            ks[s] = max(8, math.ceil(a.window_s * 1e3 * 1.15 / ms))
        times = {s: [] for s in settings}
        for _ in range(a.windows):
            for s in settings:
                out = []
                times[s].append(wall_ms(lambda: out.append(run_pass(s, ks[s]))) / ks[s])
                loss[s] = out[0]
        say(f"[{wl}] batch {B}, TIE-len {T}, {L} layers, bf16, lengths {'ragged' if ragged else 'full'}, missing {miss_mode}; "
            f"validate() --hip-graph 1, replayed")
        for s in settings:
            m, lo, hi = stats(times[s])
            gs = runs[s][1]._mtmp_graph_eval.stats()
            say(f"  --infer-forward {s}: {m:8.3f} ms / batch (min {lo:.3f} .. max {hi:.3f}, {ks[s]} batches a window); peak memory of "
                f"a pass above its start {peak[s]:9.1f} MiB; mean loss {loss[s]:.6f}; {gs['captures']} captures, {gs['replays']} replays")
        if len(settings) == 2:
            m0, m1 = stats(times[settings[0]])[0], stats(times[settings[1]])[0]
            say(f"  ratio {settings[0]} / {settings[1]}: {m0 / m1:.3f}")
        del runs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
