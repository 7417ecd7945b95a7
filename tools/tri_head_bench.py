"""Times of the three-row head on one MI355X: the figures of profiles/tri_head.txt.

    python tools/tri_head_bench.py [--repeats 10] [--iters 300] [--batches 64,256] [--out FILE]

The head section of TRI_MBT_V1 -- ie_demo, LayerNorm of the three CLS rows, fc_list, candidate mean; forward + backward from a fixed
upstream gradient, parameter gradients into the flat gradient buffer as in a training step -- with tuning.HIP_TRI_HEAD on
(ops.TriHeadFn + ops.CandidateMeanFn, csrc/head3.hip) and off (the torch chain), bf16 CLS rows of [B, N_m, 256] stream outputs.
Both variants in ONE process, alternating, ``--repeats`` windows of ``--iters`` sections each, every shape warmed first:
  eager    ms per section by the host clock around a window that ends in a device synchronise (launch-bound: what --hip-graph 0 pays)
  replayed ms per section by device events around replays of the section captured with torch.cuda.graph (what --hip-graph 1 pays)
Then the masked mean BCE (ops.BceMaskedMean, forward + backward) against the reference's boolean-index form, eager (the boolean
index synchronises the host and cannot be captured).  Reported: median and min .. max over the windows.  Needs a GPU; no fallback."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools._timing import Lines, device_ms, median, wall_ms  # noqa: E402

N_TOKENS = (8, 8, 8)               # rows per stream output: the CLS rows are strided views, as in the model, of SHORT stand-in outputs --
#                                    the zero-filled [B, N, 256] gradient autograd builds around d cls is the stack's business, not the head's


def fmt(xs):
    return f"{1e3 * median(xs):8.1f} us  ({1e3 * min(xs):.1f} .. {1e3 * max(xs):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tri_head_bench: needs an MI355X (no CPU fallback)")
    from medical_tri_modal_pilot_amd import ops, tuning
    from medical_tri_modal_pilot_amd.builder.models import get_model
    from medical_tri_modal_pilot_amd.control.config import parse_args
    from medical_tri_modal_pilot_amd.optim import FlatParams
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    say = Lines()
    say(f"three-row head on {torch.cuda.get_device_name(0)}: {a.repeats} alternating windows of {a.iters} sections per variant, bf16 CLS rows")
    args = parse_args(["--input-types", "vslt_img_txt", "--model", "tri_mbt_v1", "--modality-inclusion", "train-missing_test-missing",
                       "--batch-size", "64", "--transformer-num-layers", "1", "--imgtxt-time", "1", "--compute-dtype", "bf16"])
    args.device, args.output_dim = dev, 1
    torch.manual_seed(7)
    model = get_model(args)(args).to(dev).train()
    head = [(n, p) for n, p in model.named_parameters() if n.startswith(("ie_demo.", "layer_norms_after_concat.", "fc_list."))]
    flat = FlatParams(head)
    crit = torch.nn.BCEWithLogitsLoss()
    for B in [int(b) for b in a.batches.split(",")]:
        g = torch.Generator().manual_seed(B)
        outs = [torch.randn(B, n, 256, generator=g).to(dev, torch.bfloat16).requires_grad_() for n in N_TOKENS]
        age, gen = torch.rand(B, generator=g).to(dev), torch.randint(0, 2, (B,), generator=g).float().to(dev)
        mnum = torch.randint(0, 4, (B,), generator=g).to(dev)
        up = torch.randn(B, generator=g).to(dev)
        y = torch.randint(0, 2, (B,), generator=g).float().to(dev)

        def section(on):
            tuning.HIP_TRI_HEAD = on
            flat.written.clear()
            flat.accumulated.clear()
            for t in outs:
                t.grad = None
            demo = None if on else model.ie_demo(torch.stack([age, gen], dim=1))
            out, _, _ = model._head(outs, demo, age, gen, mnum, on)
            out.backward(up)
            return out

        checks = {}
        for on in (True, False):
            flat.grad.zero_()
            checks[on] = (section(on).detach().clone(), flat.grad.clone(), [t.grad.float().clone() for t in outs])
        rel = lambda x, r: float((x - r).abs().max() / (r.abs().max() + 1e-30))
        say(f"B {B}: on vs off: logits {rel(checks[True][0], checks[False][0]):.1e}, parameter gradients "
            f"{rel(checks[True][1], checks[False][1]):.1e}, d cls {max(rel(x, r) for x, r in zip(checks[True][2], checks[False][2])):.1e}")
        graphs = {}
        for on in (True, False):
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    section(on)
            torch.cuda.current_stream().wait_stream(side)
            graphs[on] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[on]):
                section(on)
        eager, replay = {True: [], False: []}, {True: [], False: []}
        for _ in range(a.repeats):
            for on in (True, False):
                eager[on].append(wall_ms(lambda: [section(on) for _ in range(a.iters)]) / a.iters)
            for on in (True, False):
                replay[on].append(device_ms(graphs[on].replay, a.iters))
        for name, d in (("eager", eager), ("replayed", replay)):
            say(f"B {B} head section {name:8s}: HIP_TRI_HEAD on  {fmt(d[True])}")
            say(f"B {B} head section {name:8s}: HIP_TRI_HEAD off {fmt(d[False])}")
        tuning.HIP_TRI_HEAD = True
        # masked mean BCE, forward + backward, on logits [3, B]
        o = torch.randn(3, B, generator=g).to(dev).requires_grad_()

        def masked():
            loss = ops.BceMaskedMean.apply(o, y, mnum)
            return torch.autograd.grad(loss, o, ops.unit_grad(loss))

        def indexed():
            mask = ops._present_rows(mnum)
            loss = crit(o[mask], y.reshape(1, -1).expand(3, -1)[mask])
            return torch.autograd.grad(loss, o)
        for _ in range(5):
            masked(), indexed()
        tm, ti = [], []
        for _ in range(a.repeats):
            tm.append(wall_ms(lambda: [masked() for _ in range(a.iters)]) / a.iters)
            ti.append(wall_ms(lambda: [indexed() for _ in range(a.iters)]) / a.iters)
        say(f"B {B} masked BCE eager   : ops.BceMaskedMean  {fmt(tm)}")
        say(f"B {B} masked BCE eager   : boolean index      {fmt(ti)}")
    say.write(a.out)


if __name__ == "__main__":
    main()
