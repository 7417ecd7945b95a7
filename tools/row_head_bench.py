"""Times of the R-row head on one MI355X: the figures of profiles/row_head.txt.

    python tools/row_head_bench.py [--repeats 10] [--iters 300] [--batches 64,256] [--models a,b] [--out FILE]

The head section of tri_mbt_vflexible, bitxt_mbt_vflexible1, tri_mbt_vmultivslt and tri_mbt_vmulti2 -- ie_demo, LayerNorm of the head
rows (for tri_mbt_vmulti2: of the source means), the fc heads, for the flexible models the softmax weighting; forward + backward
from a fixed upstream gradient, parameter gradients into the flat gradient buffer as in a training step -- with tuning.HIP_ROW_HEAD
on (ops.RowHeadFn / ops.TriHeadFn + ops.FlexCombineFn, csrc/headr.hip) and off (the torch chain), bf16 rows of [B, N, 256] stream
outputs.  The method is tools/tri_head_bench.py's: both variants in ONE process, alternating, ``--repeats`` windows of ``--iters``
sections each, every shape warmed first:
  eager    ms per section by the host clock around a window that ends in a device synchronise (what --hip-graph 0 pays)
  replayed ms per section by device events around replays of the section captured with torch.cuda.graph (what --hip-graph 1 pays)
Reported: median and min .. max over the windows.  Needs a GPU; no fallback."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools._timing import Lines, device_ms, median, wall_ms  # noqa: E402

N_TOKENS = 8                       # rows per stand-in stream output (tools/tri_head_bench.py says why they are short)
MODELS = {"tri_mbt_vflexible": "vslt_img_txt", "bitxt_mbt_vflexible1": "vslt_txt", "tri_mbt_vmultivslt": "vslt_img_txt",
          "tri_mbt_vmulti2": "vslt_img_txt"}
HEAD_PREFIXES = ("ie_demo.", "layer_norms_after_concat.", "fc_list.", "fc_lists.", "flexibleavg")


def fmt(xs):
    return f"{1e3 * median(xs):8.1f} us  ({1e3 * min(xs):.1f} .. {1e3 * max(xs):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("row_head_bench: needs an MI355X (no CPU fallback)")
    from medical_tri_modal_pilot_amd import tuning
    from medical_tri_modal_pilot_amd.builder.models import get_model
    from medical_tri_modal_pilot_amd.control.config import parse_args
    from medical_tri_modal_pilot_amd.optim import FlatParams
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    say = Lines()
    say(f"R-row head on {torch.cuda.get_device_name(0)}: {a.repeats} alternating windows of {a.iters} sections per variant, bf16 rows")
    for name in a.models.split(","):
        args = parse_args(["--input-types", MODELS[name], "--model", name, "--modality-inclusion", "train-missing_test-missing",
                           "--batch-size", "64", "--transformer-num-layers", "1", "--imgtxt-time", "1", "--compute-dtype", "bf16"])
        args.device, args.output_dim = dev, 1
        torch.manual_seed(7)
        model = get_model(args)(args).to(dev).train()
        # the flexible models' torch chain copies its mask table from the host on every call, which a capture refuses: for the
        # replayed comparison the table is put on the device beforehand (the copy then is no launch at all -- in the chain's favour)
        for cls in type(model).__mro__:
            mod = sys.modules.get(cls.__module__)
            if hasattr(mod, "_ABSENT"):
                mod._ABSENT = mod._ABSENT.to(dev)
        bi = name.startswith("bi")
        flat = FlatParams([(n, p) for n, p in model.named_parameters() if n.startswith(HEAD_PREFIXES) and not n.startswith("rmse")])
        rows_out = 4 if "multi" in name else 0
        for B in [int(b) for b in a.batches.split(",")]:
            g = torch.Generator().manual_seed(B)
            outs = [torch.randn(B, N_TOKENS, 256, generator=g).to(dev, torch.bfloat16).requires_grad_() for _ in range(2 if bi else 3)]
            age, gen = torch.rand(B, generator=g).to(dev), torch.randint(0, 2, (B,), generator=g).float().to(dev)
            mnum = torch.randint(0, 2 if bi else 4, (B,), generator=g).to(dev)
            up = (torch.randn(rows_out, B, generator=g) if rows_out else torch.randn(B, 1, generator=g)).to(dev)

            def section(on):
                tuning.HIP_ROW_HEAD = on
                flat.written.clear()
                flat.accumulated.clear()
                for t in outs:
                    t.grad = None
                if bi:
                    out = model._head(outs, age, gen, mnum, B)[0]
                else:
                    demo = None if on else model.ie_demo(torch.stack([age, gen], dim=1))
                    out = model._head(outs, demo, age, gen, mnum, on)[0]
                out.backward(up)
                return out

            checks = {}
            for on in (True, False):
                flat.grad.zero_()
                # (a stream output no head row reads -- tri_mbt_vmultivslt's image and text streams -- has no gradient)
                checks[on] = (section(on).detach().clone(), flat.grad.clone(), [t.grad.float().clone() for t in outs if t.grad is not None])
            rel = lambda x, r: float((x - r).abs().max() / (r.abs().max() + 1e-30))
            say(f"{name} B {B}: on vs off: logits {rel(checks[True][0], checks[False][0]):.1e}, parameter gradients "
                f"{rel(checks[True][1], checks[False][1]):.1e}, d rows {max(rel(x, r) for x, r in zip(checks[True][2], checks[False][2])):.1e}")
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
            for kind, d in (("eager", eager), ("replayed", replay)):
                say(f"{name} B {B} head section {kind:8s}: HIP_ROW_HEAD on  {fmt(d[True])}")
                say(f"{name} B {B} head section {kind:8s}: HIP_ROW_HEAD off {fmt(d[False])}")
            tuning.HIP_ROW_HEAD = True
        del model, flat
    say.write(a.out)


if __name__ == "__main__":
    main()
