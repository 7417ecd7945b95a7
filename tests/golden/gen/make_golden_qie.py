"""Generate the goldens of ``--vslt-type QIE`` from the REAL reference.  BUILD CONTAINER ONLY.

    python tests/golden/gen/make_golden_qie.py

``qie_step.npz`` + ``state_shapes_qie_L2.json`` (``--imgtxt-time 1``) and ``qie_step_notime.npz`` (``--imgtxt-time 0``): one
train-mode forward + BCE + backward of the real ``TRI_MBT_VSLTCLS`` built with ``vslt_type="QIE"`` (B 4 -- all four ``missing_num``
patterns --, two layers, dropout 0, image encoder in eval mode), ``filler`` weights, ``filler.make_batch(seed, 4, 24)`` for
everything but ``x``: seeded, fp16-rounded TIE events [4, 24, 3] with lengths [24, 1, 7, 13] and zero rows behind them, saved in
the file.  Stored: logits, loss, a digest of every parameter's gradient, the names without a gradient.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, GOLD)


def qie_events(seed, B, T, lens):
    """TIE events (time, value, feature) as synthetic.make_batch draws them, with the given lengths"""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(B, T, 3)
    for b in range(B):
        n = int(lens[b])
        x[b, :n, 0] = torch.sort(-24.0 * torch.rand(n, generator=g))[0]
        x[b, :n, 1] = torch.rand(n, generator=g)
        x[b, :n, 2] = torch.randint(0, 18, (n,), generator=g).float()
    return x.half().float()


def gen_step(imgtxt_time, tag, shapes):
    import make_golden as MG          # installs the shims, imports filler
    import filler
    args = MG.ref_args(vslt_type="QIE", batch_size=4, transformer_num_layers=2, output_dim=1, imgtxt_time=imgtxt_time)
    from builder.models import get_model
    model = get_model(args)(args)
    MG.load_filled(model)
    model.train()
    model.img_encoder.eval()
    assert tuple(model.fc_list[0].weight.shape) == (256, 256)
    seed, B, T = 7171, 4, 24
    bt = filler.make_batch(seed, B, T)
    lens = torch.tensor([24, 1, 7, 13])
    x = qie_events(seed + 1, B, T, lens)
    mnum = bt["missing_num"].clone()
    assert sorted(mnum.tolist()) == [0, 1, 2, 3]
    out, o2, o3 = model(x, None, None, None, None, bt["age"], bt["gen"], lens.clone(), bt["txt"], bt["txt_lengths"].clone(),
                        bt["img"], mnum, None, bt["img_time"].half().float(), bt["txt_time"].half().float(), "train", None, None)
    assert o2 is None and o3 is None
    loss = torch.nn.BCEWithLogitsLoss()(out.squeeze(), bt["y"].float())
    loss.backward()
    names, nograd, dig = [], [], []
    for n, p_ in model.named_parameters():
        if p_.grad is None:
            nograd.append(n)
        else:
            names.append(n)
            dig.append(MG.digest(p_.grad))
    assert all(float(model.get_parameter(n).grad.abs().sum()) > 0 for n in names if n.startswith("ie_demo."))
    assert sum(n.startswith("ie_demo.") for n in names) == 4
    MG.save(tag, seed=np.array(seed), B=np.array(B), T=np.array(T), x=x, input_lengths=lens, logits=out, loss=loss,
            missing_num=mnum, imgtxt_time=np.array(imgtxt_time), grad_names=np.array(names), nograd_names=np.array(nograd),
            grad_digest=np.stack(dig))
    if shapes:
        d = {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in model.state_dict().items()}
        with open(os.path.join(GOLD, "state_shapes_qie_L2.json"), "w") as f:
            json.dump(d, f, indent=0)
    MG.ref_args()                     # leave the global args as the other generators expect


if __name__ == "__main__":
    gen_step(1, "qie_step", True)
    gen_step(0, "qie_step_notime", False)
