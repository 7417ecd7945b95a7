"""Generate tests/golden/tri_v2_512_step.npz: one train-mode forward + BCE + backward of the REAL TRI_MBT_V2 class at
--image-size 512 on CPU fp32 (the encoder is trained there, tri_mbt_v2.py:208-211; at 512 pixels its four stages work on maps of
128 / 64 / 32 / 16 tokens a side -- zero-padded windows at every stage, swin_transformer.py:150-152 -- and the fusion stack sees
256 image tokens).  BUILD CONTAINER ONLY, like make_golden.py, whose helpers it uses.

    python tests/golden/gen/make_golden_512.py

Follows make_golden._sibling_step (dropout 0, image encoder in eval mode but trained, token-id reports, mixed missing
modalities); stores seeds, token ids, logits, loss, gradient names and digests only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (installs the reference shims)

filler = mg.filler


def gen_tri_v2_512():
    args = mg.ref_args(input_types="vslt_img_txt", model="tri_mbt_v2", batch_size=4, transformer_num_layers=2, output_dim=1,
                       berttype="bert", image_size=512)
    from builder.models import get_model
    model = get_model(args)(args)
    mg.load_filled(model)
    model.train()
    model.img_encoder.eval()
    seed, B, T = 5151, 4, 24
    bt = filler.make_batch(seed, B, T, img_size=512)
    mnum = bt["missing_num"].clone()
    tmax = int(bt["input_lengths"].max())
    # token-id reports (tri_mbt_v2.py:205): seeded ids, zeros behind each report's length -- as make_golden._sibling_step
    tokens = torch.randint(1, 30000, (B, 128), generator=torch.Generator().manual_seed(seed + 1))
    tokens[torch.arange(128).unsqueeze(0) >= bt["txt_lengths"].unsqueeze(1)] = 0
    out, o2, o3 = model(bt["x"][:, :tmax], None, None, None, None, bt["age"], bt["gen"], bt["input_lengths"].clone(),
                        tokens.float(), bt["txt_lengths"].clone(), bt["img"], mnum, None, bt["img_time"].half().float(),
                        bt["txt_time"].half().float(), "train", None, None)
    assert o2 is None and o3 is None
    loss = torch.nn.BCEWithLogitsLoss()(out.squeeze(-1), bt["y"].float())
    loss.backward()
    names, nograd, dig = [], [], []
    for n, p_ in model.named_parameters():
        if p_.grad is None:
            nograd.append(n)
        else:
            names.append(n)
            dig.append(mg.digest(p_.grad))
    print("loss", float(loss.detach()), "tensors with a gradient", len(names))
    mg.save("tri_v2_512_step", seed=np.array(seed), B=np.array(B), T=np.array(T), image_size=np.array(512), logits=out, loss=loss,
            missing_num=mnum, grad_names=np.array(names), nograd_names=np.array(nograd), grad_digest=np.stack(dig), tokens=tokens)
    mg.ref_args(input_types="vslt_img_txt", model="tri_mbt_vsltcls", berttype="biobert", image_size=224)


if __name__ == "__main__":
    mg.ref_args()
    gen_tri_v2_512()
