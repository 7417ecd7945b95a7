"""Generate tests/golden/tri_vmultivslt_step.npz and tri_vmulti2_step.npz (+ state_shapes_tri_vmultivslt_L2.json,
state_shapes_tri_vmulti2_L2.json) from the REAL reference: the classes TRI_MBT_VMULTIVSLT and TRI_MBT_VMULTI2 (both on
TrimodalTransformerEncoder_Multitokens_MBTVSLTMAIN) driven by the reference's own ``missing_trainer``
(builder/trainer/trainer.py:20-241, the ``"multi" in args.model`` branches), once with flow_type="train" and once with "test", on
CPU fp32.  BUILD CONTAINER ONLY, like make_golden.py.

    python tests/golden/gen/make_golden_multitoken.py

What is patched to run that trainer off a GPU (generator's own code; nothing of the reference is copied), as in
make_golden_noshnoavgtr.py:
  * ``Tensor.cuda`` -> identity (trainer.py:77,82,84; the encoder's mask tables, mbt_encoder.py:64-93);
  * ``Tensor.type(torch.HalfTensor)`` -> the same fp16 rounding held as float32.
The gradients are read off ``.grad`` behind a train call with a learning rate of 0 (SGD: the parameters do not move).  The boolean
attention masks are those that each stream's block of the FIRST fusion layer received (a forward pre-hook): [B, N, N], or an empty
array for a stream the encoder leaves unmasked.
"""
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, GOLD)

import ref_shims  # noqa: E402

ref_shims.install()
import filler  # noqa: E402

torch.manual_seed(0)
torch.set_num_threads(8)
warnings.filterwarnings("ignore")


def digest(t: torch.Tensor):
    """L2 norm + 8 strided samples (make_golden.digest)."""
    f = t.detach().reshape(-1).double()
    idx = torch.linspace(0, f.numel() - 1, 8).long()
    return torch.cat([f.norm().view(1), f[idx]]).numpy()


class _Evaluator:
    def __init__(self):
        self.calls = []

    def add_batch(self, target, output):
        self.calls.append((target.detach().clone(), output.detach().clone()))


class _Logger:
    def __init__(self):
        self.evaluator, self.lrs = _Evaluator(), []

    def log_lr(self, lr, it):
        self.lrs.append(lr)


class _Scheduler:
    def step(self, it):
        pass

    def get_lr(self):
        return [0.0]


def one(args, name, tag):
    from builder.models import get_model
    from builder.trainer.trainer import missing_trainer
    args.model = name
    model = get_model(args)(args)
    assert type(model).__name__ == name.upper()
    model.load_state_dict({k: filler.fill_tensor(k, v) for k, v in model.state_dict().items()})
    seed, B, T = 5151, 4, 24
    bt = filler.make_batch(seed, B, T)
    assert bt["missing_num"].tolist() == [0, 1, 2, 3] and bt["txt_lengths"].tolist() == [28, 0, 107, 0]
    assert bt["input_lengths"].tolist() == [24, 4, 9, 5]
    static = torch.stack([bt["gen"], bt["age"]], 1)
    seen, masks = [], {}
    model.register_forward_hook(lambda m, i, o: seen.append((i[11].detach().clone(), o[0].detach().clone(), o[1], o[2])))
    for m_, layer in enumerate(model.fusion_transformer.layer_stacks[0]):
        layer.register_forward_pre_hook(lambda mod, inp, m_=m_: masks.__setitem__(m_, None if inp[1] is None else inp[1].detach().clone()))
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    crit = torch.nn.BCEWithLogitsLoss()

    def run(flow, logger):
        return missing_trainer(args, 1, bt["x"].clone(), static.clone(), bt["input_lengths"].clone(), bt["y"].clone(), model, logger,
                               torch.device("cpu"), scheduler=_Scheduler(), optimizer=opt, criterion=crit, scaler=None, flow_type=flow,
                               output_lengths=None, x_img=bt["img"].clone(), x_txt=bt["txt"].clone(),
                               txt_lengths=bt["txt_lengths"].clone(), imgtxt_time=(bt["img_time"].clone(), bt["txt_time"].clone()),
                               missing=bt["missing"].clone(), reports_tokens=None, reports_lengths=None, criterion_aux=(None, None))[1]

    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.train()
    model.img_encoder.eval()                                                 # no StochasticDepth draws
    train_loss = run("train", _Logger())
    assert all(torch.equal(before[k], v) for k, v in model.state_dict().items())      # lr 0: nothing moved
    mnum, logits, o2, o3 = seen[-1]
    logits = logits.reshape(4, B)
    assert o2 is None and o3 is None and torch.equal(mnum.cpu(), bt["missing_num"])
    train_masks = dict(masks)
    names, nograd, dig = [], [], []
    for n, p_ in model.named_parameters():
        if p_.grad is None:
            nograd.append(n)
        else:
            assert torch.isfinite(p_.grad).all(), n
            names.append(n)
            dig.append(digest(p_.grad))
    model.eval()
    log = _Logger()
    test_loss = run("test", log)
    (tgt, prob), = log.evaluator.calls
    assert tuple(prob.shape) == (B,) and torch.equal(tgt, bt["y"].float())
    assert torch.allclose(seen[-1][1].reshape(4, B), logits, rtol=0, atol=1e-6)      # dropout 0, no batch statistics
    out = dict(seed=np.array(seed), B=np.array(B), T=np.array(T), missing=bt["missing"], missing_num=bt["missing_num"], logits=logits,
               loss=np.array(train_loss), grad_names=np.array(names), nograd_names=np.array(nograd if nograd else [""]),
               grad_digest=np.stack(dig), test_loss=np.array(test_loss), test_prob=prob)
    for m_ in range(3):
        mk = train_masks[m_]
        out[f"mask{m_}"] = np.zeros((0,), dtype=bool) if mk is None else mk.numpy().astype(bool)
        assert masks[m_] is None and mk is None or torch.equal(masks[m_], mk)         # the test call builds the same masks
    out = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    np.savez_compressed(os.path.join(GOLD, f"tri_{tag}_step.npz"), **out)
    print(f"wrote tri_{tag}_step", {k: tuple(v.shape) for k, v in out.items()}, "train", train_loss, "test", test_loss,
          "grads", len(names), "encoder grads", sum(n.startswith("img_encoder.") for n in names), "no grad", len(nograd))
    d = {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in model.state_dict().items()}
    with open(os.path.join(GOLD, f"state_shapes_tri_{tag}_L2.json"), "w") as f:
        json.dump(d, f, indent=0)


def main():
    sys.argv = ["2_train.py", "--input-types", "vslt_img_txt", "--model", "tri_mbt_vmultivslt",
                "--modality-inclusion", "train-missing_test-missing", "--lr-init", "1e-5",
                "--output-type", "intubation", "--batch-size", "4", "--transformer-num-layers", "2",
                "--vslt-type", "TIE", "--model-types", "detection", "--imgtxt-time", "1",
                "--mbt-only-vslt", "1", "--multiimages", "0", "--img-pretrain", "No", "--dropout", "0.0"]
    from control.config import args
    args.device = torch.device("cpu")
    args.output_dim = 1
    args.feature_means = torch.zeros(1)
    assert args.fullmodal_definition == "txt1_img1" and args.input_types == "vslt_img_txt" and args.berttype != "bert"

    torch.Tensor.cuda = lambda self, *a, **k: self
    _type = torch.Tensor.type

    def type_(self, dtype=None, *a, **k):
        if dtype is torch.HalfTensor:
            return self.half().float()
        return _type(self, dtype, *a, **k)
    torch.Tensor.type = type_

    one(args, "tri_mbt_vmultivslt", "vmultivslt")
    one(args, "tri_mbt_vmulti2", "vmulti2")


if __name__ == "__main__":
    main()
