"""Generate the goldens of ``--vslt-type carryforward`` from the REAL reference.  BUILD CONTAINER ONLY.

    python tests/golden/gen/make_golden_carryforward.py [windows] [step]

``carryforward_windows.npz``: the real ``Multiple_Outbreaks_Training_Dataset.__getitem__`` (builder/data/dataset_new.py:1946-2181,
the branch at :2006-2011) with ``ds.vslt_type = "carryforward"`` on the reference's sample pickles, set up as make_golden_data.py
sets it up (same import plumbing, same min / max rule, same key / length scheme), for ``realtime`` 1 and 0.  The patients and
``feature_mins / feature_maxs`` are those of tie_windows.npz and are not stored again.  Per case: (realtime, patient, key, L),
plane 0 [24, 16] of ``final_seqs``, ``inputLength``, the returned text time, ``static``; once: the ``keep`` vector
(``args.vslt_mask`` as data_preprocess.py:43 derives it from the pickles' ``feature_order``).  All-``None`` windows and windows
with ``L > key + 1`` are skipped: the reference crashes on the former and raises IndexError inside for most of the latter.

``carryforward_step.npz`` + ``state_shapes_carryforward_L2.json``: one train-mode forward + BCE + backward of the real
``TRI_MBT_VSLTCLS`` built with ``vslt_type="carryforward"`` (B 4, two layers, dropout 0, image encoder in eval mode), ``filler``
weights, ``filler.make_batch(seed, 4, 24)`` for everything but ``x``: a seeded, fp16-rounded [4, 24, 16] table with lengths
[24, 1, 7, 13], saved in the file.
"""
import glob
import json
import os
import pickle
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, GOLD)


def gen_windows():
    import ref_shims
    ref_shims.install()
    sys.modules["pickle5"] = pickle
    sys.modules["h5py"] = types.ModuleType("h5py")
    tvt = sys.modules["torchvision.transforms"]
    tvt.functional = types.ModuleType("torchvision.transforms.functional")
    sys.modules["torchvision.transforms.functional"] = tvt.functional
    sys.modules["torchvision"].transforms = tvt
    REF = ref_shims.REF_ROOT
    sys.argv = ["2_train.py", "--input-types", "vslt", "--model", "tri_mbt_vsltcls", "--modality-inclusion",
                "train-missing_test-missing", "--output-type", "intubation", "--batch-size", "4", "--vslt-type", "carryforward",
                "--model-types", "detection", "--multiimages", "0", "--berttype", "biobert", "--txt-tokenization", "bert"]
    os.chdir(REF)
    from control.config import args
    from builder.data import dataset_new as D
    files = sorted(glob.glob(os.path.join(REF, "data/sample_data/train/*.pkl")))
    pk = []
    for f in files:
        with open(f, "rb") as fh:
            pk.append(pickle.load(fh))
    tie = np.load(os.path.join(GOLD, "tie_windows.npz"), allow_pickle=False)
    assert [os.path.basename(f) for f in files] == [str(s) for s in tie["files"]]
    allv = np.concatenate([np.asarray(p["data"], np.float64) for p in pk])
    fmin = allv.min(0)
    fmax = np.maximum(allv.max(0), fmin + 1.0)
    assert np.array_equal(fmin, tie["feature_mins"]) and np.array_equal(fmax, tie["feature_maxs"])
    args.feature_mins, args.feature_maxs = fmin, fmax
    # data_preprocess.py:43: True = remove, over the reference's constant list of the 18 names.  A pickle's feature_order has None
    # where the admission never measured a feature; the one pickle that names all 18 carries the same list and is stored
    from builder.data import data_preprocess as DP
    args.vslt_mask = [True if i not in args.vitalsign_labtest else False for i in DP.VITALSIGN_LABTEST]
    keep = ~np.asarray(args.vslt_mask, bool)
    full = [p["feature_order"] for p in pk if all(n is not None for n in p["feature_order"])]
    order = [str(n) for n in full[0]]
    assert order == [str(n) for n in DP.VITALSIGN_LABTEST]
    assert all(n is None or str(n) == order[j] for p in pk for j, n in enumerate(p["feature_order"]))
    assert int(keep.sum()) == len(args.vitalsign_labtest) == 16

    ds = object.__new__(D.Multiple_Outbreaks_Training_Dataset)
    ds.window_size = args.window_size
    ds.vslt_type = "carryforward"
    ds.vslt_len = len(args.vitalsign_labtest)
    ds.featureidx = np.array(list(range(18)))
    ds.image_size = [args.image_size, args.image_size]
    ds.txt_token_size, ds.token_max_length = 128, 768
    ds.model_types, ds.loss_types = args.model_types, args.loss_types
    ds.neg_multi_target = [0] * 12
    ds.time_data_array = np.zeros([1000, 3])
    cases, rng = [], np.random.RandomState(5)
    for realtime in (1, 0):
        for i, p in enumerate(pk):
            T = len(p["data_in_time"])
            keys = sorted(set([T - 1, max(0, T // 2), min(T - 1, 3)] + [int(rng.randint(0, T))]))
            for key in keys:
                for L in sorted(set([1, min(key + 1, args.window_size), int(rng.randint(1, min(key + 1, args.window_size) + 1))])):
                    win = p["data_in_time"][key - L + 1:key + 1]
                    if all(w is None for w in win) or L > key + 1:
                        continue
                    cases.append((realtime, i, key, L))
    outs = {k: [] for k in ("case", "plane0", "static", "len", "ttime")}
    for realtime, i, key, L in cases:
        args.realtime = realtime
        ds._data_list = [(files[i], [key], {key: [[0]]}, {key: [L]}, 0, [], 0)]
        ds._type_list = [7]
        seq, static, target, n, img, cxr_time, tokens, tlen, ttime, missing, f_idx, taux = ds[0]
        seq = seq.numpy() if torch.is_tensor(seq) else np.asarray(seq)
        assert seq.shape == (3, args.window_size, 16), seq.shape
        outs["case"].append([realtime, i, key, L])
        outs["plane0"].append(seq[0].astype(np.float32))
        outs["static"].append(static.numpy())
        outs["len"].append(int(n))
        outs["ttime"].append(float(ttime))
    np.savez_compressed(os.path.join(GOLD, "carryforward_windows.npz"), case=np.array(outs["case"], np.int64),
                        plane0=np.stack(outs["plane0"]).astype(np.float32), len=np.array(outs["len"], np.int64),
                        static=np.stack(outs["static"]).astype(np.float32), ttime=np.array(outs["ttime"], np.float64),
                        keep=keep, feature_order=np.array(order), wanted=np.array([str(n) for n in args.vitalsign_labtest]))
    print("cases", len(cases), "lens", sorted(set(outs["len"])))


def gen_step():
    import make_golden as MG          # installs the shims, imports filler
    import filler
    args = MG.ref_args(vslt_type="carryforward", batch_size=4, transformer_num_layers=2, output_dim=1)
    assert len(args.vitalsign_labtest) == 16 and args.window_size == 24
    from builder.models import get_model
    model = get_model(args)(args)
    MG.load_filled(model)
    model.train()
    model.img_encoder.eval()
    seed, B, W, F = 6161, 4, 24, 16
    bt = filler.make_batch(seed, B, W)
    lens = torch.tensor([24, 1, 7, 13])
    x = torch.rand(B, W, F, generator=torch.Generator().manual_seed(seed + 1)).half().float()
    x = x * (torch.arange(W).view(1, W, 1) < lens.view(B, 1, 1))
    mnum = bt["missing_num"].clone()
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
    assert all(float(model.get_parameter(n).grad.abs().sum()) > 0 for n in names if n.startswith("vslt_enc."))
    MG.save("carryforward_step", seed=np.array(seed), B=np.array(B), T=np.array(W), x=x, input_lengths=lens, logits=out, loss=loss,
            missing_num=mnum, grad_names=np.array(names), nograd_names=np.array(nograd), grad_digest=np.stack(dig))
    d = {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in model.state_dict().items()}
    with open(os.path.join(GOLD, "state_shapes_carryforward_L2.json"), "w") as f:
        json.dump(d, f, indent=0)


if __name__ == "__main__":
    which = sys.argv[1:] or ["windows", "step"]
    if len(which) > 1:               # control/config.py parses sys.argv once per process: one process per section
        import subprocess
        for w in which:
            subprocess.check_call([sys.executable, os.path.abspath(__file__), w])
    elif which == ["step"]:
        gen_step()
    else:
        gen_windows()
