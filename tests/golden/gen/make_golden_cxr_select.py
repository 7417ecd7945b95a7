"""Generate tests/golden/cxr_select_cases.npz by calling the REAL reference
``Multiple_Outbreaks_Training_Dataset.__getitem__`` (builder/data/dataset_new.py:1946-2181, the image branch :2069-2133) on the
reference's own data/sample_data pickles.  BUILD CONTAINER ONLY (needs PIL: it writes the image files).

    python tests/golden/gen/make_golden_cxr_select.py

The dataset object is made as in make_golden_reports.py (``object.__new__``, one pinned window per case).  Six of the sample
patients carry ``cxr_input`` lists of 1 to 6 ``(time, path)`` pairs, some at negative times.  ``image_data_path`` points at a
temporary directory that holds, at every such path, a 1 x 1 JPEG whose grey value is the INDEX of the file (patients in file
order, a patient's images in list order); ``F_t.equalize`` is the identity and ``ds.transform`` returns that grey value as a
[1, 1, 1] tensor, so the returned image tensor names the chosen files and their order.  An absent slot is told from file 0 by its
time (10, which no chosen image can have: a chosen image's time is <= selected_key).  ``min_time`` (realtime 0) is observed
through a module-level ``min`` that records its result; no line of the reference is held here.

Cases: --multiimages 0 / 1, missing_comb 0..3, ``_type_list`` 0, 2, 5 (images read) and 1, 7 (not), realtime 1 / 0, per patient
keys at its first present hour, around each image time and at its last present hour (the eligible set is empty, 1-2 images, more
than three), one window that ends in absent hours (``late_nones`` moves selected_key), and train-full cases where an image is
eligible (the reference exits the process otherwise).

Stored: per file its patient, time and the rank of its path among all paths (``sorted()`` breaks time ties by path); per case
the patient, flags, selected_key AFTER the late_nones correction, t0, the chosen file indices (-1: absent), ``cxr_time`` as
float32 and the ``missing`` vector.
"""
import glob
import io
import os
import pickle
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)
ROOT = os.path.dirname(os.path.dirname(GOLD))
sys.path.insert(0, HERE)
sys.path.insert(0, GOLD)
sys.path.insert(0, ROOT)
import ref_shims  # noqa: E402

ref_shims.install()
sys.modules["pickle5"] = pickle
sys.modules["h5py"] = types.ModuleType("h5py")
tvt = sys.modules["torchvision.transforms"]
tvt.functional = types.ModuleType("torchvision.transforms.functional")
tvt.functional.equalize = lambda image: image
sys.modules["torchvision.transforms.functional"] = tvt.functional
sys.modules["torchvision"].transforms = tvt

REF = ref_shims.REF_ROOT


def main():
    import torch
    from PIL import Image
    sys.argv = ["2_train.py", "--input-types", "vslt_img_txt", "--model", "tri_mbt_vsltcls", "--modality-inclusion",
                "train-missing_test-missing", "--output-type", "intubation", "--batch-size", "4", "--vslt-type", "TIE",
                "--model-types", "detection", "--multiimages", "0", "--berttype", "biobert", "--txt-tokenization", "bert"]
    os.chdir(REF)
    from control.config import args
    from builder.data import dataset_new as D
    files = sorted(glob.glob(os.path.join(REF, "data/sample_data/train/*.pkl")))
    pk = []
    for f in files:
        with open(f, "rb") as fh:
            pk.append(pickle.load(fh))
    allv = np.concatenate([np.asarray(p["data"], np.float64) for p in pk])
    args.feature_mins = allv.min(0)
    args.feature_maxs = np.maximum(allv.max(0), args.feature_mins + 1.0)
    args.TIE_len = 1000

    tmp = tempfile.mkdtemp(prefix="cxr_select_") + "/"
    f_pat, f_time, paths = [], [], []
    for i, p in enumerate(pk):
        for t, path in (p.get("cxr_input") or []):
            g = len(paths)
            assert g < 256
            os.makedirs(os.path.dirname(tmp + path), exist_ok=True)
            Image.fromarray(np.full((1, 1), g, np.uint8)).save(tmp + path, format="JPEG", quality=100)
            assert np.asarray(Image.open(tmp + path)).tolist() == [[g]]
            f_pat.append(i)
            f_time.append(float(t))
            paths.append(path)
    rank = np.argsort(np.argsort(np.array(paths)))

    seen = []
    D.min = lambda *a, **k: (seen.append(min(*a, **k)), seen[-1])[1]          # records min_time (dataset_new.py:2023)

    ds = object.__new__(D.Multiple_Outbreaks_Training_Dataset)
    ds.window_size = args.window_size
    ds.vslt_type = "TIE"
    ds.featureidx = np.array(list(range(18)))
    ds.image_size = [1, 1]
    ds.image_data_path = tmp
    ds.transform = lambda image: torch.tensor(float(np.asarray(image)[0, 0])).reshape(1, 1, 1)
    ds.txt_token_size, ds.token_max_length = 128, 768
    ds.model_types, ds.loss_types = args.model_types, args.loss_types
    ds.neg_multi_target = [0] * 12
    ds.time_data_array = np.zeros([args.TIE_len, 3])
    ds.bioemb = {p["txt_input"][0].strip(): {"embedding": np.zeros((1, 768), np.float32)} for p in pk
                 if p.get("txt_input") and len(p["txt_input"][0].strip())}

    out = {k: [] for k in ("patient", "multi", "comb", "type_id", "realtime", "train_full", "selected_key", "t0", "chosen",
                           "cxr_time", "missing")}

    def run(i, key, length, multi, comb, type_id, realtime, full):
        p = pk[i]
        args.multiimages, args.realtime = multi, realtime
        args.modality_inclusion = "train-full_test-full" if full else "train-missing_test-missing"
        window = p["data_in_time"][key - length + 1:key + 1]
        late = 0
        while window[-1 - late] is None:
            late += 1
        sel = key if full else key - late
        ds._data_list = [(files[i], [key], {key: [[0]]}, {key: [length]}, 0, [], comb)]
        ds._type_list = [type_id]
        del seen[:]
        seq, static, target, n, img, cxr_time, tokens, tlen, ttime, missing, f_idx, taux = ds[0]
        t0 = float(seen[-1]) if realtime == 0 else float(sel)
        ct = np.asarray(torch.as_tensor(cxr_time, dtype=torch.float64).reshape(-1).numpy(), np.float64)
        vals = np.asarray(img.reshape(-1).numpy(), np.float64)
        assert vals.size == ct.size == (3 if multi else 1)
        absent = (ct == 10) if multi else np.array([bool(missing[1])])
        chosen = np.where(absent, -1, np.round(vals)).astype(np.int64)
        assert (vals[absent] == 0).all()
        out["patient"].append(i)
        for k, v in (("multi", multi), ("comb", comb), ("type_id", type_id), ("realtime", realtime), ("train_full", int(full))):
            out[k].append(v)
        out["selected_key"].append(sel)
        out["t0"].append(t0)
        out["chosen"].append(np.concatenate([chosen, -np.ones(3 - chosen.size, np.int64)]))
        out["cxr_time"].append(np.concatenate([ct, np.full(3 - ct.size, np.nan)]).astype(np.float32))
        out["missing"].append(np.asarray(missing.numpy(), np.float32))

    for i, p in enumerate(pk):
        present = [k for k, a in enumerate(p["data_in_time"]) if a is not None]
        times = [t for t, _ in (p.get("cxr_input") or [])]
        keys = {present[0], present[-1]}
        for t in times:                                  # the present hours just below and just above every image time
            keys |= {max([k for k in present if k < t], default=present[0]), min([k for k in present if k >= t], default=present[-1])}
        for key in sorted(keys):
            for multi in (0, 1):
                for comb in (0, 1, 2, 3):
                    run(i, key, 1, multi, comb, 0, 1, False)
                for type_id in (2, 5, 1, 7):
                    run(i, key, 1, multi, 0, type_id, 1, False)
                run(i, key, 1, multi, 0, 3, 0, False)    # realtime 0: the single image's time is taken from min_time
                if any(t <= key for t in times):
                    run(i, key, 1, multi, 0, 7, 1, True)  # train-full ignores the type; an image is eligible
        gaps = [k for k in range(2, len(p["data_in_time"])) if p["data_in_time"][k] is None and p["data_in_time"][k - 1] is None
                and p["data_in_time"][k - 2] is not None]
        for key in gaps[:1]:                             # a three-hour window whose last two hours are absent
            for multi in (0, 1):
                run(i, key, 3, multi, 0, 0, 1, False)
                run(i, key, 3, multi, 0, 0, 0, False)

    store = dict(file_patient=np.asarray(f_pat, np.int64), file_time=np.asarray(f_time, np.float64), file_rank=rank.astype(np.int64),
                 n_patients=np.asarray(len(pk), np.int64),
                 input_types=np.asarray(args.input_types), fullmodal_definition=np.asarray(args.fullmodal_definition),
                 **{k: np.asarray(v) if k not in ("chosen", "cxr_time", "missing") else np.stack(v) for k, v in out.items()})
    np.savez_compressed(os.path.join(GOLD, "cxr_select_cases.npz"), **store)
    n_el = (store["chosen"] >= 0).sum(1)
    print("files", len(paths), "cases", len(out["patient"]), "chosen per case", np.bincount(n_el).tolist(), "moved keys",
          int(sum(1 for a, b in zip(out["selected_key"], out["t0"]) if a != b)))


if __name__ == "__main__":
    main()
