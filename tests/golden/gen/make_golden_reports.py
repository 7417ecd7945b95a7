"""Generate tests/golden/report_cases.npz by calling the REAL reference
``Multiple_Outbreaks_Training_Dataset.__getitem__`` (builder/data/dataset_new.py:1946-2181, the text branch :2135-2155) on the
reference's own data/sample_data pickles.  BUILD CONTAINER ONLY.

    python tests/golden/gen/make_golden_reports.py

The dataset object is made as in make_golden_data.py (``object.__new__``, one pinned window per file, ``_type_list = [7]`` so the
image branch returns its zeros without opening a file).  ``ds.bioemb`` is a plain dict ``{text: {'embedding': array}}`` in place of
the BioBERT h5 file: the seven files whose name says ``txt1`` get reports of the lengths of tests/report_store_model.GOLDEN_LENGTHS
with closed-form embeddings keyed by the FILE INDEX (``golden_embedding``) -- no report text is stored, a report is named by the
index of its file.  Every file is read under ``missing_comb`` 0..3: 40 cases.

Stored per case: file index, missing_comb, textLength, the ``missing`` vector and the SHA-256 of the returned float32 [128, 768]
bytes; per file whether its name carries ``txt1``; per report its file index and length.
"""
import glob
import hashlib
import os
import pickle
import sys
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
sys.modules["torchvision.transforms.functional"] = tvt.functional
sys.modules["torchvision"].transforms = tvt

REF = ref_shims.REF_ROOT


def main():
    from tests import report_store_model as M
    sys.argv = ["2_train.py", "--input-types", "vslt_img_txt", "--model", "tri_mbt_vsltcls", "--modality-inclusion",
                "train-missing_test-missing", "--output-type", "intubation", "--batch-size", "4", "--vslt-type", "TIE",
                "--model-types", "detection", "--multiimages", "0", "--berttype", "biobert", "--txt-tokenization", "bert"]
    os.chdir(REF)                      # control/config.py and builder/utils read relative paths
    from control.config import args
    from builder.data import dataset_new as D
    assert {k: getattr(args, k) for k in M.GOLDEN_FLAGS} == M.GOLDEN_FLAGS
    files = sorted(glob.glob(os.path.join(REF, "data/sample_data/train/*.pkl")))
    pk = []
    for f in files:
        with open(f, "rb") as fh:
            pk.append(pickle.load(fh))
    allv = np.concatenate([np.asarray(p["data"], np.float64) for p in pk])
    args.feature_mins = allv.min(0)
    args.feature_maxs = np.maximum(allv.max(0), args.feature_mins + 1.0)
    args.realtime, args.TIE_len = 1, 1000

    txt1 = ["txt1" in os.path.basename(f) for f in files]
    report_file = [i for i, t in enumerate(txt1) if t]
    assert len(report_file) == len(M.GOLDEN_LENGTHS)
    bioemb = {}
    for i, n in zip(report_file, M.GOLDEN_LENGTHS):
        text = pk[i]["txt_input"][0].strip()
        assert len(text) != 0 and text not in bioemb
        bioemb[text] = {"embedding": M.golden_embedding(i, n)}

    ds = object.__new__(D.Multiple_Outbreaks_Training_Dataset)
    ds.window_size = args.window_size
    ds.vslt_type = "TIE"
    ds.featureidx = np.array(list(range(18)))
    ds.image_size = [args.image_size, args.image_size]
    ds.txt_token_size, ds.token_max_length = 128, 768
    ds.model_types, ds.loss_types = args.model_types, args.loss_types
    ds.neg_multi_target = [0] * 12
    ds.time_data_array = np.zeros([args.TIE_len, 3])
    ds.bioemb = bioemb
    out = {k: [] for k in ("case_file", "case_comb", "text_length", "missing", "sha256")}
    for i, p in enumerate(pk):
        key = max(k for k, a in enumerate(p["data_in_time"]) if a is not None)       # a one-hour window on a present hour
        for comb in (0, 1, 2, 3):
            ds._data_list = [(files[i], [key], {key: [[0]]}, {key: [1]}, 0, [], comb)]
            ds._type_list = [7]
            seq, static, target, n, img, cxr_time, tokens, tlen, ttime, missing, f_idx, taux = ds[0]
            assert float(img.abs().sum()) == 0 and tokens.dtype.is_floating_point and tuple(tokens.shape) == (128, 768)
            out["case_file"].append(i)
            out["case_comb"].append(comb)
            out["text_length"].append(int(tlen))
            out["missing"].append(np.asarray(missing.numpy(), np.float32))
            out["sha256"].append(hashlib.sha256(tokens.float().contiguous().numpy().tobytes()).hexdigest())
    store = dict(file_txt1=np.asarray(txt1, np.int64), report_file=np.asarray(report_file, np.int64),
                 report_len=np.asarray(M.GOLDEN_LENGTHS, np.int64), case_file=np.asarray(out["case_file"], np.int64),
                 case_comb=np.asarray(out["case_comb"], np.int64), text_length=np.asarray(out["text_length"], np.int64),
                 missing=np.stack(out["missing"]), sha256=np.asarray(out["sha256"]))
    np.savez_compressed(os.path.join(GOLD, "report_cases.npz"), **store)
    print("cases", len(out["case_file"]), "text lengths", sorted(set(out["text_length"])), "missing[2] set in",
          int(store["missing"][:, 2].sum()))


if __name__ == "__main__":
    main()
