"""Generate tests/golden/token_report_cases.npz by calling the REAL reference
``Multiple_Outbreaks_Training_Dataset.__getitem__`` (builder/data/dataset_new.py:1946-2181, the token-id text branch :2157-2175
with ``clinical_note_transform`` :186-192) on the reference's own data/sample_data pickles, with ``--berttype bert
--txt-tokenization bert``.  BUILD CONTAINER ONLY.

    python tests/golden/gen/make_golden_token_reports.py

The dataset object is made as in make_golden_reports.py (``object.__new__``, one pinned window per file, ``_type_list = [7]`` so
the image branch returns its zeros without opening a file).  ``ds.txtDict`` is a plain dict ``{(pat_id, chid): list of ints}``: the
seven files whose name says ``txt1`` get id lists of the lengths of tests/token_store_model.GOLDEN_LENGTHS in closed form
(``golden_ids``, keyed by the FILE INDEX; the values 0, 1, 2, 3 and 29999 among them) -- no token text is stored.  The reference
MUTATES the list it reads (``tokens.insert(0, 2)``, the short branch's ``tokens.append(3)``), so the same report grows on every
read: every case gets a FRESH dictionary, the goldens are first reads.  The three ``txt0`` files are never looked up.  Every file
is read under ``missing_comb`` 0..3: 40 cases.

Stored per case: file index, missing_comb, textLength, the ``missing`` vector and the SHA-256 of the returned float32 [128]
bytes; per file whether its name carries ``txt1``; per report its file index and length.
"""
import glob
import hashlib
import os
import pickle
import sys
import types

import numpy as np
import torch

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
    from tests import token_store_model as M
    sys.argv = ["2_train.py", "--input-types", "vslt_img_txt", "--model", "tri_mbt_vsltcls", "--modality-inclusion",
                "train-missing_test-missing", "--output-type", "intubation", "--batch-size", "4", "--vslt-type", "TIE",
                "--model-types", "detection", "--multiimages", "0", "--berttype", "bert", "--txt-tokenization", "bert"]
    os.chdir(REF)                      # control/config.py and builder/utils read relative paths
    from control.config import args
    from builder.data import dataset_new as D
    assert {k: getattr(args, k) for k in M.GOLDEN_FLAGS} == M.GOLDEN_FLAGS
    assert args.bert_token_max_length == M.L and args.berttype == "bert" and args.txt_tokenization == "bert"
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
    keys = [(int(p["pat_id"]), int(p["chid"])) for p in pk]
    assert len({keys[i] for i in report_file}) == len(report_file)

    def fresh_dict():
        return {keys[i]: M.golden_ids(i, n) for i, n in zip(report_file, M.GOLDEN_LENGTHS)}
    assert {v for ids in fresh_dict().values() for v in ids} >= set(M.SPECIAL)

    ds = object.__new__(D.Multiple_Outbreaks_Training_Dataset)
    ds.window_size = args.window_size
    ds.vslt_type = "TIE"
    ds.featureidx = np.array(list(range(18)))
    ds.image_size = [args.image_size, args.image_size]
    ds.token_max_length = M.L
    ds.model_types, ds.loss_types = args.model_types, args.loss_types
    ds.neg_multi_target = [0] * 12
    ds.time_data_array = np.zeros([args.TIE_len, 3])
    out = {k: [] for k in ("case_file", "case_comb", "text_length", "missing", "sha256")}
    for i, p in enumerate(pk):
        key = max(k for k, a in enumerate(p["data_in_time"]) if a is not None)       # a one-hour window on a present hour
        for comb in (0, 1, 2, 3):
            ds._data_list = [(files[i], [key], {key: [[0]]}, {key: [1]}, 0, [], comb)]
            ds._type_list = [7]
            ds.txtDict = fresh_dict()
            seq, static, target, n, img, cxr_time, tokens, tlen, ttime, missing, f_idx, taux = ds[0]
            assert float(img.abs().sum()) == 0 and tokens.dtype == torch.float32 and tuple(tokens.shape) == (M.L,)
            want = M.reference_ids(M.golden_ids(i, dict(zip(report_file, M.GOLDEN_LENGTHS))[i]) if (txt1[i] and comb in (0, 2)) else [])
            assert torch.equal(tokens, want), (i, comb)          # the restated rule equals the reference on every case
            out["case_file"].append(i)
            out["case_comb"].append(comb)
            out["text_length"].append(int(tlen))
            out["missing"].append(np.asarray(missing.numpy(), np.float32))
            out["sha256"].append(hashlib.sha256(tokens.float().contiguous().numpy().tobytes()).hexdigest())
    store = dict(file_txt1=np.asarray(txt1, np.int64), report_file=np.asarray(report_file, np.int64),
                 report_len=np.asarray(M.GOLDEN_LENGTHS, np.int64), case_file=np.asarray(out["case_file"], np.int64),
                 case_comb=np.asarray(out["case_comb"], np.int64), text_length=np.asarray(out["text_length"], np.int64),
                 missing=np.stack(out["missing"]), sha256=np.asarray(out["sha256"]))
    np.savez_compressed(os.path.join(GOLD, "token_report_cases.npz"), **store)
    print("cases", len(out["case_file"]), "text lengths", sorted(set(out["text_length"])), "missing[2] set in",
          int(store["missing"][:, 2].sum()))


if __name__ == "__main__":
    main()
