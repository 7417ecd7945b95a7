"""CPU model of the token-id reports (csrc/token_embed.hip, builder/data/report_store.TokenReportStore), the golden cases of the
reference's ``--berttype bert`` text branch (tests/golden/token_report_cases.npz) and the closed-form id lists the generator, the
CPU and the GPU tests share.

``reference_ids`` restates what the reference's ``__getitem__`` (dataset_new.py:2157-2175) with ``clinical_note_transform``
(:186-192) returns on a FIRST read of a report, written as the two branches the reference has (not as the closed form the kernel
uses): float32 ``[L]``.  It reads a plan's descriptor and a host copy of the store's ids, nothing of the package's gather.
"""
import functools
import hashlib
import os
import types

import numpy as np
import torch

import filler
from medical_tri_modal_pilot_amd.builder.data import TokenReportStore

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
L = 128                                              # --bert-token-max-length
VOCAB = 30000
GOLDEN_LENGTHS = (1, 5, 37, 125, 126, 127, 200)      # ids of the reports of the seven txt1 sample files, in file order:
#                                                      125 = L - 3 is the last short-branch case, 126 = L - 2 the first trimmed one
GOLDEN_FLAGS = dict(input_types="vslt_img_txt", modality_inclusion="train-missing_test-missing", fullmodal_definition="txt1_img1")
SPECIAL = (0, 1, 2, 3, VOCAB - 1)                    # UNK, PAD (the loader turns it into 0), BOS, EOS, the last id of the table


def golden_ids(report: int, n: int, vocab: int = VOCAB) -> list:
    """closed-form id list of golden report ``report`` (the generator fed the reference these very values): hashed ids on
    ``[0, vocab)``, every third position one of SPECIAL in turn -- a list of 13 ids or more holds all five"""
    ids = np.minimum((filler._hash_uniform(f"tokens.{report}", n).astype(np.float64) * vocab).astype(np.int64), vocab - 1)
    ids = np.abs(ids) % vocab
    for p in range(0, n, 3):
        ids[p] = SPECIAL[(p // 3 + report) % len(SPECIAL)]
    return [int(v) for v in ids]


def reference_ids(tokens, max_length: int = L) -> torch.Tensor:
    """float32 ``[max_length]`` of a first read of the id list ``tokens``, as two cases: a report that fits with its BOS and EOS is
    followed by PAD ids up to ``max_length``; a longer one loses its tail so that BOS, ids and EOS fill the vector exactly.  The
    PAD id 1 -- the padding and any genuine 1 -- then reads as 0.  An empty report is a missing sample: zeros."""
    ids = [int(v) for v in tokens]
    if not ids:
        return torch.zeros(max_length)
    BOS, EOS, PAD = 2, 3, 1
    with_bos = [BOS] + ids
    if len(with_bos) + 1 < max_length:                       # short: room for the EOS and at least one PAD
        row = with_bos + [EOS]
        row = row + [PAD] * (max_length - len(row))
    else:                                                    # long: keep max_length - 1 values, the EOS is the last
        row = with_bos[:max_length - 1] + [EOS]
    return torch.tensor([0.0 if v == PAD else float(v) for v in row], dtype=torch.float32)


def plan_ids(batch, ids) -> torch.Tensor:
    """float32 [B, L]: what the loader and the default collate build on the host for the samples of a plan"""
    ids = np.asarray(ids)
    return torch.stack([reference_ids(ids[f:f + n].tolist(), batch.max_length)
                        for f, n in zip(np.asarray(batch.first_token).tolist(), np.asarray(batch.n_tokens).tolist())])


def closed_form_ids(first, count, ids, max_length: int) -> np.ndarray:
    """int32 [B, L] by the kernel's rule: [2, t_0 .. t_{k-1}, 3, 0 ..] with k = min(n, L - 2), every 1 written as 0; a
    descriptor row outside the store, or with n <= 0, gives zeros (NumPy model of mtmp_report_ids_gather)"""
    ids = np.asarray(ids, np.int64)
    out = np.zeros((len(first), max_length), np.int32)
    for b, (f, n) in enumerate(zip(np.asarray(first).tolist(), np.asarray(count).tolist())):
        if f < 0 or n <= 0 or f + n > ids.shape[0]:
            continue
        k = min(n, max_length - 2)
        row = np.concatenate([[2], ids[f:f + k], [3]])
        row[row == 1] = 0
        out[b, :k + 2] = row
    return out


def digest(t) -> str:
    t = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    assert t.dtype == np.float32
    return hashlib.sha256(t.tobytes()).hexdigest()


# ----------------------------------------------------------------------------------------------------------------- golden
@functools.lru_cache(None)
def golden():
    with np.load(os.path.join(GOLD, "token_report_cases.npz")) as z:
        return {k: z[k] for k in z.files}


def golden_mapping():
    """the dict the generator handed the reference as ``ds.txtDict`` (a fresh copy per read), keyed ``(file index, 0)`` here: the
    real (pat_id, chid) pairs are not committed"""
    g = golden()
    return {(int(i), 0): golden_ids(int(i), int(n)) for i, n in zip(g["report_file"], g["report_len"])}


def golden_store() -> TokenReportStore:
    return TokenReportStore.from_mapping(golden_mapping())


def golden_report_idx(store):
    """per golden case the report index a loader would hand over: ``index_of`` under ``report_wanted``, -1 otherwise (a txt0 file
    is never looked up).  The file name carries what the gate reads of it, the txt0 / txt1 tag."""
    from medical_tri_modal_pilot_amd.builder.data import report_wanted
    g, args = golden(), types.SimpleNamespace(**GOLDEN_FLAGS)
    names = [f"{int(i)}_txt{int(t)}.pkl" for i, t in enumerate(g["file_txt1"])]
    return np.asarray([store.index_of(int(f), 0) if report_wanted(args, names[int(f)]) else -1 for f in g["case_file"]], np.int64)


# -------------------------------------------------------------------------------------------------------------- the gradient
def embed_grad_reference(ids, dy, V: int):
    """float64 ``index_add`` of dy's rows by id and the worst-case error bound of ANY float32 summation order of them:
    ``n_v * 2**-24 * sum_t |dy[t, c]|`` over the id's rows (every one of the n_v - 1 additions rounds a partial sum that is at
    most the sum of the magnitudes, relative error 2**-24 each; derived, not measured).  Ids outside [0, V) contribute nothing.
    Returns (dw float64 [V, D], bound float64 [V, D], touched bool [V])."""
    ids = ids.reshape(-1).long()
    dy64 = dy.reshape(ids.numel(), -1).double()
    ok = (ids >= 0) & (ids < V)
    dw = torch.zeros(V, dy64.shape[1], dtype=torch.float64, device=dy.device).index_add_(0, ids[ok], dy64[ok])
    mag = torch.zeros_like(dw).index_add_(0, ids[ok], dy64[ok].abs())
    n = torch.zeros(V, dtype=torch.float64, device=dy.device).index_add_(0, ids[ok], torch.ones(int(ok.sum()), dtype=torch.float64,
                                                                                               device=dy.device))
    return dw, n.unsqueeze(1) * 2.0 ** -24 * mag, n > 0
