"""The report embeddings of a whole data set on the device, and the host plan of a batch of them.

The reference's loader (dataset_new.py:2135-2155) opens ``self.bioemb[text]['embedding'][:]`` for every sample -- a random read of
an h5 file --, makes a float32 ``[len, 768]`` tensor, appends zeros up to ``[128, 768]``, and the collate stacks ``[B, 128, 768]``,
which the trainer then copies to the device: 25 MB per step at B 64, most of them zeros.  The embeddings are frozen, so they are
stored once (``ReportStore``, CSR over reports -> token rows), a sample is ONE integer, the index of its report, the host resolves
the reference's control flow for a batch on the token counts alone (``ReportStore.plan`` -> ``ReportBatch``, vectorised, no
embedding is touched) and one kernel launch (``ops.report_tokens`` -> csrc/report_store.hip) writes what the text projection reads.

What is stored, and why the result has the bits of the reference: the values rounded to float32 once, as ``torch.Tensor(...)``
rounds them; in a bfloat16 store those float32 values rounded once more by torch's own ``.to(torch.bfloat16)`` on the host -- the
rounding the bf16 build's projection applies to its input anyway.  The gather copies or converts, it does no other arithmetic.
"""
import numpy as np
import torch

from . import resolve_device

DESC_WORDS = 2      # int64 words per sample of the kernel's descriptor (include/mtmp.h, mtmp_report_gather): first row, rows


def report_wanted(args, file_name: str) -> bool:
    """The reference's gate in front of the text branch (dataset_new.py:2137), verbatim -- the ``test-`` prefixes inside the
    TRAINING data set are its own."""
    return bool((("txt" in args.input_types and "txt1" in args.fullmodal_definition and 'test-full' in args.modality_inclusion)
                 or ('test-missing' in args.modality_inclusion and "txt" in args.input_types)) and ("txt1" in file_name))


class _ReportBatch:
    """What the report plans share.  A subclass declares ``berttype`` (the ``--berttype`` of the models that read it), ``holds``
    (its noun in the trainer's messages), ``model_lengths`` (the attribute the model's key mask reads) and ``gather`` (the one launch
    that makes the device tensor): the trainer's text input is driven by these four."""

    def __init__(self, store, report_idx, first_token, n_tokens, txt_lengths, missing):
        self.store, self.report_idx = store, report_idx
        self.first_token, self.n_tokens = first_token, n_tokens          # int64 [B] each; 0 tokens when missing
        self.txt_lengths, self.missing = txt_lengths, missing            # int64 [B]; float32 [B], column 2 of the loader's `missing`

    @property
    def batch_size(self) -> int:
        return int(self.txt_lengths.numel())

    def descriptor(self) -> torch.Tensor:
        """int64 [B, DESC_WORDS]: the per-sample words of mtmp_report_gather and mtmp_report_ids_gather."""
        return torch.from_numpy(np.ascontiguousarray(np.stack([self.first_token, self.n_tokens], axis=1).astype(np.int64)))


class _ReportStoreBase:
    """What the report stores share: ``tok_ptr`` int64 [R + 1] (host, numpy), the key -> index map, the plan on the counts."""

    def __init__(self, tok_ptr, index):
        self.tok_ptr, self._index = tok_ptr, index
        self.device = torch.device("cpu")

    @staticmethod
    def _csr(counts, rows, empty):
        """per-report arrays -> (tok_ptr, their concatenation; ``empty`` without a report)"""
        tok_ptr = np.zeros(len(counts) + 1, np.int64)
        np.cumsum(np.asarray(counts, np.int64), out=tok_ptr[1:])
        return tok_ptr, np.concatenate(rows, axis=0) if rows else empty

    @property
    def n_reports(self) -> int:
        return int(self.tok_ptr.shape[0] - 1)

    @property
    def n_tokens(self) -> int:
        return int(self.tok_ptr[-1])

    def _resolve(self, report_idx, missing_comb):
        """The text branch's control flow on the counts alone, vectorised over the batch -> (report index, first row, rows, missing)
        of every sample; no embedding and no id is touched."""
        idx = np.asarray(report_idx)
        if idx.ndim != 1 or idx.shape[0] < 1 or idx.dtype.kind not in "iu":
            raise ValueError(f"plan: report_idx must be an integer array [B >= 1], got {idx.dtype} {idx.shape}")
        idx = idx.astype(np.int64)
        if (idx >= self.n_reports).any():
            b = int(np.flatnonzero(idx >= self.n_reports)[0])
            raise ValueError(f"plan: sample {b} names report {int(idx[b])}, the store holds 0..{self.n_reports - 1}")
        have = idx >= 0
        at = np.where(have, idx, 0)
        first = self.tok_ptr[at] if self.n_reports else np.zeros_like(at)
        n = (self.tok_ptr[at + 1] - first) if self.n_reports else np.zeros_like(at)
        miss = ~have | (n == 0)
        if missing_comb is not None:
            mc = np.broadcast_to(np.asarray(missing_comb), idx.shape)
            miss = miss | (mc == 1) | (mc == 3)
        n = np.where(miss, 0, n).astype(np.int64)
        first = np.where(miss, 0, first).astype(np.int64)
        return idx, first, n, miss


class ReportBatch(_ReportBatch):
    """The host plan of a batch of reports: everything but the embeddings.  ``ops.report_tokens`` turns it into the
    ``[B, max_tokens, width]`` tensor on the device; the lengths and the missing flags are here without a device sync."""
    berttype, holds, model_lengths = "biobert", "BioBERT token embeddings", "txt_lengths"

    def __init__(self, store, report_idx, first_token, n_tokens, txt_lengths, missing):
        super().__init__(store, report_idx, first_token, n_tokens, txt_lengths, missing)
        self.max_tokens, self.width = store.max_tokens, store.width

    def gather(self, device, dtype):
        from medical_tri_modal_pilot_amd import ops
        return ops.report_tokens(self, device, dtype)


class ReportStore(_ReportStoreBase):
    """CSR form of all reports' token embeddings: ``tok_ptr`` int64 [R + 1] (host, numpy) and ``emb`` [total_tokens, width]
    (a torch tensor: float32 on the host after building, float32 or bfloat16 wherever ``to`` put it)."""

    def __init__(self, tok_ptr, emb, index, width: int = 768, max_tokens: int = 128):
        super().__init__(tok_ptr, index)
        self.emb, self.width, self.max_tokens = emb, int(width), int(max_tokens)

    # ------------------------------------------------------------------------------------------------------------ building
    @classmethod
    def from_mapping(cls, mapping, width: int = 768, max_tokens: int = 128):
        """``mapping[text]['embedding'][:]`` -> array, the shape of the reference's h5 file (an open ``h5py.File`` or a plain
        dict of ``{'embedding': ndarray}``), in the mapping's own order.  Keys are indexed by ``text.strip()``, the form the
        loader looks a report up by; a key that strips to nothing can never be asked for and is left out."""
        if width < 8 or width % 8:
            raise ValueError(f"ReportStore: width {width} is not a positive multiple of 8 (16-byte pieces in float32 and bfloat16)")
        index, counts, rows = {}, [], []
        for text in mapping:
            key = str(text).strip()
            if not key:
                continue
            if key in index:
                raise ValueError(f"ReportStore: two reports share the key {key[:40]!r} once stripped")
            a = np.asarray(mapping[text]['embedding'][:])
            name = f"report {len(counts)} ({key[:40]!r})"
            if a.ndim == 1:
                raise NotImplementedError(f"ReportStore: {name} is a 1-D CLS vector of {a.shape[0]} values (txt_token_size == 1, "
                                          "dataset_new.py:1590-1593): no model here takes [B, width] report batches")
            if a.ndim != 2 or a.shape[1] != width:
                raise ValueError(f"ReportStore: {name} has shape {tuple(a.shape)}, want [tokens, {width}]")
            if a.shape[0] > max_tokens:
                raise ValueError(f"ReportStore: {name} has {a.shape[0]} tokens, more than max_tokens {max_tokens} (the reference's "
                                 f"torch.zeros([{max_tokens} - len, {width}]) raises there too)")
            with np.errstate(over="ignore"):
                a = a.astype(np.float32)                                  # the one rounding of torch.Tensor(...)
            if not np.isfinite(a).all():
                raise ValueError(f"ReportStore: {name} holds a non-finite value")
            index[key] = len(counts)
            counts.append(a.shape[0])
            rows.append(a)
        tok_ptr, emb = cls._csr(counts, rows, np.zeros((0, width), np.float32))
        return cls(tok_ptr, torch.from_numpy(np.ascontiguousarray(emb)), index, width, max_tokens)

    def index_of(self, text: str) -> int:
        """index of the report the loader would look up by ``text.strip()``; -1 for an empty stripped text (the reference's
        ``len(text_data) != 0``) or a key the store does not hold"""
        key = str(text).strip()
        return self._index.get(key, -1) if key else -1

    # ------------------------------------------------------------------------------------------------------------ placement
    @property
    def dtype(self) -> torch.dtype:
        return self.emb.dtype

    @property
    def nbytes(self) -> int:
        """size of the embeddings as they are held: 4 * width bytes per token in float32, 2 * width in bfloat16"""
        return int(self.emb.numel() * self.emb.element_size())

    def to(self, device, dtype: torch.dtype = torch.float32):
        """Upload once, in ``dtype``.  bfloat16 is made on the HOST by torch's ``.to(torch.bfloat16)``, which defines the bits.  The
        embeddings move (no host copy is kept); ``tok_ptr`` stays on the host for ``plan``."""
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"ReportStore.to: float32 or bfloat16, got {dtype}")
        device = resolve_device(device)
        if device == self.device and dtype == self.emb.dtype:
            return self
        if self.device.type != "cpu" or self.emb.dtype != torch.float32:
            raise RuntimeError(f"ReportStore.to: the store is already {self.emb.dtype} on {self.device} and keeps no float32 host "
                               "copy; build another one for another device or type")
        self.emb = self.emb.to(dtype).to(device)
        self.device = self.emb.device
        return self

    # ------------------------------------------------------------------------------------------------------------ the plan
    def plan(self, report_idx, missing_comb=None) -> ReportBatch:
        """``report_idx`` int [B]: the report of every sample, -1 where ``report_wanted`` is false or ``index_of`` gave -1;
        ``missing_comb``: the loader's per-sample (or one for all) modality combination, 1 and 3 drop the report (:2148-2149).
        The text branch's control flow on the token counts, vectorised over the batch."""
        idx, first, n, miss = self._resolve(report_idx, missing_comb)
        return ReportBatch(self, idx, first, n, torch.from_numpy(n.copy()), torch.from_numpy(miss.astype(np.float32)))


# ------------------------------------------------------------------------------------------------- token-id reports (--berttype bert)
# The reference's second text branch (dataset_new.py:2157-2175): a report is a list of token ids, ``txtDict[(pat_id, chid)]``, and the
# model looks them up in a TRAINED ``nn.Embedding(30000, 256)``.  Per sample the loader puts a BOS (2) in front, lets
# ``clinical_note_transform`` (:186-192) trim to ``L - 1`` values, append an EOS (3) and pad with 1 up to ``L =
# --bert-token-max-length``, and replaces every 1 by 0.  With ``n`` ids and ``k = min(n, L - 2)`` that is
#     tokens[L] = [2, t_0 .. t_{k-1}, 3, 0 .. 0]  with every 1 written as 0,        textLength = n (NOT trimmed),
# and zeros with textLength 0 for a missing sample.  The ids are stored once (``TokenReportStore``), a sample is ONE integer, the plan
# is the control flow on the counts, and ``ops.report_token_ids`` (csrc/token_embed.hip) writes the int32 ``[B, L]`` batch.
#
# Two things the reference does that the store does NOT reproduce: (1) ``tokens.insert(0, 2)`` and the short branch's
# ``tokens.append(3)`` change the list INSIDE ``txtDict``, so the same report grows by a BOS and an EOS on every read -- the store
# reproduces a FIRST read, of a copy it made; (2) a key that ``txtDict`` lacks raises ``KeyError`` in ``__getitem__`` (the data set's
# ``__init__`` drops such files beforehand, :300-308) -- here ``index_of`` gives -1 and the plan treats the sample as missing.
class TokenReportBatch(_ReportBatch):
    """The host plan of a batch of token-id reports: everything but the ids.  ``ops.report_token_ids`` turns it into the int32
    ``[B, max_length]`` tensor on the device; the lengths and the missing flags are here without a device sync.  ``txt_lengths`` is
    the reference's textLength, UNTRIMMED; the model gets ``key_lengths``, so that its key count textLength + 2 never names more
    rows than the stream has (the mask is the same: all L rows)."""
    berttype, holds, model_lengths = "bert", "token ids", "key_lengths"

    def __init__(self, store, report_idx, first_token, n_tokens, txt_lengths, key_lengths, missing):
        super().__init__(store, report_idx, first_token, n_tokens, txt_lengths, missing)
        self.key_lengths = key_lengths                                   # int64 [B]: min(textLength, L - 2), what the model's mask reads
        self.max_length = store.max_length

    def gather(self, device, dtype=None):
        from medical_tri_modal_pilot_amd import ops
        return ops.report_token_ids(self, device)


class TokenReportStore(_ReportStoreBase):
    """CSR form of all reports' token ids: ``tok_ptr`` int64 [R + 1] (host, numpy) and ``ids`` int32 [total] (a torch tensor: on
    the host after building, on the device after ``to``)."""

    def __init__(self, tok_ptr, ids, index, vocab: int = 30000, max_length: int = 128):
        super().__init__(tok_ptr, index)
        self.ids, self.vocab, self.max_length = ids, int(vocab), int(max_length)

    @classmethod
    def from_mapping(cls, mapping, vocab: int = 30000, max_length: int = 128):
        """``mapping[(pat_id, chid)]`` -> sequence of ints, the shape of the reference's ``txtDictLoad`` result, in the mapping's
        own order.  The ids are COPIED: the caller's lists are neither kept nor changed."""
        if max_length < 3:
            raise ValueError(f"TokenReportStore: max_length {max_length} < 3 leaves no room for BOS, one id and EOS")
        if vocab < 4:
            raise ValueError(f"TokenReportStore: vocab {vocab} < 4 does not hold UNK, PAD, BOS and EOS")
        index, counts, rows = {}, [], []
        for key in mapping:
            k = (int(key[0]), int(key[1]))
            if k in index:
                raise ValueError(f"TokenReportStore: two reports share the key {k}")
            a = np.array(mapping[key], copy=True)
            if a.size == 0:
                a = np.zeros(0, np.int64)
            if a.ndim != 1:
                raise ValueError(f"TokenReportStore: report {k} has shape {tuple(a.shape)}, want a flat sequence of ids")
            if a.dtype.kind not in "iu":
                raise ValueError(f"TokenReportStore: report {k} holds a non-integer value ({a.dtype})")
            if ((a < 0) | (a >= vocab)).any():
                bad = a[(a < 0) | (a >= vocab)][0]
                raise ValueError(f"TokenReportStore: report {k} holds the id {int(bad)}, outside [0, {vocab})")
            index[k] = len(counts)
            counts.append(a.shape[0])
            rows.append(a.astype(np.int32))
        tok_ptr, ids = cls._csr(counts, rows, np.zeros(0, np.int32))
        return cls(tok_ptr, torch.from_numpy(np.ascontiguousarray(ids, np.int32)), index, vocab, max_length)

    def index_of(self, pat_id, chid) -> int:
        """index of the report ``txtDict[(int(pat_id), int(chid))]``; -1 for a key the store does not hold"""
        return self._index.get((int(pat_id), int(chid)), -1)

    @property
    def nbytes(self) -> int:
        """size of the ids as they are held: 4 bytes per token"""
        return int(self.ids.numel() * 4)

    def to(self, device):
        """Upload the ids once (no host copy is kept); ``tok_ptr`` stays on the host for ``plan``."""
        device = resolve_device(device)
        if device != self.device:
            self.ids = self.ids.to(device)
            self.device = self.ids.device
        return self

    def plan(self, report_idx, missing_comb=None) -> TokenReportBatch:
        """``report_idx`` int [B]: the report of every sample, -1 where ``report_wanted`` is false or ``index_of`` gave -1;
        ``missing_comb``: the loader's per-sample (or one for all) modality combination, 1 and 3 drop the report (:2159).
        The same control flow as ``ReportStore.plan``, on the id counts alone: no id is touched."""
        idx, first, n, miss = self._resolve(report_idx, missing_comb)
        return TokenReportBatch(self, idx, first, n, torch.from_numpy(n.copy()),
                                torch.from_numpy(np.minimum(n, self.max_length - 2)), torch.from_numpy(miss.astype(np.float32)))
