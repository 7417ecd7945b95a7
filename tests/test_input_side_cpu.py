"""What the input stores share on the host: the two report stores resolve a batch by ONE control flow
(builder/data/report_store.py ``_resolve``), and ``resolve_device`` leaves alone what already names one device."""
import numpy as np
import torch

from medical_tri_modal_pilot_amd.builder.data import ReportStore, TokenReportStore, resolve_device

COUNTS = (0, 1, 37, 128, 127)
IDX, COMB = [0, -1, 3, 1, 2, 4], [0, 0, 1, 3, 2, 0]


def test_the_two_report_stores_plan_alike():
    """the same per-report counts in both stores, the same indices (a missing sample, an empty report) and combinations (1 and 3
    drop the report): the plans agree in everything but what they hold"""
    emb = ReportStore.from_mapping({f"r{k}": {"embedding": np.full((n, 8), k + 1.0, np.float32)} for k, n in enumerate(COUNTS)},
                                   width=8)
    tok = TokenReportStore.from_mapping({(k, 0): [5 + k] * n for k, n in enumerate(COUNTS)})
    assert emb.n_reports == tok.n_reports == 5 and emb.n_tokens == tok.n_tokens == sum(COUNTS)
    assert np.array_equal(emb.tok_ptr, tok.tok_ptr)
    a, b = emb.plan(np.asarray(IDX), np.asarray(COMB)), tok.plan(np.asarray(IDX), np.asarray(COMB))
    # report 3 goes with combination 1 and report 1 with combination 3; report 0 is empty, sample 1 has none
    assert a.n_tokens.tolist() == [0, 0, 0, 0, 37, 127] and a.first_token.tolist() == [0, 0, 0, 0, 1, 166]
    assert a.missing.tolist() == [1, 1, 1, 1, 0, 0]
    for name in ("report_idx", "first_token", "n_tokens"):
        assert np.array_equal(getattr(a, name), getattr(b, name)) and getattr(a, name).dtype == getattr(b, name).dtype == np.int64
    for name in ("txt_lengths", "missing"):
        assert torch.equal(getattr(a, name), getattr(b, name)) and getattr(a, name).dtype == getattr(b, name).dtype
    assert torch.equal(a.descriptor(), b.descriptor()) and a.descriptor().dtype == torch.int64 and a.batch_size == b.batch_size == 6
    assert torch.equal(b.key_lengths, torch.minimum(b.txt_lengths, torch.tensor(tok.max_length - 2)))
    full = tok.plan(np.asarray([3, 4, 2]))                 # 128 and 127 ids are trimmed to L - 2, 37 are not
    assert full.txt_lengths.tolist() == [128, 127, 37] and full.key_lengths.tolist() == [126, 126, 37]


def test_resolve_device_returns_a_named_device_as_given():
    assert resolve_device("cpu") == torch.device("cpu")
    d = torch.device("cuda", 0)
    assert resolve_device(d) == d and resolve_device(d).index == 0
    assert resolve_device("cuda:1") == torch.device("cuda", 1)
