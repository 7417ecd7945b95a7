"""The preamble the four store gathers share (ops._store_gather): ``ops.tie_windows`` refuses tables of another shape or type on
the host, before anything is launched, and "cuda" means the device the store is on -- the result is there, with the bits of the call
that names ``cuda:0``.  (The model call validate() and get_trainer(flow_type="test") share is covered by
tests/test_validation_gpu.py::test_validate_eager_equals_the_test_flow, bit for bit.)"""
import numpy as np
import pytest
import torch

from medical_tri_modal_pilot_amd.builder.data import ReportStore, TokenReportStore
from tests import tie_store_model as M
from tests.test_gpu_parity import DEV

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from medical_tri_modal_pilot_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def sstore():
    return M.new_synthetic_store().to(DEV)


def test_tie_windows_checks_its_tables_on_the_host(ops, sstore):
    """the synthetic patients' store of tests/test_tie_store_gpu.py, B 3"""
    batch = sstore.plan(np.asarray([(0, 8, 7), (0, 8, 7), (0, 11, 3)]), 1000, 1)
    B, n = batch.batch_size, batch.total_rows
    desc, cu = batch.descriptor().to(DEV), batch.cu_seqlens.to(DEV)
    assert B == 3 and tuple(desc.shape) == (3, 8) and tuple(cu.shape) == (4,)
    want = ops.tie_windows(batch, DEV, 64).events
    got = ops.tie_windows(batch, DEV, 64, tables=(desc, cu)).events
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and got.device == torch.device(DEV)
    for tables, word in (((desc[:, :7].contiguous(), cu), "descriptor"), ((desc[:B - 1].contiguous(), cu), "descriptor"),
                         ((desc.to(torch.int32), cu), "descriptor"), ((desc, cu[:B].contiguous()), "cu_seqlens")):
        out = torch.full((n, 3), float("nan"), device=DEV)
        with pytest.raises(ValueError, match=word):
            ops.tie_windows(batch, DEV, 64, out=out, tables=tables)
        torch.cuda.synchronize()
        assert torch.isnan(out).all(), word                # nothing was launched


def test_cuda_without_an_index_is_the_stores_device(ops, sstore):
    """B 2 for each op; max_tokens 3 and width 8 for reports, max_length 5 for ids, window_size 4 for hourly windows"""
    assert sstore.device == torch.device("cuda", 0) and torch.cuda.current_device() == 0
    wins = np.asarray([(0, 8, 4), (2, 7, 3)])
    reports = ReportStore.from_mapping({f"r{k}": {"embedding": np.arange(8 * n, dtype=np.float32).reshape(n, 8) + k}
                                        for k, n in enumerate((3, 1))}, width=8, max_tokens=3).to(DEV)
    ids = TokenReportStore.from_mapping({(k, 0): list(range(7, 7 + n)) for k, n in enumerate((6, 2))}, max_length=5).to(DEV)
    tie, hourly = sstore.plan(wins, 1000, 1), sstore.plan_hourly(wins, 4)
    rep, tok = reports.plan(np.asarray([0, 1])), ids.plan(np.asarray([0, 1]))
    assert tie.batch_size == hourly.batch_size == rep.batch_size == tok.batch_size == 2
    calls = {"tie_windows": lambda d: ops.tie_windows(tie, d, 64).events,
             "tie_windows padded": lambda d: ops.tie_windows(tie, d, 64, padded=True),
             "hourly_windows": lambda d: ops.hourly_windows(hourly, d),
             "report_tokens float32": lambda d: ops.report_tokens(rep, d, torch.float32),
             "report_tokens bfloat16": lambda d: ops.report_tokens(rep, d, torch.bfloat16),
             "report_token_ids": lambda d: ops.report_token_ids(tok, d)}
    for name, fn in calls.items():
        named, bare = fn(torch.device("cuda", 0)), fn("cuda")
        assert bare.device == named.device == torch.device("cuda", 0), name
        assert bare.shape == named.shape and bare.dtype == named.dtype, name
        assert torch.equal(bare.contiguous().view(torch.uint8), named.contiguous().view(torch.uint8)), name
        assert bool(named.any()), name                     # not a comparison of two empty results
