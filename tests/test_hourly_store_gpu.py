"""The hourly carry-forward windows and their embedding on the GPU: ``ops.hourly_windows`` (csrc/tie_store.hip) bit-equal to the
reference's ``__getitem__`` goldens and to the NumPy model, and ``ops.HourlyEmbedFn`` (csrc/elementwise.hip) against the torch
chain it replaces, forward and the four parameter gradients."""
import numpy as np
import pytest
import torch

from tests import hourly_store_model as H
from tests import tie_store_model as M
from tests.test_gpu_parity import DEV, check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from medical_tri_modal_pilot_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def gstore():
    return M.new_golden_store().to(DEV)


@pytest.fixture(scope="module")
def sstore():
    return M.new_synthetic_store().to(DEV)


def _both_roundings(ops, batch, tag):
    for r16 in (False, True):
        got = ops.hourly_windows(batch, DEV, round_fp16=r16)
        want = H.model_of(batch, r16)
        assert got.dtype == torch.float32 and tuple(got.shape) == want.shape and got.is_contiguous()
        ne = int((got.cpu().numpy().view(np.uint32) != want.view(np.uint32)).sum())
        print(f"hourly_windows[{tag}, round_fp16 {r16}]: {want.shape}, {ne} values differ")
        assert got.cpu().numpy().tobytes() == want.tobytes()
    return got


@pytest.mark.parametrize("k", range(len(H.golden_groups())))
def test_golden_cases(ops, gstore, k):
    g = H.golden()
    rt, sel = H.golden_groups()[k]
    batch = gstore.plan_hourly(g["case"][sel][:, 1:4], 24, g["keep"], rt)
    raw = ops.hourly_windows(batch, DEV, round_fp16=False)
    want = np.ascontiguousarray(g["plane0"][sel])                      # the reference's own __getitem__ output
    assert raw.cpu().numpy().tobytes() == want.tobytes()
    r16 = ops.hourly_windows(batch, DEV)
    assert torch.equal(r16.cpu(), torch.from_numpy(want).half().float())      # the trainer's .half().float()


def test_synthetic_store_with_none_hours_at_either_end(ops, sstore):
    wins, pats = M.synthetic_windows(), M.synthetic_patients()
    kinds = set().union(*(M.kinds_of(pats, *w, 1000) for w in wins.tolist()))
    assert {"none_head", "none_tail", "none_both"} <= kinds
    _both_roundings(ops, sstore.plan_hourly(wins), f"synthetic, {len(wins)} windows")


def test_edge_shapes(ops, sstore):
    # B = 1 with L = 1; L = W; a patient that is not the first (first_row > 0)
    for w, tag in (([(0, 2, 1)], "B 1, L 1"), ([(1, 25, 24)], "L = W"), ([(2, 7, 4), (1, 3, 2)], "first_row > 0")):
        b = sstore.plan_hourly(np.asarray(w))
        if "first_row" in tag:
            assert (b.first_row > 0).all()
        _both_roundings(ops, b, tag)
    # all 18 columns, and a single one
    w = np.asarray([(1, 20, 9), (0, 8, 7), (2, 10, 10)])
    assert tuple(_both_roundings(ops, sstore.plan_hourly(w, keep=[True] * 18), "F 18").shape) == (3, 24, 18)
    assert tuple(_both_roundings(ops, sstore.plan_hourly(w, keep=[17]), "F 1").shape) == (3, 24, 1)
    assert tuple(_both_roundings(ops, sstore.plan_hourly(w, 10, keep=[0, 5]), "W 10, F 2").shape) == (3, 10, 2)
    # out= a buffer pre-filled with NaN: the kernel, not a memset, writes every element
    batch = sstore.plan_hourly(w)
    out = torch.full((3, 24, 16), float("nan"), device=DEV)
    got = ops.hourly_windows(batch, DEV, out=out)
    assert got.data_ptr() == out.data_ptr() and not torch.isnan(out).any()
    assert out.cpu().numpy().tobytes() == H.model_of(batch, True).tobytes()
    # descriptor rows the plan would never make: behind the store, more rows than the window, negative -- those samples come back
    # as zeros, the neighbours stay intact
    for row, bad in ((1, (sstore.n_hours - 3, 4)), (0, (5, 25)), (2, (-1, 3)), (1, (3, -2))):
        desc = batch.descriptor()
        desc[row] = torch.tensor(bad)
        out = torch.full((3, 24, 16), float("nan"), device=DEV)
        ops.hourly_windows(batch, DEV, out=out, tables=desc.to(DEV))
        want = H.model_table(sstore.norm, sstore.n_hours, desc.numpy(), 24, batch.keep_bits, True)
        assert not want[row].any() and all(want[r].any() for r in range(3) if r != row)
        assert out.cpu().numpy().tobytes() == want.tobytes(), bad
    with pytest.raises(ValueError, match="out must be"):
        ops.hourly_windows(batch, DEV, out=torch.empty(3, 24, 15, device=DEV))
    with pytest.raises(ValueError, match="descriptor"):
        ops.hourly_windows(batch, DEV, tables=torch.zeros(3, 3, dtype=torch.int64, device=DEV))


# ---------------------------------------------------------------------------------------------------------- the embedding
# 1537 rows: the backward's 64 workgroups of four waves take 256 rows a trip, so a wave sums up to seven rows and the slab has
# all 64 rows; 67 and 24 are no multiple of the four rows a workgroup takes per trip
N_ROWS = (1, 24, 67, 96, 1537)


def _chain_inputs(n, F, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(1, n, F, generator=g).half().float()
    x[0, ::5] = 0                                            # all-zero rows (the rows behind a sample's length)
    if n > 2:
        x[0, -2:] = 0
    w = torch.randn(256, F, generator=g) * (1.7 / F ** 0.5)
    b, gam, beta = 0.05 * torch.randn(256, generator=g), 1 + 0.1 * torch.randn(256, generator=g), 0.1 * torch.randn(256, generator=g)
    dy = torch.randn(1, n, 256, generator=g)
    return x, [w, b, gam, beta], dy


@pytest.mark.parametrize("F", [1, 16, 18])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_hourly_embed_vs_torch_chain(ops, dt, F):
    for n in N_ROWS:
        x, prm, dy = _chain_inputs(n, F, 100 * F + n)
        ref_p = [p.clone().requires_grad_() for p in prm]
        ref = torch.relu(torch.nn.functional.layer_norm(torch.nn.functional.linear(x, ref_p[0], ref_p[1]), (256,), ref_p[2], ref_p[3]))
        (ref * dy).sum().backward()
        t = f"hourly_embed[{str(dt)[6:]},F={F},n={n}]"
        runs = []
        for _ in range(2):
            p = [q.clone().to(DEV).requires_grad_() for q in prm]
            out = ops.HourlyEmbedFn.apply(x.to(DEV), *p, dt)
            assert out.dtype == dt and tuple(out.shape) == (1, n, 256)
            (out.float() * dy.to(DEV).to(dt).float()).sum().backward()
            runs.append((out, [q.grad for q in p]))
        out, grads = runs[0]
        print(t, "out", float((out.detach().float().cpu() - ref.detach()).abs().max()), "grads",
              [float((a.cpu() - b.grad).abs().max() / (b.grad.abs().max() + 1e-30)) for a, b in zip(grads, ref_p)])
        check(t + ".out", out.float(), ref, 1e-5 if dt == torch.float32 else 1e-2)
        for nm, a, b in zip(("dw", "db", "dgamma", "dbeta"), grads, ref_p):
            assert a.shape == b.shape
            check(f"{t}.{nm}", a, b.grad, 1e-4 if dt == torch.float32 else 2e-2)
        # two backward calls on the same inputs: bit-identical gradients (fixed-order slab sums, no float atomics)
        assert torch.equal(runs[0][0], runs[1][0]) and all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1])), t


def test_hourly_embed_takes_a_batch_of_tables_and_refuses_other_shapes(ops):
    x, prm, _ = _chain_inputs(96, 16, 5)
    p = [q.to(DEV) for q in prm]
    a = ops.HourlyEmbedFn.apply(x.to(DEV), *p, torch.float32)
    b = ops.HourlyEmbedFn.apply(x.view(4, 24, 16).to(DEV), *p, torch.float32)
    assert tuple(b.shape) == (4, 24, 256) and torch.equal(a.view(-1), b.view(-1))
    with pytest.raises(ValueError, match="HourlyEmbedFn"):
        ops.HourlyEmbedFn.apply(x.to(DEV), p[0][:, :15].contiguous(), *p[1:], torch.float32)
