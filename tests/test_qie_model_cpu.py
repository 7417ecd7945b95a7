"""CPU-only: the float64 models of tests/qie_model.py are the torch modules' chains (nn.Linear, nn.LayerNorm, nn.BatchNorm1d, autograd)
to 1e-12; every seeded fault a QIE kernel could make exceeds the bound the GPU tests hold the kernels to; the seeds' gate margins;
the new C entries are declared, bound and the ABI is still 6."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import head_model as HM
from tests import qie_model as Q
from tests import row_kernels_model as R

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
D = Q.D


def _close(a, b, tol=1e-12):
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def _demo_module(prm):
    m = nn.Sequential(nn.Linear(2, D), nn.LayerNorm(D, eps=Q.LN_EPS), nn.ReLU()).double()
    with torch.no_grad():
        for q, v in zip((m[0].weight, m[0].bias, m[1].weight, m[1].bias), prm):
            q.copy_(v.double())
    return m


@pytest.mark.parametrize("with_time", [True, False])
@pytest.mark.parametrize("B,N_v", [(1, 1), (3, 9), (5, 24)])
def test_adds_model_is_the_torch_chain(B, N_v, with_time):
    """demo = ie_demo([age, gender]) added to every token of the three streams: the add rows, and through autograd of
    sum((x + add) * dx) the gradients of it / tt and of the four ie_demo parameters (tri_mbt_vsltcls.py:191-198, 216-221)"""
    inp = Q.adds_inputs(B, N_v, F32, 0, with_time)
    ref = Q.adds_chain(inp, ft=F64)
    m = _demo_module(inp["params"])
    demo = m(torch.stack([inp["age"], inp["gender"]], 1).double())
    assert _close(ref["add_v"], demo)
    loss = (demo.unsqueeze(1) * inp["dx_v"].double()).sum()
    if with_time:
        it, tt = inp["it"].double().requires_grad_(), inp["tt"].double().requires_grad_()
        ai, at = it + demo, tt + demo
        assert _close(ref["add_i"], ai) and _close(ref["add_t"], at)
        loss = loss + (ai.unsqueeze(1) * inp["dx_i"].double()).sum() + (at.unsqueeze(1) * inp["dx_t"].double()).sum()
    loss.backward()
    if with_time:
        assert _close(ref["d_it"], it.grad) and _close(ref["d_tt"], tt.grad)
    for k, q in zip(Q.ADD_GRADS, (m[0].weight, m[0].bias, m[1].weight, m[1].bias)):
        assert _close(ref[k], q.grad), k
        assert _close(ref["per_sample"][k].sum(0), q.grad), k


def test_stream_rows_model_is_layer_norm_of_cls_and_tokens_plus_add():
    g = torch.Generator().manual_seed(3)
    x, add, cls = torch.randn(3, 5, D, generator=g), torch.randn(3, D, generator=g), torch.randn(D, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    want = F.layer_norm(torch.cat([cls.double().view(1, 1, D).expand(3, 1, D), x.double() + add.double().unsqueeze(1)], 1), (D,),
                        gamma.double(), beta.double(), 1e-5)
    assert _close(Q.stream_rows(x, add, cls, gamma, beta, ft=F64), want)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("B", [2, 5, 64])
def test_head_model_is_the_torch_chain(B, training):
    inp = Q.qhead_inputs(B, F32, 0)
    ref = Q.qhead_chain(inp, training, ft=F64)
    ln = nn.LayerNorm(D, eps=Q.LN_EPS).double()
    fc = nn.Sequential(nn.Linear(D, D), nn.BatchNorm1d(D, eps=Q.BN_EPS, momentum=Q.MOMENTUM), nn.ReLU(), nn.Linear(D, 1)).double()
    P = [ln.weight, ln.bias, fc[0].weight, fc[0].bias, fc[1].weight, fc[1].bias, fc[3].weight, fc[3].bias]
    with torch.no_grad():
        for q, v in zip(P, inp["params"]):
            q.copy_(v.double())
        fc[1].running_mean.copy_(inp["run_mean"].double())
        fc[1].running_var.copy_(inp["run_var"].double())
    fc.train(training)
    cls = inp["cls"].double().requires_grad_()
    o = fc(ln(cls))
    (o * inp["w"].double()).sum().backward()
    assert _close(ref["o"], o) and _close(ref["dcls"], cls.grad)
    assert _close(ref["run_mean"], fc[1].running_mean) and _close(ref["run_var"], fc[1].running_var)
    for k, q in zip(Q.HEAD_GRADS, P):
        assert _close(ref[k].reshape(q.shape), q.grad, 1e-11), k


# ------------------------------------------------------------------------------------------ seeded faults
@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("fault", Q.ADD_FAULTS)
def test_adds_fault_exceeds_the_bound(fault, dt):
    """the dx_v sum one token short, the dx_i share dropped, d_demo rounded to bf16 in front of the ie_demo backward, the
    LayerNorm eps taken for BatchNorm's: each is visible in a parameter gradient (d_demo_bf16 too: ~4e-3 against a bound of ~3e-6)"""
    for B, N_v in ((2, 9), (64, 24), (3, 1000)):
        c = Q.adds_case(B, N_v, dt)
        bad = Q.adds_chain(c["inp"], ft=F64, fault=fault)
        over = {k: R.err(bad[k], c["ref"][k]) / R.bound(c["e_torch"][k]) for k in Q.ADD_GRADS}
        assert max(over.values()) > 50, (fault, B, N_v, over)
        if fault != "eps_swapped":                   # (ddemo_be does not depend on eps)
            assert min(over.values()) > 50, (fault, B, N_v, over)


@pytest.mark.parametrize("fault", Q.ROW_FAULTS)
def test_row_fault_exceeds_the_bound(fault):
    """demo not added to the CLS row's neighbour (token 0), demo added to the CLS row, demo added behind the LayerNorm"""
    inp = Q.adds_inputs(4, 9, F32, 0)
    demo = Q.adds_chain(inp, ft=F64)["add_v"].float()
    g = torch.Generator().manual_seed(11)
    x, cls = torch.randn(4, 9, D, generator=g), torch.randn(D, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    ref, f32 = Q.stream_rows(x, demo, cls, gamma, beta, ft=F64), Q.stream_rows(x, demo, cls, gamma, beta, ft=F32)
    bound = R.bound(R.err(f32, ref))
    bad = Q.stream_rows(x, demo, cls, gamma, beta, ft=F64, fault=fault)
    assert R.err(bad, ref) > 50 * bound, (fault, R.err(bad, ref), bound)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("fault", Q.HEAD_FAULTS)
def test_head_fault_exceeds_the_bound(fault, training):
    """a head that still walks 512 columns per row; LayerNorm and BatchNorm eps swapped"""
    for B in (5, 64, 129):
        c = Q.qhead_case(B, F32, training)
        bad = Q.qhead_chain(c["inp"], training, ft=F64, fault=fault)
        over = {k: Q.qhead_err(k, bad[k], c["ref"], training) / R.bound(c["e_torch"][k]) for k in ("o", "dcls", "dw1", "dbn_g")}
        assert max(over.values()) > 50, (fault, B, over)


def test_seeds_keep_every_gate_clear_of_zero():
    for B, s in Q.SEEDS.items():
        assert Q.adds_chain(Q.adds_inputs(B, 3, F32, s, False), ft=F64)["margin"] > Q.GATE_MARGIN, B
    for B, s in Q.HEAD_SEEDS.items():
        for dt in (F32, BF16):
            for tr in HM.modes(B):
                assert Q.qhead_chain(Q.qhead_inputs(B, dt, s), tr, ft=F64)["margin"] > Q.GATE_MARGIN, (B, dt, tr)


def test_new_entries_are_declared_and_the_abi_is_6():
    from medical_tri_modal_pilot_amd import _lib
    from tests import abi
    for name in ("mtmp_qie_adds_fwd", "mtmp_qie_adds_bwd", "mtmp_qie_adds_bwd_ws_floats", "mtmp_headq_ws_floats", "mtmp_headq_fwd_t",
                 "mtmp_headq_bwd_scatter"):
        assert name in _lib.SIGNATURES and name in abi.declarations(), name
    assert len(_lib.SIGNATURES["mtmp_headq_bwd_scatter"][1]) == len(_lib.SIGNATURES["mtmp_head_bwd_scatter"][1]) - 2
    assert len(_lib.SIGNATURES["mtmp_headq_fwd_t"][1]) == len(_lib.SIGNATURES["mtmp_head_fwd_t"][1]) - 2
    assert "#define MTMP_ABI_VERSION 6\n" in abi.header_text()
