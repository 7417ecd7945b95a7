"""-m gpu: the contract the one layer engine (ops.layer_forward / ops.layer_backward over lists of streams) rests on.  In bf16 a
group of ONE stream is bit-identical to the chain of single-stream wrappers written out below -- the single C entries and the
``_grouped`` entries share their argument builders and launchers (csrc/gemm.hip: "the single form IS a group of one"), so the
engine needs no single-stream copy.  In fp32 the stream-list ops launch per stream: a list of two streams equals two lists of one."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 256


@pytest.fixture(scope="module")
def ops():
    from medical_tri_modal_pilot_amd import ops as _ops
    return _ops


def _layer(dtype, seed):
    from medical_tri_modal_pilot_amd.builder.models.src.transformer.encoder import TransformerEncoderLayer
    torch.manual_seed(seed)
    layer = TransformerEncoderLayer(d_model=D, num_heads=4, d_ff=1024, dropout_p=0.0).to(DEV)
    with torch.no_grad():
        for prm in layer.parameters():
            if prm.dim() > 1:
                prm.mul_(3.0)
    return layer.param_list(), type(layer).fused_weights_of([layer], dtype)[0]


def _chain(ops, z, kv, P, fused, p, seeds, d_out, mask):
    """one layer, forward and backward, through the single-stream wrappers -> (out, dz, the 14 gradients in parameter order)"""
    f = ops.FusedWeights._make(fused)
    B, N, _ = z.shape
    M = B * N
    z2, d2 = z.view(M, D), d_out.view(M, D)
    qkv, xn1, st1, knorm = ops.ln_gemm_qkv(z2, P[ops.P_G1], P[ops.P_B1], f.wqkv, f.bqkv)
    qkv = qkv.view(B, N, 3 * D)
    o, r1, lse = ops.attn_fwd(qkv, kv, res=z, knorm=knorm, qk_mask=mask)
    r1_2 = r1.view(M, D)
    h, xn2, st2, hsign = ops.ln_gemm(r1_2, P[ops.P_G2], P[ops.P_B2], f.w1, P[ops.P_C1], 4 * D, relu=True, drop_p=p, seed=seeds[0],
                                     want_signs=True)
    out = ops.gemm_nt(h, f.w2, P[ops.P_C2], res2d=r1_2, drop_p=p, seed=seeds[1])
    red = []
    if p > 0:
        dh, dy2 = ops.gemm_nt_signs(d2, f.w2t, hsign, 1.0 / (1.0 - p), drop_p=p, seed=seeds[1])
    else:
        dh, dy2 = ops.gemm_nt_signs(d2, f.w2t, hsign, 1.0), d2
    dw2, dc2 = ops.gemm_tn(dy2, h, defer=red)
    dw1, dc1 = ops.gemm_tn(dh, xn2, defer=red)
    dr1, dg2, db2 = ops.gemm_lnbwd(dh, f.w1t, r1_2, st2, P[ops.P_G2], d_res2d=d2, defer=red)
    dqkv = ops.attn_bwd(qkv, o, dr1.view(B, N, D), lse, kv, mask).view(M, 3 * D)
    dwq, dbq = ops.gemm_tn(dqkv, xn1, defer=red)
    dz, dg1, db1 = ops.gemm_lnbwd(dqkv, f.wqkvt, z2, st1, P[ops.P_G1], d_res2d=dr1, defer=red)
    ops.reduce_batch(red)
    grads = (dg1, db1, dwq[:D], dbq[:D], dwq[D:2 * D], dbq[D:2 * D], dwq[2 * D:], dbq[2 * D:], dg2, db2, dw1, dc1, dw2, dc2)
    return out.view(B, N, D), dz.view(B, N, D), grads


def _engine(ops, zs, kvs, Ps, fuseds, p, seeds, d_outs, masks=None):
    outs, saved = ops.layer_forward(zs, kvs, Ps, fuseds, p, seeds, qk_masks=masks)
    dzs, grads = ops.layer_backward(saved, d_outs)
    return outs, dzs, grads


def _tn_plan_accepts(M, N, K):
    from medical_tri_modal_pilot_amd import _lib
    splits = (ctypes.c_int * 1)()
    return _lib.lib().mtmp_gemm_tn_group_plan(1, (ctypes.c_int * 1)(M), N, K, splits) == 0


# (B, N, key lengths, prefix mask): M = 210 is no multiple of the 128-row tile, one sample of a single key; one row in all; M = 8192,
# where the three weight gradients take the grouped LDS-DMA launch (asserted below) instead of the per-stream fallback
CASES = [(3, 70, [70, 1, 33], None), (3, 70, [70, 1, 33], [0b0110, 0b0100, 0b1000, 0b0010]), (1, 1, [1], None),
         (8, 1024, [1024, 1, 513, 700, 1024, 64, 65, 999], None)]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B,N,lens,mask", CASES)
def test_bf16_group_of_one_is_the_single_wrapper_chain(ops, B, N, lens, mask, p):
    if B * N == 8192:
        for n_out, k in ((3 * D, D), (4 * D, D), (D, 4 * D)):
            assert _tn_plan_accepts(B * N, n_out, k), (n_out, k)
    dt = torch.bfloat16
    P, fused = _layer(dt, 7)
    g = torch.Generator().manual_seed(100 * B + N)
    z = torch.randn(B, N, D, generator=g).to(DEV, dt)
    d_out = torch.randn(B, N, D, generator=g).to(DEV, dt)
    kv = torch.tensor(lens, dtype=torch.int32, device=DEV)
    seeds = (1234, 98765)
    out_c, dz_c, g_c = _chain(ops, z, kv, P, fused, p, seeds, d_out, mask)
    (out_e,), (dz_e,), (g_e,) = _engine(ops, [z], [kv], [P], [fused], p, [seeds], [d_out.clone()], [mask])
    assert torch.equal(out_e, out_c), "out"
    assert torch.equal(dz_e, dz_c), "dz"
    assert len(g_e) == len(g_c) == ops.PARAMS_PER_LAYER
    for k, (a, b) in enumerate(zip(g_e, g_c)):
        assert torch.equal(a, b), f"gradient {k}"


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_fp32_list_of_two_equals_two_lists_of_one(ops, p):
    dt = torch.float32
    B, Ns = 3, (54, 133)
    lens = ([54, 7, 1], [100, 133, 2])
    g = torch.Generator().manual_seed(5)
    layers = [_layer(dt, 11 + i) for i in range(2)]
    Ps, fuseds = [l[0] for l in layers], [l[1] for l in layers]
    zs = [torch.randn(B, N, D, generator=g).to(DEV) for N in Ns]
    d_outs = [torch.randn(B, N, D, generator=g).to(DEV) for N in Ns]
    kvs = [torch.tensor(ln, dtype=torch.int32, device=DEV) for ln in lens]
    seeds = [(11, 12), (13, 14)]
    outs, dzs, grads = _engine(ops, zs, kvs, Ps, fuseds, p, seeds, [d.clone() for d in d_outs])
    for i in range(2):
        (out1,), (dz1,), (g1,) = _engine(ops, [zs[i]], [kvs[i]], [Ps[i]], [fuseds[i]], p, [seeds[i]], [d_outs[i].clone()])
        assert torch.equal(outs[i], out1) and torch.equal(dzs[i], dz1), i
        for k, (a, b) in enumerate(zip(grads[i], g1)):
            assert torch.equal(a, b), (i, k)
