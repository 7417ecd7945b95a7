"""-m gpu: prefix-masked attention (mtmp_attn_prefix_fwd / _bwd and their grouped forms) against a float64 torch softmax with the
full boolean mask, and against the plain entries where the two must agree to the bit.

The masks are the three of the multi-token bottleneck encoder (reference mbt_encoder.py:64-94): 16 rows on the vital-sign stream
(12 bottleneck rows + 4 CLS rows), 12 on the image stream (a single masked row) and 12 on the text stream.  Shapes: the smallest at
which each path can break -- one partial key tile (N 20, with kv_len 16 = only the prefix valid), no kv_len (N 61), three key tiles
(N 140), a second forward workgroup and second backward workgroups (N 300: rows / keys 128.., 256.. are no prefix rows), and one
stream long enough for the 64-key dK / dV kernel.  Bounds: those of tests/test_gpu_parity.py::test_attention_fwd_bwd."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {torch.float32: 1e-4, torch.bfloat16: 3e-2}          # test_gpu_parity.TOL
TOL_GRAD_BF16 = 4e-2                                        # test_gpu_parity.test_attention_fwd_bwd
DT = [torch.float32, torch.bfloat16]


def _v16():
    m = torch.ones(16, 16)
    for a in (0, 4, 8):
        m[a:a + 4, a:a + 4] = 0
    for c, a in ((12, 0), (13, 4), (14, 8)):
        m[c, a:a + 4] = 0
        m[a:a + 4, c] = 0
    for c in range(12, 16):
        m[c, c] = 0
    return m.ge(0.5)


def _i12():
    m = torch.zeros(12, 12)
    m[::12, :12] = 1
    for a in (0, 4, 8):
        m[a:a + 4, a:a + 4] = 0
    return m.ge(0.5)


def _t12():
    m = torch.ones(12, 12)
    for a in (0, 4, 8):
        m[a:a + 4, a:a + 4] = 0
    return m.ge(0.5)


MASKS = {"v16": _v16(), "i12": _i12(), "t12": _t12()}


def words(mask):
    return [sum(int(mask[i, j]) << j for j in range(mask.shape[1])) for i in range(mask.shape[0])]


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def check(name, got, ref, tol):
    e = _rel(got, ref)
    print(f"{name}: rel err {e:.3e} (bound {tol:.1e})")
    assert math.isfinite(e) and e <= tol, f"{name}: rel err {e:.3e} > {tol:.1e}"


def reference(qkv, kv, mask, w):
    """float64: softmax(Q K^T / 8 + keymask + prefixmask) V per head, and the gradients of sum(o * w) -> (o, dqkv)"""
    x = qkv.double().clone().requires_grad_()
    B, N, _ = x.shape
    q, k, v = (x[..., 256 * i:256 * (i + 1)].view(B, N, 4, 64).transpose(1, 2) for i in range(3))
    s = q @ k.transpose(-1, -2) / 8.0
    full = torch.zeros(B, N, N, dtype=torch.bool)
    if kv is not None:
        full |= torch.arange(N)[None, None, :] >= kv[:, None, None]
    if mask is not None:
        P = mask.shape[0]
        full[:, :P, :P] |= mask
    o = (torch.softmax(s.masked_fill(full[:, None], float("-inf")), -1) @ v).transpose(1, 2).reshape(B, N, 256)
    (o * w.double()).sum().backward()
    return o.detach(), x.grad


def inputs(N, B, dt, seed, inflate=None):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, N, 768, generator=g)
    if inflate is not None:                              # a common direction on the prefix's queries and keys: every prefix pair
        P, gain = inflate                                # scores ~ +gain, so the masked pairs would dominate their rows
        u = torch.randn(4, 64, generator=g)
        u = (u / u.norm(dim=1, keepdim=True) * math.sqrt(8.0 * gain)).reshape(256)
        qkv[:, :P, :256] += u
        qkv[:, :P, 256:512] += u
    qkv = qkv.to(dt).float()                             # the same rounded inputs on both sides
    res = torch.randn(B, N, 256, generator=g).to(dt).float()
    w = torch.randn(B, N, 256, generator=g).to(dt).float()
    return qkv, res, w


@pytest.fixture(scope="module")
def ops():
    from medical_tri_modal_pilot_amd import ops as _ops
    return _ops


def _run_case(ops, dt, N, lens, mname, bounded, seed, inflate=None):
    mask = MASKS[mname]
    P, mw = mask.shape[0], words(mask)
    qkv, res, w = inputs(N, 3, dt, seed, inflate)
    kv = None if lens is None else torch.tensor(lens)
    o_ref, g_ref = reference(qkv, kv, mask, w)
    qd, rd, wd = qkv.to(DEV, dt), res.to(DEV, dt), w.to(DEV, dt)
    kvd = None if kv is None else kv.to(DEV, torch.int32)
    kn = ops.key_norms(qd) if bounded else None
    o, o_res, lse = ops.attn_fwd(qd, kvd, res=rd, knorm=kn, qk_mask=mw)
    tag = f"prefix[{str(dt)[6:]},N={N},{mname},{lens}{',bounded' if bounded else ''}]"
    check(tag + ".o", o.float(), o_ref, TOL[dt])
    check(tag + ".o_res", o_res.float(), o_ref.to(dt).float() + res, TOL[dt])
    dqkv = ops.attn_bwd(qd, o, wd, lse, kvd, qk_mask=mw)
    for i, nm in enumerate("qkv"):
        check(f"{tag}.d{nm}", dqkv[..., 256 * i:256 * (i + 1)].float(), g_ref[..., 256 * i:256 * (i + 1)],
              TOL[dt] if dt == torch.float32 else TOL_GRAD_BF16)
    # rows outside the prefix: the plain entries, to the bit
    o0, o_res0, lse0 = ops.attn_fwd(qd, kvd, res=rd, knorm=kn)
    dq0 = ops.attn_bwd(qd, o0, wd, lse0, kvd)[..., :256]
    assert torch.equal(o[:, P:], o0[:, P:]) and torch.equal(o_res[:, P:], o_res0[:, P:]), tag
    assert torch.equal(lse[:, :, P:], lse0[:, :, P:]), tag
    assert torch.equal(dqkv[:, P:, :256], dq0[:, P:]), tag
    return (o, o_ref), (o0, dq0)


CASES = [(20, [16, 17, 20], "v16"), (61, None, "i12"), (140, [12, 13, 140], "t12"), (300, [300, 131, 64], "v16")]


@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("N,lens,mname", CASES)
def test_prefix_attention_fwd_bwd(ops, dt, N, lens, mname, bounded):
    _run_case(ops, dt, N, lens, mname, bounded, seed=11 + N)


@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("N,lens,mname", CASES)
def test_mask_is_applied_where_it_matters(ops, dt, N, lens, mname, bounded):
    """Queries and keys of the prefix share a large common direction (every prefix pair scores ~ +12 before the mask): the result
    still meets the reference's bounds, and the plain entry on the same inputs is far outside them."""
    (o, o_ref), (o0, _) = _run_case(ops, dt, N, lens, mname, bounded, seed=23 + N, inflate=(MASKS[mname].shape[0], 12.0))
    P = MASKS[mname].shape[0]
    assert _rel(o0[:, :P].float(), o_ref[:, :P]) > 10 * TOL[torch.bfloat16]


@pytest.mark.parametrize("dt", DT)
def test_no_prefix_is_the_plain_entry(ops, dt):
    """P = 0 (no words) and an all-zero mask: torch.equal to the plain entries everywhere."""
    qkv, res, w = inputs(140, 3, dt, 5)
    qd, rd, wd = qkv.to(DEV, dt), res.to(DEV, dt), w.to(DEV, dt)
    kvd = torch.tensor([140, 13, 77], dtype=torch.int32, device=DEV)
    kn = ops.key_norms(qd)
    o0, r0, l0 = ops.attn_fwd(qd, kvd, res=rd, knorm=kn)
    d0 = ops.attn_bwd(qd, o0, wd, l0, kvd)
    for mw in ([], [0] * 12):
        o, r, l = ops.attn_fwd(qd, kvd, res=rd, knorm=kn, qk_mask=mw)
        assert torch.equal(o, o0) and torch.equal(r, r0) and torch.equal(l, l0)
        assert torch.equal(ops.attn_bwd(qd, o, wd, l, kvd, qk_mask=mw), d0)


@pytest.mark.parametrize("dt", DT)
def test_grouped_equals_single_launches(ops, dt):
    """Three streams (16-row mask, none, 12-row mask) in one launch: torch.equal to three single launches, both ways."""
    g = torch.Generator().manual_seed(41)
    B, Ns = 3, [300, 61, 140]
    lens = [[300, 131, 64], None, [12, 13, 140]]
    mws = [words(MASKS["v16"]), None, words(MASKS["t12"])]
    qkv = [torch.randn(B, N, 768, generator=g).to(DEV, dt) for N in Ns]
    res = [torch.randn(B, N, 256, generator=g).to(DEV, dt) for N in Ns]
    do = [torch.randn(B, N, 256, generator=g).to(DEV, dt) for N in Ns]
    kv = [None if l is None else torch.tensor(l, dtype=torch.int32, device=DEV) for l in lens]
    kn = [ops.key_norms(q) for q in qkv]
    kn[2] = None                                         # a stream without the table takes the online body
    single = [ops.attn_fwd(q, k, res=r, knorm=t, qk_mask=m) for q, k, r, t, m in zip(qkv, kv, res, kn, mws)]
    o, o_res, lse = ops.attn_fwd_grouped(qkv, kv, res, kn, qk_masks=mws)
    for i in range(3):
        assert torch.equal(o[i], single[i][0]) and torch.equal(o_res[i], single[i][1]) and torch.equal(lse[i], single[i][2]), i
    d1 = [ops.attn_bwd(q, oo, d, l, k, qk_mask=m) for q, oo, d, l, k, m in zip(qkv, o, do, lse, kv, mws)]
    dg = ops.attn_bwd_grouped(qkv, o, do, lse, kv, qk_masks=mws)
    for i in range(3):
        assert torch.equal(d1[i], dg[i]), i
    # the unmasked stream of the masked launch is the plain entry's result
    assert torch.equal(o[1], ops.attn_fwd(qkv[1], kv[1], res=res[1], knorm=kn[1])[0])


def test_long_stream_takes_the_64_key_backward(ops):
    """N >= 1536 in bf16: dK / dV come from the 64-keys-per-wave kernel, which zeroes the masked pairs in its own way."""
    dt, N = torch.bfloat16, 1600
    mask = MASKS["v16"]
    mw = words(mask)
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(1, N, 768, generator=g)
    u = torch.randn(4, 64, generator=g)
    u = (u / u.norm(dim=1, keepdim=True) * math.sqrt(8.0 * 12.0)).reshape(256)
    qkv[:, :16, :256] += u
    qkv[:, :16, 256:512] += u
    qkv = qkv.to(dt).float()
    w = torch.randn(1, N, 256, generator=g).to(dt).float()
    kv = torch.tensor([1500])
    o_ref, g_ref = reference(qkv, kv, mask, w)
    qd, kvd = qkv.to(DEV, dt), kv.to(DEV, torch.int32)
    o, _, lse = ops.attn_fwd(qd, kvd, knorm=ops.key_norms(qd), qk_mask=mw)
    check("prefix64.o", o.float(), o_ref, TOL[dt])
    dqkv = ops.attn_bwd(qd, o, w.to(DEV, dt), lse, kvd, qk_mask=mw)
    for i, nm in enumerate("qkv"):
        check(f"prefix64.d{nm}", dqkv[..., 256 * i:256 * (i + 1)].float(), g_ref[..., 256 * i:256 * (i + 1)], TOL_GRAD_BF16)
    # the prefix keys' own gradient rows, where the masked pairs would land, on their own scale
    for i, nm in ((1, "k"), (2, "v")):
        check(f"prefix64.d{nm}[:16]", dqkv[:, :16, 256 * i:256 * (i + 1)].float(), g_ref[:, :16, 256 * i:256 * (i + 1)], TOL_GRAD_BF16)
