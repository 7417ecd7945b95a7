"""-m gpu: the weight-gradient product dW = dY^T X, db = column sums of dY (ops.gemm_tn -> mtmp_gemm_tn) at the widths of the
trainable image encoder, which are not multiples of 128, and everything that hangs on it: the deferred reduction, the live-row
word, ops.LinearFn, and a whole encoder backward with every library matrix product disabled.

Tolerance: 1e-4 max-norm relative against a float64 product of the same dtype-rounded inputs, in both builds (fp32 accumulation
either way) -- the figure test_gemm_tn_weight_gradient and test_gemm_tn_large_m_dma_tiles hold the 128-multiple kernels to."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-4
DT = [torch.float32, torch.bfloat16]
# (N = dY width, K = X width, rows per image) of the ten weight gradients of the stem, stages 1-2 and patch merging 1
ENCODER = [(96, 16, 3136), (288, 96, 3136), (96, 96, 3136), (384, 96, 3136), (96, 384, 3136), (192, 384, 784),
           (576, 192, 784), (192, 192, 784), (768, 192, 784), (192, 768, 784)]


@pytest.fixture(scope="module")
def ops():
    from medical_tri_modal_pilot_amd import ops as _ops
    return _ops


def _rel(a, b):
    """max |a-b| / (max|b| + tiny): error relative to the tensor's scale"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _check(name, got, ref, tol=TOL):
    e = _rel(got, ref)
    print(f"{name}: rel err {e:.3e} (tol {tol:.1e})")
    assert math.isfinite(e) and e <= tol, f"{name}: rel err {e:.3e} > {tol:.1e}"


def _operands(M, N, K, dt, seed=0, pad=0):
    """dtype-rounded dy [M,N], x [M,K] on the device; pad > 0: column windows [pad : pad + width] of buffers 2 pad wider"""
    g = torch.Generator().manual_seed(1000003 * seed + 31 * M + 7 * N + K)
    wy = torch.randn(M, N + 2 * pad, generator=g).to(dt).to(DEV)
    wx = torch.randn(M, K + 2 * pad, generator=g).to(dt).to(DEV)
    return wy[:, pad:pad + N], wx[:, pad:pad + K]


def _ref(dy, x):
    dy, x = dy.double(), x.double()
    return dy.t() @ x, dy.sum(0)


def _check_product(ops, tag, dy, x, **kw):
    dw, db = ops.gemm_tn(dy, x, **kw)
    rw, rb = _ref(dy, x)
    assert dw.dtype == torch.float32 and db.dtype == torch.float32 and dw.shape == rw.shape and db.shape == rb.shape
    _check(tag + ".dw", dw, rw)
    _check(tag + ".db", db, rb)
    return dw, db


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("N,K,hw", ENCODER)
def test_encoder_widths(ops, dt, N, K, hw):
    dy, x = _operands(3 * hw, N, K, dt)
    _check_product(ops, f"gemm_tn[{str(dt)[6:]},M={3 * hw},N={N},K={K}]", dy, x)


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("M", [1, 7, 63, 130])
@pytest.mark.parametrize("N,K", [(96, 96), (96, 16)])
def test_few_rows(ops, dt, M, N, K):
    dy, x = _operands(M, N, K, dt)
    _check_product(ops, f"gemm_tn[{str(dt)[6:]},M={M},N={N},K={K}]", dy, x)


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("M,N,K", [(200704, 96, 16), (200704, 288, 96), (200704, 96, 384), (50176, 768, 192), (50176, 192, 768)])
def test_sizes_of_64_images_bf16(ops, M, N, K):
    dy, x = _operands(M, N, K, torch.bfloat16)
    dw, db = _check_product(ops, f"gemm_tn[bf16,M={M},N={N},K={K}]", dy, x)
    dw2, db2 = ops.gemm_tn(dy, x)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)          # deterministic (no atomics)


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("N,K", [(96, 96), (192, 384), (576, 192)])
def test_column_windows_of_wider_buffers(ops, dt, N, K):
    dy, x = _operands(3136, N, K, dt, pad=8)
    assert dy.stride(0) == N + 16 and x.stride(0) == K + 16 and not dy.is_contiguous()
    _check_product(ops, f"gemm_tn.window[{str(dt)[6:]},N={N},K={K},ld={dy.stride(0)}]", dy, x)


# ------------------------------------------------------------------ 4
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("N,K", [(8, 8), (40, 104), (136, 264), (128, 96), (96, 128)])
def test_other_widths_inside_the_contract(ops, dt, N, K):
    dy, x = _operands(1000, N, K, dt)
    _check_product(ops, f"gemm_tn[{str(dt)[6:]},M=1000,N={N},K={K}]", dy, x)


@pytest.mark.parametrize("dt", DT)
def test_width_outside_the_contract_raises(ops, dt):
    dy, x = _operands(1000, 100, 96, dt)
    with pytest.raises(RuntimeError, match="mtmp_gemm_tn"):
        ops.gemm_tn(dy, x)


# ------------------------------------------------------------------ 5
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("N,K", [(288, 96), (192, 768)])
def test_deferred_reduction_same_bits(ops, dt, N, K):
    dy, x = _operands(3136, N, K, dt)
    dw, db = ops.gemm_tn(dy, x)
    pending = []
    dw2, db2 = ops.gemm_tn(dy, x, defer=pending)
    assert len(pending) == 1
    ops.reduce_batch(pending)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    out = (torch.full((N, K), float("nan"), device=DEV), torch.full((N,), float("nan"), device=DEV))
    dw3, db3 = ops.gemm_tn(dy, x, out=out)
    assert dw3 is out[0] and db3 is out[1] and torch.equal(dw, dw3) and torch.equal(db, db3)


# ------------------------------------------------------------------ 6
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("r", [1, 1000])
@pytest.mark.parametrize("N,K", [(96, 96), (192, 384)])
def test_live_rows(ops, dt, r, N, K):
    M = 3136
    dy, x = _operands(M, N, K, dt)
    dy, x = dy.clone(), x.clone()
    dy[r:] = float("nan")                                          # a read of a row past the live count shows
    x[r:] = float("nan")
    pack = torch.tensor([0, r], dtype=torch.int32, device=DEV)     # the live count is the element at numel // 2
    dw, db = ops.gemm_tn(dy, x, pack=pack)
    rw, rb = _ref(dy[:r], x[:r])
    t = f"gemm_tn.live[{str(dt)[6:]},N={N},K={K},r={r}]"
    _check(t + ".dw", dw, rw)
    _check(t + ".db", db, rb)


# ------------------------------------------------------------------ 7
def _fsum(t):
    """(sum, sum of squares) of an fp32 tensor in float64, correctly rounded (the squares are exact in float64): no
    dependence on a summation order"""
    v = t.detach().cpu().double().flatten().tolist()
    return math.fsum(v), math.fsum(e * e for e in v)


# Recorded from the commit before the encoder widths were added, on an MI355X, with the inputs of _operands(M, N, K, bf16):
# (M, N, K) -> ((sum dw, sum dw^2), (sum db, sum db^2)) as float.hex
TUNED_BITS = {
    (3456, 768, 256): (("0x1.43198316e4000p+15", "0x1.43d84ad7be384p+29"), ("-0x1.213ae23000000p+10", "0x1.35cd02cf977b1p+21")),
    (64320, 256, 1024): (("-0x1.423fbfa70a000p+17", "0x1.f699b3c9e9ab0p+33"), ("0x1.0d1e49ba00000p+12", "0x1.ac4ae091f7dd3p+23")),
}


@pytest.mark.parametrize("M,N,K", sorted(TUNED_BITS))
def test_128_multiples_keep_their_bits(ops, M, N, K):
    dy, x = _operands(M, N, K, torch.bfloat16)
    dw, db = ops.gemm_tn(dy, x)
    got = tuple(tuple(float(v).hex() for v in _fsum(t)) for t in (dw, db))
    print(f"gemm_tn.bits[M={M},N={N},K={K}]: {got}")
    assert got == TUNED_BITS[(M, N, K)]


# ------------------------------------------------------------------ 8
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_encoder_backward_without_library_products(ops, dtype, monkeypatch):
    from medical_tri_modal_pilot_amd.builder.models.src import swin_transformer as sw

    def banned(name):
        def f(*a, **k):
            raise AssertionError(f"library matrix product {name} on the encoder's training path")
        return f

    torch.manual_seed(5)
    enc = sw.SwinTransformer(compute_dtype=dtype).to(DEV)
    enc.train()
    g = torch.Generator().manual_seed(11)
    img = torch.rand(2, 1, 224, 224, generator=g).to(DEV)
    wgt = torch.randn(2, 7, 7, 768, generator=g).to(DEV)
    for name in ("__matmul__", "__rmatmul__"):
        monkeypatch.setattr(torch.Tensor, name, banned("Tensor." + name))
    for name in ("matmul", "mm", "bmm", "addmm", "einsum"):
        monkeypatch.setattr(torch, name, banned("torch." + name))
    monkeypatch.setattr(torch.nn.functional, "linear", banned("F.linear"))
    feat = enc.forward_train(img)
    (feat.float() * wgt).sum().backward()
    torch.cuda.synchronize()
    grads = {k: p.grad for k, p in enc.named_parameters() if not k.startswith("head.")}
    assert len(grads) == 171
    for k, gr in grads.items():
        assert gr is not None and bool(torch.isfinite(gr).all()), k


# ------------------------------------------------------------------ 9
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("M,N,K,bias", [(3 * 3136, 288, 96, True), (784, 192, 384, False)])
def test_linear_fn_vs_autograd(ops, dt, M, N, K, bias):
    g = torch.Generator().manual_seed(M + N)
    x = torch.randn(M, K, generator=g).to(dt).float()
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(dt).float()
    b = 0.1 * torch.randn(N, generator=g) if bias else None
    up = torch.randn(M, N, generator=g).to(dt).float()            # the upstream gradient, exact in dt
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    br = b.double().requires_grad_() if bias else None
    (torch.nn.functional.linear(xr, wr, br) * up.double()).sum().backward()
    xd = x.to(DEV, dt).requires_grad_()
    wd = w.to(DEV).requires_grad_()
    bd = b.to(DEV).requires_grad_() if bias else None
    y = ops.LinearFn.apply(xd, wd, bd, dt)
    (y.float() * up.to(DEV)).sum().backward()
    t = f"LinearFn[{str(dt)[6:]},M={M},N={N},K={K}]"
    _check(t + ".dw", wd.grad, wr.grad)
    if bias:
        _check(t + ".db", bd.grad, br.grad)
    _check(t + ".dx", xd.grad.float(), xr.grad, 1e-4 if dt == torch.float32 else 3e-2)
