"""Float64 reference of the fused FFN block of csrc/ffn_infer.hip (mtmp_ffn_block, mtmp_ffn_block_grouped), the same chain in
working precision, and the inputs of tests/test_ffn_block_gpu.py.  Plain torch, device-agnostic; nothing here imports the HIP library.

    out[M,256] = x + relu(LN(x) W1^T + c1) W2^T + c2        LN: module.py:138-144 (unbiased std, eps added to the std)

Metric and tolerance rule are the project's (tests/row_kernels_model.py: err, bound):

    err(got, ref) = max over elements |got - ref| / (|ref| + rms(ref))
    bound         = max(8 e_chain, 16 * 2^-24)  [+ 2^-8 for a bf16 output],   e_chain = err(working-precision chain, float64 chain)

ft = float64 is the exact formula, no rounding anywhere.  ft = float32 is the working-precision chain; its rounding points are read
from ffn_block_kernel, not fitted to what it returns:

    F1  LayerNorm as ln_gemm (gemm_model L1, L2): mean and sigma in fp32 from the compute-type row, and
        xn = T(fma(gamma, (x - mean) * rs, beta)) is rounded to the compute type BEFORE the first product (the operand fragments af)
    F2  first product: c1 is the INITIAL accumulator (the sC1 rows copied into hacc at the top of a step), then the 16 k-steps over
        d_model in index order (gemm_model P1, P2) -- ln_gemm_model does exactly this
    F3  h = T(relu(hacc)): the hidden activation is rounded to the compute type as the second product's operand (frag_from_acc)
    F4  second product: accumulators start at ZERO and walk the hidden index in order -- group 0 .. 31, two k-steps of 16 per group
        (bf16; fp32: the f32 matrix instruction's 2-wide steps, whose order inside a 16-wide step differs from the index order: the
        chain is a yardstick of the error's size, not of its bits)
    F5  y = T(acc + c2) is parked in the LDS tile (a rounding point in front of the residual, as gemm_nt's N1 / N2), then
        out = y + x in fp32; the final store to the compute type is not part of the chain (the 2^-8 of the bound)

No element is left out of a check: ReLU is continuous.

`without` = a hidden group g (32 features): the model of a kernel that LOSES that group's contribution (its 32 hidden features are
zero in front of the second product) -- what the one-group probes must be able to tell from the right answer.
"""
import math

import torch

from tests.gemm_model import PROBE_BOUND, PROBE_LOSS, _gen, _mm, _rounder, ln_gemm_inputs, ln_gemm_model  # noqa: F401
from tests.row_kernels_model import BF16, F32, F64, bound, dt_name, err, rnd  # noqa: F401

D, H = 256, 1024
GROUP = 32                                   # hidden features per group of the kernel's walk
N_GROUPS = H // GROUP
DTS = (F32, BF16)


def ffn_block_model(x, gamma, beta, w1, c1, w2, c2, *, dt, ft, without=None):
    """x [M,256], gamma / beta [256], w1 [1024,256], c1 [1024], w2 [256,1024], c2 [256] -> dict(out=[M,256]) in ft"""
    r = _rounder(dt, ft)
    h = r(ln_gemm_model(x, gamma, beta, w1, c1, "relu", dt=dt, ft=ft)["y"])                                   # F1, F2, F3
    if without is not None:
        h = h.clone()
        h[:, GROUP * without:GROUP * (without + 1)] = 0
    y = r(_mm(h, w2, None, dt, ft) + c2.to(ft))                                                               # F4, F5
    return dict(out=y + x.to(ft))


def ffn_inputs(M, dt, seed=0, ldx=D):
    """x, gamma, beta, w1, c1 at the scales of gemm_model.ln_gemm_inputs (N = 1024); w2 ~ 1 / sqrt(1024), c2 ~ 0.3"""
    p = ln_gemm_inputs(M, H, dt, seed=seed, ldx=ldx)
    g = _gen(21, M, seed)
    w2 = rnd(torch.randn(D, H, generator=g) / math.sqrt(H), dt)
    return dict(x=p["x"], gamma=p["gamma"], beta=p["beta"], w1=p["w"], c1=p["bias"], w2=w2, c2=0.3 * torch.randn(D, generator=g))


# ---- one-group probes: the group's c1 is large and positive (it survives the ReLU) and its columns of W2 are scaled by the same gain,
# so the group carries most of the output.  Groups 0 and 31 are the ends of the walk; together with 1, 2 and 3 they sit in every stage of
# the kernel's weight ring for both products (group g: first product from ring buffer g % NST, second from (g + 1) % NST, NST = 4 / 2).
PROBE_GROUPS = (0, 1, 2, 3, 31)
PROBE_GAIN = 32.0
PROBE_M = 130


def probe_inputs(dt, group):
    p = ffn_inputs(PROBE_M, dt, seed=90 + group)
    c1, w2 = p["c1"].clone(), p["w2"].clone()
    sl = slice(GROUP * group, GROUP * (group + 1))
    c1[sl] = PROBE_GAIN * c1[sl].abs().clamp_min(0.05)
    w2[:, sl] *= PROBE_GAIN
    return dict(p, c1=c1, w2=rnd(w2, dt))


def e_chain_of(p, dt, **kw):
    """(float64 out, e_chain) of one set of inputs"""
    ref = ffn_block_model(**p, dt=dt, ft=F64, **kw)["out"]
    return ref, err(ffn_block_model(**p, dt=dt, ft=F32, **kw)["out"], ref)
