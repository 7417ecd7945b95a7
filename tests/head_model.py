"""Float64 model of the BatchNorm classification head (csrc/head.hip: ops.HeadFn, mtmp_head_fwd / mtmp_head_bwd) and of the
mean-reduced BCE-with-logits loss (mtmp_bce_logits_mean), the inputs of tests/test_head_model_gpu.py and the rule that bounds
them.  Plain torch on the CPU, forward AND backward written out in tensor arithmetic (no nn.Module, no autograd: the per-sample
summands of the row-summed gradients are needed, and tests/test_head_model_cpu.py pins the whole of it to the torch modules in
float64); nothing here imports the HIP library.

    demo = ReLU(LN(age w[:,0] + gender w[:,1] + b))          ie_demo: Linear(2,256), LayerNorm, ReLU
    x    = [LN(cls) | demo]                                  layer_norms_after_concat, cat
    h    = x W1^T + b1 ; y = BatchNorm1d(h) ; a = ReLU(y) ; o = a W2^T + b2

`head_case(B, cls_dt, training, seed, ft)` draws seeded inputs (all fp32-representable, the CLS rows rounded to `cls_dt` first) and
runs the chain in the float type `ft`: torch.float64 is the reference, torch.float32 the same chain in working precision.
The three constants differ on purpose -- LayerNorm eps 1e-5, BatchNorm eps 1e-3, momentum 0.25 -- so that one taken for another shows.

Metric and bound are those of tests/row_kernels_model.py, unchanged:
    err(got, ref) = max |got - ref| / (|ref| + rms(ref)),  bound = max(8 e_torch, 16 * 2^-24) [+ 2^-8 for a bf16 output],
    e_torch = err(this chain in fp32 on the CPU, this chain in float64).  Nothing is fitted to what a kernel returns.

Cancelling sums.  In training mode BatchNorm makes sum_b dh[b][j] = 0, so db1 = sum_b dh and dln_b = sum_b dx_cls are
mathematically zero, and so is ddemo_be[k] = sum_b d demo_pre[b][k] wherever the demo gate of column k is the same for every sample.
Their float64 values are ~1e-16 and |ref| + rms(ref) says nothing; what the kernels must get right is the SUM, so in training mode
these three are held to the size of what is summed: err_sum(got, ref, A) = max |got - ref| / (A + rms(A)) with the per-column
absolute sums A_db1 = sum_b |dh|, A_dln_b = sum_b |dx_cls|, A_ddemo_be = sum_b |d demo_pre| -- for the kernel's error and for
e_torch alike.  A dropped or doubly counted row is then an error of ~1/B, five orders above the bound.

ReLU gates.  A pre-activation that rounds to the other side of 0 in fp32 would fail a gradient without a bug.  The LayerNorm
weights in front of the demo ReLU and the BatchNorm weights in front of the other are drawn as in test_tri_head_gpu._gated
(|g| in [0.1, 0.3], |b| in [0.75, 1.2]: a gate flips where the normalised value passes 2.5 .. 12, so some BatchNorm gates depend on
the sample, the demo gates -- age and gender move a normalised value little -- mostly do not, which makes ddemo_be a cancelling sum
in nearly every live column, and few values come near zero), the model returns the smallest
|pre-activation| of both ReLUs, SEEDS names per batch size the first seed whose margin exceeds GATE_MARGIN for both CLS types and
both modes (find_seeds), and every GPU case asserts that margin from the float64 reference before it compares.  No element is ever
left out of a comparison.

Batch sizes: 63 / 64 / 65, 127 / 128 / 129 and 255 / 256 are the ragged, full and first-of-the-next sizes of the one-, two- and
four-rows-per-lane kernels; 1 has no batch statistics (eval only).  B = 2 and 3 in training mode are ill-conditioned in themselves
-- two-sample BatchNorm outputs are +-1 and dh is a difference close to 0 -- so e_torch of their gradients reaches 5e-4 (ddemo_b at
B = 2) and the rule gives them a loose gradient bound of their own: those sizes are here for the forward pass, the running
statistics and the B / (B - 1) factor of the running variance.
"""
import functools

import torch

from tests import row_kernels_model as R

D, DX = 256, 512
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
LN_EPS, BN_EPS, MOMENTUM = 1e-5, 1e-3, 0.25
GATE_MARGIN = 1e-4
BATCHES = [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256]           # 1: eval only
SEEDS = {1: 0, 2: 0, 3: 0, 4: 0, 5: 0, 63: 0, 64: 0, 65: 0, 127: 0, 128: 0, 129: 0, 255: 0, 256: 0}
#        ie_demo.0.{weight,bias}, ie_demo.1.{weight,bias}, layer_norms_after_concat.{weight,bias}, fc_list.0 / .1 / .3 {weight,bias}
PARAM_NAMES = ["demo_w", "demo_b", "demo_g", "demo_be", "ln_g", "ln_b", "w1", "b1", "bn_g", "bn_b", "w2", "b2"]
GRAD_NAMES = ["d" + n for n in PARAM_NAMES]
CANCELLING = {"db1": "A_db1", "dln_b": "A_dln_b", "ddemo_be": "A_ddemo_be"}
FAULTS = ("drop_last_row", "pad_rows_in_mean", "unbiased_norm", "biased_running_var", "eps_swapped", "momentum_swapped", "gate_ge")


def modes(B):
    return (False,) if B == 1 else (True, False)


# ------------------------------------------------------------------------------------------ inputs
def _gated(gen, n):
    """LayerNorm / BatchNorm weight and bias in front of a ReLU (test_tri_head_gpu._gated)"""
    sign = lambda: (torch.randint(0, 2, (n,), generator=gen) * 2 - 1).double()
    g = (0.1 + 0.2 * torch.rand(n, generator=gen, dtype=F64)) * sign()
    b = (0.75 + 0.45 * torch.rand(n, generator=gen, dtype=F64)) * sign()
    return g.float(), b.float()


def head_inputs(B, cls_dt, seed):
    """fp32 tensors of one case: cls (holding `cls_dt` values), age, gender, w (the loss weights), the twelve parameters and the
    running statistics the call starts from.  The draw does not depend on cls_dt or the mode."""
    gen = torch.Generator().manual_seed(1000 * B + seed)
    r = lambda *s: torch.randn(*s, generator=gen)
    demo_w, demo_b = r(D, 2), 0.5 * r(D)
    demo_g, demo_be = _gated(gen, D)
    ln_g, ln_b = 1 + 0.2 * r(D), 0.2 * r(D)
    w1, b1 = r(D, DX) / DX ** 0.5, 0.1 * r(D)
    bn_g, bn_b = _gated(gen, D)
    w2, b2 = r(1, D) / 16.0, r(1)
    run_mean, run_var = 0.1 * r(D), 0.5 + torch.rand(D, generator=gen)
    cls = R.rnd(1.5 * r(B, D) + 0.3, cls_dt)
    age, gender = torch.rand(B, generator=gen), torch.randint(0, 2, (B,), generator=gen).float()
    w = torch.round(r(B, 1) * 256.0) / 256.0                  # on a 2^-8 grid: db2 = sum_b w is exact in fp32 in any order
    return dict(cls=cls, age=age, gender=gender, w=w, run_mean=run_mean, run_var=run_var,
                params=[demo_w, demo_b, demo_g, demo_be, ln_g, ln_b, w1, b1, bn_g, bn_b, w2, b2])


# ------------------------------------------------------------------------------------------ the chain, forward and backward
def _ln_rows(v, eps):
    """LayerNorm statistics of the rows of v (biased variance, eps inside the root): normalised rows, 1 / std"""
    d = v - v.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt((d * d).mean(1, keepdim=True) + eps)
    return d * rstd, rstd


def _ln_rows_bwd(gy, xh, rstd):
    """gradient of the LayerNorm input from gy = (gradient of the output) * weight"""
    return rstd * (gy - gy.mean(1, keepdim=True) - xh * (gy * xh).mean(1, keepdim=True))


def head_chain(inp, training, *, ft, fault=None, zero_gate=None, ln_eps=LN_EPS, bn_eps=BN_EPS, momentum=MOMENTUM):
    """The head on the tensors of head_inputs() in the float type ft, loss = sum(o * w).  -> logits o [B,1], dcls, the twelve
    parameter gradients (GRAD_NAMES), the running statistics after the call, `margin` and the absolute sums A_* (module docstring).
    zero_gate = (b, j): fc_list.1.bias[j] is set so that the BatchNorm output y[b][j] is exactly 0 (ReLU'(0) = 0, as torch has it).
    fault: one of FAULTS -- the model with a mistake a kernel could make, for tests/test_head_model_cpu.py."""
    assert fault is None or fault in FAULTS, fault
    cls, age, gen, w = (inp[k].to(ft) for k in ("cls", "age", "gender", "w"))
    demo_w, demo_b, demo_g, demo_be, ln_g, ln_b, w1, b1, bn_g, bn_b, w2, b2 = (p.to(ft) for p in inp["params"])
    rm0, rv0 = inp["run_mean"].to(ft), inp["run_var"].to(ft)
    B = cls.shape[0]
    assert B > 1 or not training
    if fault == "eps_swapped":
        ln_eps, bn_eps = bn_eps, ln_eps
    # forward
    u = age[:, None] * demo_w[None, :, 0] + gen[:, None] * demo_w[None, :, 1] + demo_b
    xh_d, rs_d = _ln_rows(u, ln_eps)
    pre_d = xh_d * demo_g + demo_be
    xh_c, rs_c = _ln_rows(cls, ln_eps)
    x = torch.cat([xh_c * ln_g + ln_b, pre_d.clamp_min(0)], 1)
    h = x @ w1.t() + b1
    if training:
        mean = h.mean(0)
        if fault == "pad_rows_in_mean":                      # the rows past B of the lane groups (x = 0 there, so h = b1) counted in
            cap = 64 if B <= 64 else (128 if B <= 128 else 256)
            mean = (h.sum(0) + (cap - B) * b1) / B
        var = ((h - mean) ** 2).mean(0)                       # biased: the one BatchNorm normalises with
        unbiased = var * (B / (B - 1.0))
        m_new, m_old = (1.0 - momentum, momentum) if fault == "momentum_swapped" else (momentum, 1.0 - momentum)
        run_mean = m_old * rm0 + m_new * mean
        run_var = m_old * rv0 + m_new * (var if fault == "biased_running_var" else unbiased)
        if fault == "unbiased_norm":
            var = unbiased
    else:
        mean, var, run_mean, run_var = rm0, rv0, rm0.clone(), rv0.clone()
    rstd = 1.0 / torch.sqrt(var + bn_eps)
    hh = (h - mean) * rstd
    if zero_gate is not None:
        bn_b = bn_b.clone()
        bn_b[zero_gate[1]] = -(hh[zero_gate] * bn_g[zero_gate[1]])
    y = hh * bn_g + bn_b
    a = y.clamp_min(0)
    o = a @ w2.t() + b2
    # backward of sum(o * w)
    do = w
    dw2, db2 = do.t() @ a, do.sum(0)
    dy = (do @ w2) * ((y >= 0) if fault == "gate_ge" else (y > 0)).to(ft)
    dbn_g, dbn_b = (dy * hh).sum(0), dy.sum(0)
    dh = bn_g * rstd * (dy - dbn_b / B - hh * dbn_g / B) if training else bn_g * rstd * dy
    dx = dh @ w1
    dxc, dpre = dx[:, :D], dx[:, D:] * (pre_d > 0).to(ft)
    du = _ln_rows_bwd(dpre * demo_g, xh_d, rs_d)
    dcls = _ln_rows_bwd(dxc * ln_g, xh_c, rs_c)
    keep = slice(0, B - 1) if fault == "drop_last_row" else slice(0, B)          # the rows the sums over the samples take in
    rsum = lambda t: t[keep].sum(0)
    grads = dict(ddemo_w=torch.stack([rsum(du * age[:, None]), rsum(du * gen[:, None])], 1), ddemo_b=rsum(du),
                 ddemo_g=rsum(dpre * xh_d), ddemo_be=rsum(dpre), dln_g=rsum(dxc * xh_c), dln_b=rsum(dxc),
                 dw1=dh.t() @ x, db1=rsum(dh), dbn_g=dbn_g, dbn_b=dbn_b, dw2=dw2, db2=db2)
    margin = min(float(pre_d.abs().min()), float(y.abs().min()))
    return dict(o=o, dcls=dcls, **grads, run_mean=run_mean, run_var=run_var, margin=margin,
                A_db1=dh.abs().sum(0), A_dln_b=dxc.abs().sum(0), A_ddemo_be=dpre.abs().sum(0),
                gate_const=((pre_d > 0) == (pre_d[:1] > 0)).all(0))


def head_case(B, cls_dt, training, seed, ft, **kw):
    return head_chain(head_inputs(B, cls_dt, seed), training, ft=ft, **kw)


# ------------------------------------------------------------------------------------------ metric
def err_sum(got, ref, A):
    """max |got - ref| / (A + rms(A)): a cancelling sum held to the size of its summands (A = their per-column absolute sum, from
    the float64 reference)"""
    got, ref, A = (t.detach().to("cpu", F64).reshape(-1) for t in (got, ref, A))
    assert got.shape == ref.shape == A.shape, (got.shape, ref.shape, A.shape)
    den = A + A.pow(2).mean().sqrt()
    assert float(den.min()) > 0
    q = (got - ref).abs() / den
    return float(torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q).max())


def err_of(name, got, ref_case, training):
    """the error of tensor `name`: err_sum for the three cancelling gradients in training mode, row_kernels_model.err otherwise"""
    if training and name in CANCELLING:
        return err_sum(got, ref_case[name], ref_case[CANCELLING[name]])
    return R.err(got.reshape(ref_case[name].shape), ref_case[name])


CHECKED = ["o", "dcls"] + GRAD_NAMES + ["run_mean", "run_var"]


def e_torch_of(inp, training, **kw):
    """(float64 outputs, {name: e_torch}) of one case"""
    ref, f32 = head_chain(inp, training, ft=F64, **kw), head_chain(inp, training, ft=F32, **kw)
    return ref, {k: err_of(k, f32[k], ref, training) for k in CHECKED}


@functools.lru_cache(maxsize=None)
def case(B, cls_dt, training, seed=None):
    """inputs, float64 reference and e_torch of the case, made once and shared; the tests leave them unchanged"""
    inp = head_inputs(B, cls_dt, SEEDS[B] if seed is None else seed)
    ref, et = e_torch_of(inp, training)
    return dict(inp=inp, ref=ref, e_torch=et)


def find_seeds(limit=200):
    """(CPU, not a test) per batch size the first seed whose gate margin exceeds GATE_MARGIN for both CLS types and both modes"""
    return {B: next(s for s in range(limit) if all(head_case(B, dt, tr, s, F64)["margin"] > GATE_MARGIN
                                                   for dt in (F32, BF16) for tr in modes(B))) for B in BATCHES}


# ------------------------------------------------------------------------------------------ BCE with logits, mean-reduced
BCE_N = [1, 2, 255, 256, 257, 300, 1000]                    # 255 / 256 / 257: the edges of the kernel's 256-stride loop
BCE_PLANTED = [20.0, -20.0, 88.0, -88.0, 89.0, -89.0, 104.0, -104.0, 0.0]   # exp overflows past 88.7, sigmoid saturates


def bce_model(o, t, *, ft):
    """BCEWithLogitsLoss(reduction="mean"): loss = mean(max(o,0) - o t + log(1 + exp(-|o|))), dlogit = (sigmoid(o) - t) / n as
    ((1 - t) sigmoid(o) - t (1 - sigmoid(o))) / n with both factors in their overflow-free form: no cancellation against a target of 1"""
    o, t = o.to(ft), t.to(ft)
    e = torch.exp(-o.abs())
    loss = (o.clamp_min(0) - o * t + torch.log1p(e)).mean()
    big, small = 1.0 / (1.0 + e), e / (1.0 + e)
    sig, one_minus_sig = torch.where(o >= 0, big, small), torch.where(o >= 0, small, big)
    return dict(loss=loss.reshape(1), dlogit=((1.0 - t) * sig - t * one_minus_sig) / o.numel())


@functools.lru_cache(maxsize=None)
def bce_case(n, planted=False):
    """logits 2 randn and 0 / 1 targets; planted: the first 18 (as far as n allows) are BCE_PLANTED with target 0 and with target 1"""
    g = torch.Generator().manual_seed(11000 + n)
    o = 2.0 * torch.randn(n, generator=g)
    t = torch.randint(0, 2, (n,), generator=g).float()
    if planted:
        vals = torch.tensor([v for v in BCE_PLANTED for _ in (0, 1)])[:n]
        o[:len(vals)] = vals
        t[:len(vals)] = torch.tensor([0.0, 1.0] * len(BCE_PLANTED))[:n]
    ref, et = R.e_torch_of(bce_model, o, t)
    return dict(o=o, t=t, ref=ref, e_torch=et)
