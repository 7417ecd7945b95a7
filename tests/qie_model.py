"""Float64 models of the two pieces ``--vslt-type QIE`` changes in TRI_MBT_VSLTCLS (tri_mbt_vsltcls.py:191-198, 216-221, 248-250), the
inputs of tests/test_qie_gpu.py and the rule that bounds them.  Plain torch on the CPU, forward AND backward written out in tensor
arithmetic (no nn.Module, no autograd; tests/test_qie_model_cpu.py pins both to the torch modules in float64); nothing here imports
the HIP library.

The adds (csrc/qie.hip: ops.QieAddsFn, mtmp_qie_adds_fwd / mtmp_qie_adds_bwd):
    demo  = ReLU(LN(age w[:,0] + gender w[:,1] + b))                     ie_demo: Linear(2,256), LayerNorm, ReLU
    add_v = demo ;  add_i = it + demo ;  add_t = tt + demo               one row per sample, added to EVERY token of its stream
    d_it  = sum_j dx_i[b,j] ;  d_tt = sum_j dx_t[b,j]                    for the time-embedding node
    d_demo = sum_t dx_v[b,t] + sum_j dx_i[b,j] + sum_j dx_t[b,j]         never rounded to the streams' type
    (ddemo_w, ddemo_b, ddemo_g, ddemo_be) = ie_demo backward of d_demo, summed over the samples (per-sample summands returned too)
dx_v / dx_i / dx_t are the stream-input node's input gradients: DATA here (values of the streams' type).  Where the rows go --
x[b,t] + add[b] for every token t in FRONT of the stream's LayerNorm, the CLS row without it -- is `stream_rows`.

The 256-wide head (csrc/head.hip at width 256: ops.QieHeadFn):
    x = LN(cls) ;  h = x W1^T + b1, W1 [256,256] ;  y = BatchNorm1d(h) ;  a = ReLU(y) ;  o = a W2^T + b2
tests/head_model.py's chain without the ie_demo half of x; its constants (LayerNorm eps 1e-5, BatchNorm eps 1e-3, momentum 0.25:
different on purpose), its batch sizes and its rule for the two sums BatchNorm makes cancel in training mode (db1, dln_b: held to the
per-column absolute sum of what is summed, head_model.err_sum).

Metric and bound are those of tests/row_kernels_model.py, unchanged:
    err(got, ref) = max |got - ref| / (|ref| + rms(ref)),  bound = max(8 e_torch, 16 * 2^-24) [+ 2^-8 for a bf16 output],
    e_torch = err(this chain in fp32 on the CPU, this chain in float64).  Nothing is fitted to what a kernel returns.

ReLU gates.  The LayerNorm weights in front of the demo ReLU and the BatchNorm weights in front of the head's are drawn as
head_model._gated; both models return the smallest |pre-activation|, SEEDS / HEAD_SEEDS name per batch size the first seed whose
margin exceeds GATE_MARGIN (find_seeds, run on the CPU), and every GPU case asserts that margin from the float64 reference before it
compares.  No element is ever left out of a comparison.
"""
import functools

import torch

from tests import head_model as HM
from tests import row_kernels_model as R

D = 256
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
LN_EPS, BN_EPS, MOMENTUM, GATE_MARGIN = HM.LN_EPS, HM.BN_EPS, HM.MOMENTUM, HM.GATE_MARGIN
N_I, N_T = 49, 128
ADD_BATCHES = [1, 2, 63, 64, 65, 256]
SEEDS = {1: 0, 2: 0, 3: 0, 63: 0, 64: 0, 65: 0, 256: 0}                    # find_seeds(): margin > GATE_MARGIN at seed 0 for every size
HEAD_SEEDS = {B: 0 for B in HM.BATCHES}
ADD_GRADS = ["ddemo_w", "ddemo_b", "ddemo_g", "ddemo_be"]
ADD_CHECKED = ["add_v", "add_i", "add_t", "d_it", "d_tt"] + ADD_GRADS
ADD_FAULTS = ("dx_v_one_short", "dx_i_dropped", "d_demo_bf16", "eps_swapped")
ROW_FAULTS = ("skip_first_token", "add_to_cls", "add_after_ln")
HEAD_PARAMS = ["ln_g", "ln_b", "w1", "b1", "bn_g", "bn_b", "w2", "b2"]
HEAD_GRADS = ["d" + n for n in HEAD_PARAMS]
HEAD_CHECKED = ["o", "dcls"] + HEAD_GRADS + ["run_mean", "run_var"]
HEAD_CANCELLING = {"db1": "A_db1", "dln_b": "A_dln_b"}
HEAD_FAULTS = ("reads_512", "eps_swapped")


# ------------------------------------------------------------------------------------------ the adds
def adds_inputs(B, N_v, dt, seed, with_time=True, kv_live=None, N_i=N_I, N_t=N_T):
    """fp32 tensors of one case: age, gender, the four ie_demo parameters, it / tt and the three stream-input gradients (holding
    values of the streams' type `dt`).  kv_live [B] (optional): a packed vital-sign stream, dx_v's rows from kv_live[b] on are zero."""
    gen = torch.Generator().manual_seed(100 * B + seed)          # the demo chain: what the gate margin of (B, seed) depends on
    r = lambda *s: torch.randn(*s, generator=gen)
    demo_w, demo_b = r(D, 2), 0.5 * r(D)
    demo_g, demo_be = HM._gated(gen, D)
    age, gender = torch.rand(B, generator=gen), torch.randint(0, 2, (B,), generator=gen).float()
    gen = torch.Generator().manual_seed(100000 * N_v + 100 * B + seed + 7)
    it, tt = (R.rnd(r(B, D), dt), R.rnd(r(B, D), dt)) if with_time else (None, None)
    dx_v = R.rnd(0.05 * r(B, N_v, D), dt)
    if kv_live is not None:
        dx_v = dx_v * (torch.arange(N_v).view(1, N_v, 1) < torch.as_tensor(kv_live).view(B, 1, 1))
    dx_i, dx_t = (R.rnd(0.05 * r(B, N_i, D), dt), R.rnd(0.05 * r(B, N_t, D), dt)) if with_time else (None, None)
    return dict(age=age, gender=gender, params=[demo_w, demo_b, demo_g, demo_be], it=it, tt=tt, dx_v=dx_v, dx_i=dx_i, dx_t=dx_t, dt=dt)


def adds_chain(inp, *, ft, fault=None, ln_eps=LN_EPS):
    """The adds on the tensors of adds_inputs() in the float type ft (module docstring).  fault: one of ADD_FAULTS."""
    assert fault is None or fault in ADD_FAULTS, fault
    age, gen = inp["age"].to(ft), inp["gender"].to(ft)
    demo_w, demo_b, demo_g, demo_be = (p.to(ft) for p in inp["params"])
    if fault == "eps_swapped":
        ln_eps = BN_EPS
    u = age[:, None] * demo_w[None, :, 0] + gen[:, None] * demo_w[None, :, 1] + demo_b
    xh, rs = HM._ln_rows(u, ln_eps)
    pre = xh * demo_g + demo_be
    demo = pre.clamp_min(0)
    out = dict(add_v=demo, margin=float(pre.abs().min()))
    dx_v = inp["dx_v"].to(ft)
    d_demo = (dx_v[:, :-1] if fault == "dx_v_one_short" else dx_v).sum(1)
    if inp["it"] is not None:
        dx_i, dx_t = inp["dx_i"].to(ft), inp["dx_t"].to(ft)
        out.update(add_i=inp["it"].to(ft) + demo, add_t=inp["tt"].to(ft) + demo, d_it=dx_i.sum(1), d_tt=dx_t.sum(1))
        d_demo = d_demo + (0 if fault == "dx_i_dropped" else out["d_it"]) + out["d_tt"]
    if fault == "d_demo_bf16":
        d_demo = d_demo.to(BF16).to(ft)
    dpre = d_demo * (pre > 0).to(ft)
    du = HM._ln_rows_bwd(dpre * demo_g, xh, rs)
    per_sample = dict(ddemo_w=torch.stack([du * age[:, None], du * gen[:, None]], 2), ddemo_b=du, ddemo_g=dpre * xh, ddemo_be=dpre)
    out.update({k: v.sum(0) for k, v in per_sample.items()})
    out.update(d_demo=d_demo, per_sample=per_sample)
    return out


def adds_checked(inp):
    return [k for k in ADD_CHECKED if inp["it"] is not None or k not in ("add_i", "add_t", "d_it", "d_tt")]


def adds_e_torch(inp, **kw):
    ref, f32 = adds_chain(inp, ft=F64, **kw), adds_chain(inp, ft=F32, **kw)
    return ref, {k: R.err(f32[k], ref[k]) for k in adds_checked(inp) + ["d_demo"]}


@functools.lru_cache(maxsize=None)
def adds_case(B, N_v, dt, with_time=True, kv_live=None, seed=None):
    """inputs, float64 reference and e_torch of the case, made once and shared; the tests leave them unchanged"""
    inp = adds_inputs(B, N_v, dt, SEEDS.get(B, 0) if seed is None else seed, with_time, None if kv_live is None else list(kv_live))
    ref, et = adds_e_torch(inp)
    return dict(inp=inp, ref=ref, e_torch=et)


def stream_rows(x, add, cls, gamma, beta, *, ft, fault=None, eps=1e-5):
    """rows [B, 1 + N, 256] of the stream-input LayerNorm with an add: LN(cat(CLS, x[b] + add[b])) -- every token t < N, pad rows too,
    the CLS row without it (tri_mbt_vsltcls.py:191-198 adds before the encoder prepends its CLS token).  fault: one of ROW_FAULTS."""
    assert fault is None or fault in ROW_FAULTS, fault
    x, add, cls, gamma, beta = (t.to(ft) for t in (x, add, cls, gamma, beta))
    B = x.shape[0]
    a = add[:, None, :].expand_as(x).clone()
    if fault == "skip_first_token":
        a[:, 0] = 0
    rows = torch.cat([cls.view(1, 1, D).expand(B, 1, D) + (add[:, None, :] if fault == "add_to_cls" else 0),
                      x if fault == "add_after_ln" else x + a], 1)
    xh, _ = HM._ln_rows(rows.reshape(-1, D), eps)
    y = (xh * gamma + beta).view(B, -1, D)
    if fault == "add_after_ln":
        y = torch.cat([y[:, :1], y[:, 1:] + a], 1)
    return y


# ------------------------------------------------------------------------------------------ the 256-wide head
def qhead_inputs(B, cls_dt, seed):
    """fp32 tensors of one case: cls (holding `cls_dt` values), w (the loss weights), the eight parameters and the running statistics"""
    gen = torch.Generator().manual_seed(7000 * B + seed)
    r = lambda *s: torch.randn(*s, generator=gen)
    ln_g, ln_b = 1 + 0.2 * r(D), 0.2 * r(D)
    w1, b1 = r(D, D) / D ** 0.5, 0.1 * r(D)
    bn_g, bn_b = HM._gated(gen, D)
    w2, b2 = r(1, D) / 16.0, r(1)
    run_mean, run_var = 0.1 * r(D), 0.5 + torch.rand(D, generator=gen)
    cls = R.rnd(1.5 * r(B, D) + 0.3, cls_dt)
    w = torch.round(r(B, 1) * 256.0) / 256.0                  # on a 2^-8 grid: db2 = sum_b w is exact in fp32 in any order
    return dict(cls=cls, w=w, run_mean=run_mean, run_var=run_var, params=[ln_g, ln_b, w1, b1, bn_g, bn_b, w2, b2])


def qhead_chain(inp, training, *, ft, fault=None, ln_eps=LN_EPS, bn_eps=BN_EPS, momentum=MOMENTUM):
    """The head on the tensors of qhead_inputs() in the float type ft, loss = sum(o * w) (module docstring).  fault: HEAD_FAULTS."""
    assert fault is None or fault in HEAD_FAULTS, fault
    cls, w = inp["cls"].to(ft), inp["w"].to(ft)
    ln_g, ln_b, w1, b1, bn_g, bn_b, w2, b2 = (p.to(ft) for p in inp["params"])
    rm0, rv0 = inp["run_mean"].to(ft), inp["run_var"].to(ft)
    B = cls.shape[0]
    assert B > 1 or not training
    if fault == "eps_swapped":
        ln_eps, bn_eps = bn_eps, ln_eps
    xh_c, rs_c = HM._ln_rows(cls, ln_eps)
    x = xh_c * ln_g + ln_b
    w1f = w1
    if fault == "reads_512":
        # the 512-wide head's walk on this head's tensors: rows of x and W1 taken with a stride of 512 elements (past the end: from
        # the start again), the second half of each "row" being what lies behind it in memory
        xf, wf = x.reshape(-1), w1.reshape(-1)
        ix = (torch.arange(B)[:, None] * 512 + torch.arange(512)[None, :]) % xf.numel()
        iw = (torch.arange(D)[:, None] * 512 + torch.arange(512)[None, :]) % wf.numel()
        h = xf[ix] @ wf[iw].t() + b1
    else:
        h = x @ w1f.t() + b1
    if training:
        mean = h.mean(0)
        var = ((h - mean) ** 2).mean(0)
        run_mean = (1.0 - momentum) * rm0 + momentum * mean
        run_var = (1.0 - momentum) * rv0 + momentum * var * (B / (B - 1.0))
    else:
        mean, var, run_mean, run_var = rm0, rv0, rm0.clone(), rv0.clone()
    rstd = 1.0 / torch.sqrt(var + bn_eps)
    hh = (h - mean) * rstd
    y = hh * bn_g + bn_b
    a = y.clamp_min(0)
    o = a @ w2.t() + b2
    do = w
    dw2, db2 = do.t() @ a, do.sum(0)
    dy = (do @ w2) * (y > 0).to(ft)
    dbn_g, dbn_b = (dy * hh).sum(0), dy.sum(0)
    dh = bn_g * rstd * (dy - dbn_b / B - hh * dbn_g / B) if training else bn_g * rstd * dy
    dx = dh @ w1
    dcls = HM._ln_rows_bwd(dx * ln_g, xh_c, rs_c)
    return dict(o=o, dcls=dcls, dln_g=(dx * xh_c).sum(0), dln_b=dx.sum(0), dw1=dh.t() @ x, db1=dh.sum(0), dbn_g=dbn_g, dbn_b=dbn_b,
                dw2=dw2, db2=db2, run_mean=run_mean, run_var=run_var, margin=float(y.abs().min()),
                A_db1=dh.abs().sum(0), A_dln_b=dx.abs().sum(0))


def qhead_err(name, got, ref_case, training):
    """the error of tensor `name`: head_model.err_sum for the two cancelling gradients in training mode, row_kernels_model.err otherwise"""
    if training and name in HEAD_CANCELLING:
        return HM.err_sum(got, ref_case[name], ref_case[HEAD_CANCELLING[name]])
    return R.err(got.reshape(ref_case[name].shape), ref_case[name])


def qhead_e_torch(inp, training, **kw):
    ref, f32 = qhead_chain(inp, training, ft=F64, **kw), qhead_chain(inp, training, ft=F32, **kw)
    return ref, {k: qhead_err(k, f32[k], ref, training) for k in HEAD_CHECKED}


@functools.lru_cache(maxsize=None)
def qhead_case(B, cls_dt, training, seed=None):
    inp = qhead_inputs(B, cls_dt, HEAD_SEEDS[B] if seed is None else seed)
    ref, et = qhead_e_torch(inp, training)
    return dict(inp=inp, ref=ref, e_torch=et)


def find_seeds(limit=200):
    """(CPU, not a test) per batch size the first seed whose gate margin exceeds GATE_MARGIN: the adds (the demo gate depends on the
    sample and the parameters only) and the head, both CLS types and both modes"""
    adds = {B: next(s for s in range(limit) if adds_chain(adds_inputs(B, 3, F32, s, False), ft=F64)["margin"] > GATE_MARGIN)
            for B in sorted(SEEDS)}
    head = {B: next(s for s in range(limit) if all(qhead_chain(qhead_inputs(B, dt, s), tr, ft=F64)["margin"] > GATE_MARGIN
                                                   for dt in (F32, BF16) for tr in HM.modes(B))) for B in HM.BATCHES}
    return adds, head
