"""Float64 references of the row-streaming kernels (csrc/elementwise.hip, the slab reductions of csrc/gemm.hip), the error
metric, the tolerance rule and the inputs of tests/test_row_kernels_gpu.py.  Plain torch on the CPU, written from the
reference's formulas (the lines the kernels' comments cite); nothing here imports the HIP library.

Every model function takes the tensors the kernel takes -- bit for bit, the fp32 LayerNorm `stats` and the fp32-rounded scalars
of AdamW included -- and a float type `ft`: torch.float64 is the reference, torch.float32 the same chain in working precision.
The models round where the kernels round on purpose (the CLS row to the compute type) and nowhere else.

    err(got, ref) = max over elements |got - ref| / (|ref| + rms(ref))                     (float64, element-wise)
    e_torch       = err(fp32 chain, float64 chain)
    bound         = max(8 e_torch, 16 * 2^-24)  [+ 2^-8 for a bf16 output]

The factor 8 allows another summation order and the hardware's 1-ulp reciprocal / rsqrt; the floor is sixteen fp32 round-offs
(every output ends a chain of more than sixteen rounded operations, and e_torch is exactly 0 for some one-row cases); 2^-8 is one
round-to-nearest of an fp32-accurate value to bf16.  Nothing in the bound comes from what a kernel returns.
"""
import functools
import math

import torch
import torch.nn.functional as F

D = 256
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
FLOOR = 16 * 2.0 ** -24
BF16_ROUND = 2.0 ** -8
RELU_MARGIN = 1e-4
RESAMPLE_CAP = 0.10


# ------------------------------------------------------------------------------------------ metric and bound
def err(got, ref):
    """max |got - ref| / (|ref| + rms(ref)) in float64: a small entry is held to its own size plus the tensor's rms, not to the
    largest entry.  Where the denominator is 0 (an all-zero reference) any difference is infinite error."""
    got, ref = got.detach().to("cpu", F64), ref.detach().to("cpu", F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.numel() == 0:
        return 0.0
    den = ref.abs() + ref.pow(2).mean().sqrt()
    diff = (got - ref).abs()
    q = torch.where(den > 0, diff / den.clamp_min(1e-300), torch.where(diff > 0, torch.full_like(diff, math.inf), torch.zeros_like(diff)))
    q = torch.where(torch.isnan(q), torch.full_like(q, math.inf), q)
    return float(q.max())


def bound(e_torch, bf16_out=False):
    return max(8.0 * e_torch, FLOOR) + (BF16_ROUND if bf16_out else 0.0)


def e_torch_of(model, *args, **kw):
    """(float64 outputs, {name: e_torch}) of a model function that takes the float type as the keyword `ft`."""
    ref, f32 = model(*args, ft=F64, **kw), model(*args, ft=F32, **kw)
    return ref, {k: err(f32[k], ref[k]) for k in ref if isinstance(ref[k], torch.Tensor) and ref[k].is_floating_point()}


def rnd(t, dt):
    """the values a tensor of the compute type `dt` holds, as fp32"""
    return t.to(dt).float()


def _leaf(t, ft):
    return t.detach().to(ft).requires_grad_()


# ------------------------------------------------------------------------------------------ custom LayerNorm backward
LN_EPS = 1e-6


def ln_bwd_model(z, stats, gamma, dy, d_res, *, ft):
    """module.py:138-144: y = gamma (z - mu) / (sigma + eps) + beta with the unbiased std and eps outside the root, differentiated by
    autograd at the point the kernel is given: mu and 1/(sigma+eps) take the VALUES of `stats` (fp32 [M,2]), their derivatives are
    autograd's.  dz includes the residual term (encoder.py:24-32)."""
    zr, g, b = _leaf(z, ft), _leaf(gamma, ft), torch.zeros(D, dtype=ft, requires_grad=True)
    mu_a, sd_a = zr.mean(-1, keepdim=True), zr.std(-1, keepdim=True)
    mu = mu_a + (stats[:, :1].to(ft) - mu_a).detach()
    sd = sd_a + (1.0 / stats[:, 1:].to(ft) - LN_EPS - sd_a).detach()
    y = g * ((zr - mu) / (sd + LN_EPS)) + b
    (y * dy.to(ft)).sum().backward()
    dz = zr.grad if d_res is None else zr.grad + d_res.to(ft)
    return dict(dz=dz, dgamma=g.grad, dbeta=b.grad)


def ln_stats(z):
    """the statistics the forward keeps: fp32 (mean, 1 / (unbiased std + eps)) of the compute-type row"""
    zf = z.float()
    return torch.stack([zf.mean(-1), 1.0 / (zf.std(-1) + LN_EPS)], 1).contiguous()


# ------------------------------------------------------------------------------------------ stream input
def sinusoid_table(length, d_model=D):
    """module.py:21-32"""
    pos = torch.arange(0, length, dtype=F32).unsqueeze(1)
    div = torch.exp(torch.arange(0, d_model, 2).float() * -(math.log(10000.0) / d_model))
    pe = torch.zeros(length, d_model)
    pe[:, 0::2] = torch.sin(pos * div)
    pe[:, 1::2] = torch.cos(pos * div)
    return pe


def stream_input_model(x, cls, gamma, beta, pe, bott, w, kv_len=None, keep=None, keep_bwd=None, keep_bott=None, *, dt, ft):
    """mbt_encoder.py:697-729 and the concatenation of :745: z[b] = [bott | drop(LN(cat(CLS.to(dt), x[b])) + pe)], nn.LayerNorm (biased
    variance, eps 1e-5 inside the root).  kv_len (packed form): only the first kv_len[b] rows of sample b exist -- the others carry no
    gradient.  keep (tests/dropout_model.Keep over the [B, N + 1, 256] LayerNorm rows; None = off): y = keep ? y * keep_scale : 0 behind
    LN + PE, in front of the store's one rounding; the bottleneck rows are never masked; autograd gives the backward its g = keep ?
    g * keep_scale : 0 in front of the LayerNorm backward.  keep_bwd / keep_bott exist for the seeded faults only: a backward that
    applies another mask than the forward, and a mask [B, nb, 256] over the bottleneck rows.
    Returns the padded z, the live mask and the gradients of loss = sum(z * w) over live rows."""
    B, N, _ = x.shape
    nb = 0 if bott is None else bott.shape[-2]
    xr, cr, gr, br = _leaf(x, ft), _leaf(cls, ft), _leaf(gamma, ft), _leaf(beta, ft)
    tr = None if bott is None else _leaf(bott, ft)
    c = cr.view(1, 1, D)
    c = c + (c.to(dt).to(ft) - c).detach()                              # the CLS row is rounded to the compute type (its gradient is not)
    y = F.layer_norm(torch.cat([c.expand(B, 1, D), xr], 1), (D,), gr, br, 1e-5)
    if pe is not None:
        y = y + pe[None, :N + 1].to(ft)
    if keep is not None:
        mult = lambda k: torch.where(k.mask, torch.full((), k.scale, dtype=ft), torch.zeros((), dtype=ft))
        y = y * mult(keep) if keep_bwd is None else y * mult(keep_bwd) + (y * mult(keep) - y * mult(keep_bwd)).detach()
    tb = None if tr is None else tr.view(1, nb, D).expand(B, nb, D)
    if keep_bott is not None:
        tb = tb * torch.where(keep_bott.mask, torch.full((), keep_bott.scale, dtype=ft), torch.zeros((), dtype=ft))
    z = y if tb is None else torch.cat([tb, y], 1)
    R = nb + 1 + N
    live = torch.ones(B, R, dtype=torch.bool) if kv_len is None else torch.arange(R)[None, :] < kv_len.long().cpu()[:, None]
    (z * w.to(ft) * live[..., None]).sum().backward()
    out = dict(z=z.detach(), dx=xr.grad, dcls=cr.grad.view(-1), dgamma=gr.grad, dbeta=br.grad)
    if tr is not None:
        out["dbott"] = tr.grad.view(nb, D)
    out["live"] = live
    return out


# ------------------------------------------------------------------------------------------ TIE / time embedding
TIE_NAMES = ("dWv", "dbv", "dgv", "dhv", "dWt", "dbt", "dgt", "dht", "dF")


def _tie_pre(ev, P, chain):
    """pre-ReLU activations of one chain (0 value, 1 time) of events [n,3] = (time, value, feature index): tri_mbt_vsltcls.py:59-71"""
    w, b, g, h = P[4 * chain:4 * chain + 4]
    s = ev[:, 1 - chain].to(w.dtype).unsqueeze(1)
    return F.layer_norm(F.linear(s, w.view(D, 1), b), (D,), g, h, 1e-5)


def _tie_fwd(ev, P, value):
    idx = ev[:, 2].to(torch.int32).long().clamp(0, 19)                     # x[:,:,2].type(IntTensor), :187
    out = torch.relu(_tie_pre(ev, P, 1)) + P[8][idx]
    return out + torch.relu(_tie_pre(ev, P, 0)) if value else out


def tie_model(ev, prm, w, tev=None, w_t=None, value=True, *, ft):
    """tri_mbt_vsltcls.py:183-190: E = ReLU(LN(v w_v + b_v)) + ReLU(LN(tau w_t + b_t)) + F[f] for events ev [n,3]; value=False: the
    time-only embedding of :216-224.  tev [n2,3] (optional): time events embedded with the same parameters (ops.TieTimeEmbed).
    Gradients of loss = sum(E * w) (+ sum(E_time * w_t)) for all nine parameter tensors, in the order of TIE_NAMES."""
    P = [_leaf(p, ft) for p in prm]
    out = _tie_fwd(ev, P, value)
    loss = (out * w.to(ft)).sum()
    res = dict(out=out.detach())
    if tev is not None:
        emb = _tie_fwd(tev, P, False)
        loss = loss + (emb * w_t.to(ft)).sum()
        res["emb"] = emb.detach()
    loss.backward()
    for name, p in zip(TIE_NAMES, P):
        res[name] = torch.zeros_like(p) if p.grad is None else p.grad
    return res


def tie_near_zero(ev, prm, value=True):
    """bool[n]: events with a pre-activation of a chain within RELU_MARGIN of zero in float64 (there the fp32 and the float64
    gradient differ by a whole term, which says nothing about the kernel)"""
    with torch.no_grad():
        P = [p.to(F64) for p in prm]
        bad = (_tie_pre(ev, P, 1).abs() < RELU_MARGIN).any(1)
        if value:
            bad |= (_tie_pre(ev, P, 0).abs() < RELU_MARGIN).any(1)
    return bad


def tie_params(seed):
    """the nine tensors of ie_vslt / ie_time / ie_feat with random values of the trained model's scale"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return [r(D, 1), 0.5 * r(D), 1 + 0.1 * r(D), 0.1 * r(D), 0.2 * r(D, 1), 0.5 * r(D), 1 + 0.1 * r(D), 0.1 * r(D), r(20, D)]


def tie_events(n, prm, seed, value=True, time_ids=False):
    """(events fp32 [n,3], resampled per round): times in (-24, 0], values in [0, 1) -- both through fp16 as the trainer rounds them
    -- and feature indices that cover 0..19 with 0 and 19 present and index 5 used by ONE event (as far as n allows); time_ids: the
    image / text ids 18 | 19 with value 0.  Events with a pre-activation inside the ReLU margin are drawn again until none is
    left; the first round may touch at most RESAMPLE_CAP of them (more means badly chosen parameters)."""
    g = torch.Generator().manual_seed(seed)

    def draw(k):
        e = torch.zeros(k, 3)
        e[:, 0] = (-24 * torch.rand(k, generator=g)).half().float()
        if not time_ids:
            e[:, 1] = torch.rand(k, generator=g).half().float()
        return e

    ev = draw(n)
    if time_ids:
        ev[:, 2] = torch.randint(18, 20, (n,), generator=g).float()
    else:
        idx = torch.randint(0, 19, (n,), generator=g)
        idx = idx + (idx >= 5).long()                                    # 0..19 without 5
        for k, v in enumerate((19, 0, 5)):
            if k < n:
                idx[k] = v
        if n >= 64:
            idx[3:23] = torch.arange(20)
            idx[3 + 5] = 6                                               # (index 5 stays with event 2 alone)
        ev[:, 2] = idx.float()
    rounds = []
    for _ in range(50):
        bad = tie_near_zero(ev, prm, value)
        rounds.append(int(bad.sum()))
        if rounds[-1] == 0:
            break
        assert len(rounds) > 1 or rounds[0] <= RESAMPLE_CAP * n, f"{rounds[0]} of {n} events inside the ReLU margin in the first round"
        ev[bad, :2] = draw(rounds[-1])[:, :2]
    assert rounds[-1] == 0, rounds
    return ev, rounds


# ------------------------------------------------------------------------------------------ column sums, token-group sums
def column_sum_model(slab, *, ft):
    return dict(sum=slab.to(ft).sum(0))


def token_sums_model(dx, L, *, ft):
    """out[j] = sum_{t < L} dx[j L + t]: the gradient of a vector added to every token of its L-token group (tri_mbt_vsltcls.py:216-224)"""
    return dict(sum=dx.to(ft).view(-1, L, D).sum(1))


# ------------------------------------------------------------------------------------------ bottleneck exchange
# mbt_encoder.py:764-779: candidates (mean of the three, mean of vslt + img, mean of vslt + txt, vslt alone) picked by `missing`
EXCHANGE_STREAMS = ((0, 1, 2), (0, 1), (0, 2), (0,))


def exchange_weights(ft):
    w = torch.zeros(4, 3, dtype=ft)
    for p, ms in enumerate(EXCHANGE_STREAMS):
        for m in ms:
            w[p, m] = 1.0 / len(ms)
    return w


def exchange_model(rows, missing, prev, d_rows, d_prev_in, *, ft):
    """rows: the streams' bottleneck rows [B,4,256] (2 or 3 tensors), missing int64[B], prev [B,4,256] | None (resbottle:
    new = mean(new, prev), :778-779).  d_rows: what each consumer sends back for ITS copy of the new tokens, d_prev_in: what the
    next exchange's residual sends back (or None).  -> new tokens, and by autograd the gradients of every stream's rows and of prev."""
    zs = [_leaf(r, ft) for r in rows]
    pv = None if prev is None else _leaf(prev, ft)
    wt = exchange_weights(ft)[missing.long().cpu()]                         # [B,3]
    new = sum(z * wt[:, m, None, None] for m, z in enumerate(zs))
    if pv is not None:
        new = torch.stack([new, pv]).mean(0)
    loss = sum((new * d.to(ft)).sum() for d in d_rows)
    if d_prev_in is not None:
        loss = loss + (new * d_prev_in.to(ft)).sum()
    loss.backward()
    out = dict(new=new.detach())
    for m, z in enumerate(zs):
        out[f"d{m}"] = z.grad
    if pv is not None:
        out["d_prev"] = pv.grad
    return out


# ------------------------------------------------------------------------------------------ AdamW
def f32_scalar(v):
    """the value a C float argument carries"""
    return float(torch.tensor(v, dtype=F32))


def adamw_model(p, g, m, v, lr, beta1, beta2, eps, wd, step, grad_scale, *, ft):
    """torch.optim.AdamW single-tensor math (2_train.py:110) on grad * grad_scale.  The scalars are the fp32 values the kernel's C
    float arguments carry (f32_scalar), used exactly: 1 - beta2 is 1 - fp32(0.999), not fp32(0.001).  `update` is param - old
    param formed without the old parameter's magnitude in the way: -lr wd p - lr / bc1 * m / (sqrt(v / bc2) + eps)."""
    p, g, m, v = (t.to(ft).clone() for t in (p, g, m, v))
    p0 = p.clone()
    g = g * grad_scale
    p.mul_(1.0 - lr * wd)
    m.mul_(beta1).add_(g, alpha=1.0 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1.0 - beta2)
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    denom = (v.sqrt() / math.sqrt(bc2)).add_(eps)
    p.addcdiv_(m, denom, value=-lr / bc1)
    return dict(param=p, exp_avg=m, exp_avg_sq=v, update=p0 * (-(lr * wd)) + (m / denom) * (-lr / bc1))


# ------------------------------------------------------------------------------------------ the cases (inputs + reference, made once)
DTS = (F32, BF16)


def dt_name(dt):
    return "fp32" if dt == F32 else "bf16"


LN_CASES = [(1, "res"), (3, "res"), (17, "res"), (1024, "res"), (1025, "res"), (32787, "res"),
            (1025, "nores"), (1025, "ldz320"), (1025, "ldr264")]


@functools.lru_cache(maxsize=None)
def ln_case(M, variant, dt):
    g = torch.Generator().manual_seed(1000 + M + 7 * len(variant))
    z = rnd(torch.randn(M, D, generator=g) * 2 + 0.3, dt)
    gam = 1 + 0.1 * torch.randn(D, generator=g)
    dy = rnd(torch.randn(M, D, generator=g), dt)
    dres = None if variant == "nores" else rnd(torch.randn(M, D, generator=g), dt)
    stats = ln_stats(z)
    ref, et = e_torch_of(ln_bwd_model, z, stats, gam, dy, dres)
    return dict(z=z, gamma=gam, dy=dy, d_res=dres, stats=stats, ref=ref, e_torch=et)


#                 B, N, nb, sinusoid table
STREAM_CASES = [(1, 1, 0, False), (2, 5, 1, False), (3, 37, 4, True), (7, 146, 4, False), (5, 3400, 4, True)]
STREAM_PACKED = (4, 37, 4, (42, 5, 6, 20))


@functools.lru_cache(maxsize=None)
def stream_case(B, N, nb, use_pe, dt, kv=None):
    g = torch.Generator().manual_seed(2000 + B * 131 + N + nb)
    x = rnd(torch.randn(B, N, D, generator=g) * 1.5 + 0.2, dt)
    cls, gam, bet = torch.randn(1, 1, D, generator=g), 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    bott = torch.randn(1, nb, D, generator=g) if nb else None
    pe = sinusoid_table(N + 1) if use_pe else None
    w = rnd(torch.randn(B, nb + 1 + N, D, generator=g), dt)
    kv_len = None if kv is None else torch.tensor(kv, dtype=torch.int32)
    ref, et = e_torch_of(stream_input_model, x, cls, gam, bet, pe, bott, w, kv_len, dt=dt)
    return dict(x=x, cls=cls, gamma=gam, beta=bet, bott=bott, pe=pe, w=w, kv_len=kv_len, ref=ref, e_torch=et)


TIE_SIZES = [1, 5, 256, 257, 2049, 8197]
TIME_SIZES = [5, 2049]
TIE_PACKED_LENS = (37, 1, 200, 64, 0, 199)
TIE_PACKED_TPAD = 200
#                 n events, n time events, time rows of the first gradient tensor
TIE_TIME_CASES = [(37, 11, 0), (37, 11, 11), (37, 11, 4), (2045, 11, 0), (2045, 11, 11), (2045, 11, 4)]
TIE_PARAM_SEED = 31


@functools.lru_cache(maxsize=None)
def tie_case(n, dt, value=True, n_time=0):
    prm = tie_params(TIE_PARAM_SEED)
    ev, rounds = tie_events(n, prm, 3000 + n, value=value, time_ids=not value)
    g = torch.Generator().manual_seed(4000 + n)
    w = rnd(torch.randn(n, D, generator=g), dt)
    tev = w_t = None
    rounds_t = []
    if n_time:
        tev, rounds_t = tie_events(n_time, prm, 5000 + n, value=False, time_ids=True)
        w_t = rnd(torch.randn(n_time, D, generator=g), dt)
    ref, et = e_torch_of(tie_model, ev, prm, w, tev, w_t, value)
    return dict(ev=ev, prm=prm, w=w, tev=tev, w_t=w_t, rounds=rounds, rounds_t=rounds_t, ref=ref, e_torch=et)


@functools.lru_cache(maxsize=None)
def tie_packed_case(dt):
    """the ragged layout: events back to back, sample b's first lens[b] rows of the padded [B, t_pad, 256] output are its events"""
    lens, T = TIE_PACKED_LENS, TIE_PACKED_TPAD
    prm = tie_params(TIE_PARAM_SEED)
    ev, rounds = tie_events(sum(lens), prm, 3500)
    g = torch.Generator().manual_seed(4500)
    w = rnd(torch.randn(len(lens), T, D, generator=g), dt)
    valid = torch.arange(T)[None, :] < torch.tensor(lens)[:, None]
    cu = torch.tensor([0] + list(lens), dtype=torch.int64).cumsum(0).to(torch.int32)
    ref, et = e_torch_of(tie_model, ev, prm, w[valid], None, None, True)
    return dict(ev=ev, prm=prm, w=w, valid=valid, cu=cu, rounds=rounds, ref=ref, e_torch=et)


REDUCE_ROWS = [1, 3, 63, 64, 255, 256, 257, 2053]
REDUCE_WIDE_COLS = 786432 + 768


@functools.lru_cache(maxsize=None)
def reduce_case(rows, ld, seed=0):
    g = torch.Generator().manual_seed(6000 + rows + ld + seed)
    slab = torch.randn(rows, ld, generator=g) * (2.0 ** torch.randint(-2, 3, (rows, 1), generator=g).float())
    ref, et = e_torch_of(column_sum_model, slab)
    return dict(slab=slab, ref=ref["sum"], e_torch=et["sum"])


TOKEN_L = [1, 4, 5, 8, 9, 49, 128]


@functools.lru_cache(maxsize=None)
def token_case(L, rows, dt):
    g = torch.Generator().manual_seed(7000 + L + rows)
    dx = rnd(torch.randn(rows * L, D, generator=g), dt)
    ref, et = e_torch_of(token_sums_model, dx, L)
    return dict(dx=dx, ref=ref["sum"], e_torch=et["sum"])


EXCHANGE_MISSING = (0, 1, 2, 3, 0)
EXCHANGE_ROWS = [(7, 5, 13), (4, 4, 4)]


@functools.lru_cache(maxsize=None)
def exchange_case(n_rows, resbottle, with_prev_in, two_stream, dt):
    B = len(EXCHANGE_MISSING)
    g = torch.Generator().manual_seed(8000 + sum(n_rows) + 2 * resbottle + with_prev_in + 4 * two_stream)
    ns = n_rows[:2] if two_stream else n_rows
    z = [rnd(torch.randn(B, n, D, generator=g), dt) for n in ns]
    dz = [rnd(torch.randn(B, n, D, generator=g), dt) for n in ns]
    missing = torch.tensor([1, 3, 3, 1, 1] if two_stream else EXCHANGE_MISSING, dtype=torch.int64)
    prev = torch.randn(B, 4, D, generator=g) if resbottle else None
    d_prev_in = torch.randn(B, 4, D, generator=g) if with_prev_in else None
    ref, et = e_torch_of(exchange_model, [t[:, :4] for t in z], missing, prev, [t[:, :4] for t in dz], d_prev_in)
    return dict(z=z, dz=dz, missing=missing, prev=prev, d_prev_in=d_prev_in, ref=ref, e_torch=et)


ADAMW_N = [4, 1020, 2097152 + 1028]
#                step, weight_decay, grad_scale, bf16 shadow
ADAMW_RUNS = [(1, 0.0, 1.0, False), (1000, 0.01, 0.25, True), (1, 0.01, 0.25, True), (1000, 0.0, 1.0, False)]
ADAMW_HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)


@functools.lru_cache(maxsize=None)
def adamw_case(n, step, wd, grad_scale):
    """|param| in [0.02, 2) and sqrt(exp_avg_sq) >= 0.05: the absolute round-off of the new exp_avg (half an ulp of ~0.3), carried
    into the parameter, then stays below the 2 * 2^-24 |param| the parameter check allows for the sum's own rounding."""
    g = torch.Generator().manual_seed(9000 + n % 1000 + step)
    sign = torch.randint(0, 2, (n,), generator=g).float() * 2 - 1
    p = sign * 0.02 * 100.0 ** torch.rand(n, generator=g)
    gr = torch.randn(n, generator=g) / grad_scale
    first = step == 1                                                   # (the moments of a first step are zero)
    m = torch.zeros(n) if first else 0.3 * torch.randn(n, generator=g)
    v = torch.zeros(n) if first else (0.05 + 0.3 * torch.rand(n, generator=g)).pow(2)
    hp = {k: f32_scalar(x) for k, x in ADAMW_HYPER.items()}
    args = (hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], f32_scalar(wd), step, f32_scalar(grad_scale))
    ref, et = e_torch_of(adamw_model, p, gr, m, v, *args)
    return dict(p=p, g=gr, m=m, v=v, args=args, ref=ref, e_torch=et)
