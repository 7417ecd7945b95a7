"""The R-row LayerNorm head (csrc/headr.hip) and the flexible combine written out in float64, forward AND backward: an explicit
model -- every gradient is a formula below, nothing here calls autograd -- that tests/test_row_head_cpu.py holds to the torch
module chain and tests/test_row_head_gpu.py holds the kernels to.

    v[m]   = ((a + b) + c) / n of head row m's sources (block, row)          a source sum, a missing 1 / n: seeded faults
    x[m]   = [ LN(v[m]) | ReLU(LN(age w0 + gender w1 + b)) ]
    o[m]   = ReLU(LN(x[m] W1^T + b1; g, be)) . w2 + b2                       one parameter set per row, or one shared by all
    p[m,b] = softmax over the PRESENT rows of T a[m], 0 elsewhere;  out[b] = sum_m p o
    d_o    = p g,  d_a[m] = T sum_b p g (o - out)

``fault`` switches one seeded fault on (FAULTS); the tests show that each is far outside the bound the GPU tests use.
Also here: the cases (forms, seeded weights and inputs) both test files share.
"""
import functools
import math

import torch

D = 256
F64 = torch.float64
FAULTS = ("absent_weight", "softmax_all", "no_temperature", "source_sum", "no_div_nsrc", "shared_row0")

# form -> (rows per block, source table, parameter sets): the four heads the models use
FORMS = {
    "r2_shared": ((1, 1), (((0, 0),), ((1, 0),)), 1),                                       # bitxt_ / biimg_mbt_vflexible1
    "r3_shared": ((1, 1, 1), (((0, 0),), ((1, 0),), ((2, 0),)), 1),                         # tri_mbt_vflexible / 2 / 3
    "r4_block": ((4,), (((0, 0),), ((0, 1),), ((0, 2),), ((0, 3),)), 4),                    # tri_mbt_vmultivslt
    "r4_multi2": ((4, 2, 2), (((0, 0), (1, 0), (2, 0)), ((0, 1), (1, 1)), ((0, 2), (2, 1)), ((0, 3),)), 4),   # tri_mbt_vmulti2
    "r2_sparse": ((4, 3), (((0, 1), (1, 2)), ((0, 3),)), 2),                  # no model's: rows 0, 2 of block 0 and 0, 1 of block 1 feed nothing
}
SMALL_SCALE = 4e-3          # block rows with a variance near LayerNorm's eps (case())
TRI_PRESENT = ((True, True, True), (True, True, False), (True, False, True), (True, False, False))
BI_PRESENT = ((True, True), (True, False), (True, False), (True, False))


def _ln(v, eps=1e-5):
    mean = v.mean(-1, keepdim=True)
    d = v - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)
    return d * rstd, rstd


def _ln_bwd(gy, xh, rstd):
    return rstd * (gy - gy.mean(-1, keepdim=True) - xh * (gy * xh).mean(-1, keepdim=True))


def head_forward(blocks, table, age, gender, params, fault=None):
    """blocks: list of [B, P, 256]; params: 6 shared + 6 per set (1 or R sets), float64.  Returns the cache head_backward reads;
    cache["o"] = logits [R, B], cache["margin"] = the smallest |pre-activation| of the two ReLUs."""
    R, n_sets = len(table), (len(params) - 6) // 6
    dw, db, dg, dbe, lg, lb = params[:6]
    u = age[:, None] * dw[:, 0] + gender[:, None] * dw[:, 1] + db
    uh, rstd_u = _ln(u)
    dpre = uh * dg + dbe
    demo = dpre.clamp(min=0)
    rows, o, margin = [], [], float(dpre.abs().min())
    for m, srcs in enumerate(table):
        v = blocks[srcs[0][0]][:, srcs[0][1]]
        for s, r in srcs[1:]:
            v = v + blocks[s][:, r]
        if fault != "source_sum":
            v = v / len(srcs)
        ch, rstd_c = _ln(v)
        x = torch.cat([ch * lg + lb, demo], dim=1)
        k = 6 + (6 * m if n_sets > 1 else 0)
        w1, b1, g, be, w2, b2 = params[k:k + 6]
        hh, rstd_h = _ln(x @ w1.t() + b1)
        pre = hh * g + be
        o.append(pre.clamp(min=0) @ w2.reshape(-1) + b2.reshape(()))
        margin = min(margin, float(pre.abs().min()))
        rows.append(dict(ch=ch, rstd_c=rstd_c, x=x, hh=hh, rstd_h=rstd_h, pre=pre))
    return dict(o=torch.stack(o), rows=rows, uh=uh, rstd_u=rstd_u, dpre=dpre, table=table, shapes=[b.shape for b in blocks],
                age=age, gender=gender, params=params, margin=margin)


def head_backward(c, d_o, fault=None):
    """(gradient blocks, parameter gradients in the order of params) for the upstream gradient d_o [R, B]"""
    params, table = c["params"], c["table"]
    R, n_sets = len(table), (len(params) - 6) // 6
    lg = params[4]
    dblocks = [torch.zeros(s, dtype=F64) for s in c["shapes"]]
    grads = [torch.zeros_like(p) for p in params]
    ddemo = torch.zeros_like(c["uh"])
    for m, (srcs, row) in enumerate(zip(table, c["rows"])):
        k = 6 + (6 * m if n_sets > 1 else 0)
        w1, b1, g, be, w2, b2 = params[k:k + 6]
        dl = d_o[m]
        dy = dl[:, None] * w2.reshape(1, -1) * (row["pre"] > 0)
        dh = _ln_bwd(dy * g, row["hh"], row["rstd_h"])
        dx = dh @ w1
        if not (fault == "shared_row0" and n_sets == 1 and m > 0):
            grads[k] += dh.t() @ row["x"]
            grads[k + 1] += dh.sum(0)
            grads[k + 2] += (dy * row["hh"]).sum(0)
            grads[k + 3] += dy.sum(0)
            grads[k + 4] += (dl[:, None] * row["pre"].clamp(min=0)).sum(0).reshape(w2.shape)
            grads[k + 5] += dl.sum().reshape(b2.shape)
        dc = dx[:, :D]
        ddemo = ddemo + dx[:, D:]
        grads[4] += (dc * row["ch"]).sum(0)
        grads[5] += dc.sum(0)
        dv = _ln_bwd(dc * lg, row["ch"], row["rstd_c"])
        if fault != "no_div_nsrc":
            dv = dv / len(srcs)
        for s, r in srcs:
            dblocks[s][:, r] = dv
    dyd = ddemo * (c["dpre"] > 0)
    grads[2] += (dyd * c["uh"]).sum(0)
    grads[3] += dyd.sum(0)
    du = _ln_bwd(dyd * params[2], c["uh"], c["rstd_u"])
    grads[0] += torch.stack([du.t() @ c["age"], du.t() @ c["gender"]], dim=1)
    grads[1] += du.sum(0)
    return dblocks, grads


def _present(ids, table, R):
    tab = torch.tensor([[bool(table[p][r]) for r in range(R)] for p in range(4)])
    return tab[ids.long() & 3].t()                                                            # [R, B]


def flex_forward(o, a, T, ids, table, fault=None):
    """(out [B], p [R, B]) of logits o [R, B], weights a [R], pattern ids [B] and present[pattern][row]"""
    R = o.shape[0]
    on = _present(ids, table, R)
    if fault == "softmax_all":
        on = torch.ones_like(on)
    z = (T * a.reshape(R, 1)).expand(R, o.shape[1])
    e = torch.where(on, torch.exp(z - torch.where(on, z, torch.full_like(z, -math.inf)).max(0, keepdim=True).values), torch.zeros_like(z))
    p = e / e.sum(0, keepdim=True)
    if fault == "absent_weight":
        p = torch.where(on, p, torch.full_like(p, 0.05))
    return (p * o).sum(0), p


def flex_backward(o, a, T, ids, table, g, fault=None):
    """(d_o [R, B], d_a [R], the absolute sum sum_b |summand| of d_a [R])"""
    out, p = flex_forward(o, a, T, ids, table, fault)
    terms = (1.0 if fault == "no_temperature" else T) * p * g * (o - out)
    return p * g, terms.sum(1), terms.abs().sum(1)


def flex_da_terms(o, a, T, ids, table, g):
    """sum_b T p |g| (|o| + |out|) [R]: the magnitude of what a softmax backward subtracts to get d a.  Autograd of the
    reference's chain forms d a from p * (g o) and p * sum_j p (g o) separately, so ITS rounding error scales with this -- not
    with the summands of the closed form, which are small where one weight is close to 1 -- and the float64 comparison of the
    model with that chain is made against it."""
    out, p = flex_forward(o, a, T, ids, table)
    return (T * p * g.abs() * (o.abs() + out.abs())).sum(1)


# ---- the cases the CPU and GPU tests share -------------------------------------------------------------------------------------
def _gated(gen, n):
    """LayerNorm weight / bias in front of a ReLU, drawn as in tests/test_tri_head_gpu.py: |g| in [0.1, 0.3], |b| in [0.75, 1.2]"""
    sign = lambda: (torch.randint(0, 2, (n,), generator=gen) * 2 - 1).double()
    g = (0.1 + 0.2 * torch.rand(n, generator=gen, dtype=F64)) * sign()
    b = (0.75 + 0.45 * torch.rand(n, generator=gen, dtype=F64)) * sign()
    return g, b


def make_params(gen, n_sets):
    """float64: ie_demo.0.{weight,bias}, ie_demo.1.{weight,bias}, layer_norms_after_concat.{weight,bias}, then n_sets heads"""
    Rn = lambda *s: torch.randn(*s, generator=gen, dtype=F64)
    g, b = _gated(gen, D)
    prm = [Rn(D, 2), 0.5 * Rn(D), g, b, 1 + 0.2 * Rn(D), 0.2 * Rn(D)]
    for _ in range(n_sets):
        g, b = _gated(gen, D)
        prm += [Rn(D, 2 * D) / math.sqrt(2.0 * D), 0.1 * Rn(D), g, b, Rn(1, D) / 16.0, Rn(1)]
    return prm


@functools.lru_cache(maxsize=None)
def case(form, B, dt=torch.float32, seed=0, n_sets=None, scale=1.5):
    """One seeded case, computed once and shared, never modified: inputs (the blocks rounded to ``dt``), float64 parameters and
    the model's results for the upstream gradient w.  ``scale``: the spread of the block rows.  LayerNorm removes the scale of its
    input but for eps, so at the encoder's O(1) rows a source SUM in place of the mean changes nothing measurable; SMALL_SCALE
    puts the rows' variance at the size of eps (1e-5), where the two differ by a factor of about 1.5."""
    P, table, sets = FORMS[form]
    sets = sets if n_sets is None else n_sets
    gen = torch.Generator().manual_seed(100000 * (sorted(FORMS).index(form) + 1) + 1000 * B + seed)
    params = make_params(gen, sets)
    blocks = [(scale * torch.randn(B, p, D, generator=gen) + 0.2 * scale).to(dt).float() for p in P]
    age, gender = torch.rand(B, generator=gen), torch.randint(0, 2, (B,), generator=gen).float()
    w = torch.randn(len(table), B, generator=gen)
    c = head_forward([b.double() for b in blocks], table, age.double(), gender.double(), params)
    dblocks, grads = head_backward(c, w.double())
    return dict(form=form, B=B, P=P, table=table, n_sets=sets, blocks=blocks, age=age, gender=gender, w=w, params=params, o=c["o"],
                dblocks=dblocks, grads=grads, margin=c["margin"], cache=c)


def rel(a, b):
    """max |a - b| / (max |b| + tiny): error relative to the tensor's scale (tests/test_gpu_parity.py)"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def mixed_ids(B, lo=0, hi=4, seed=3):
    """pattern ids in [lo, hi), every one present when B allows"""
    ids = torch.randint(lo, hi, (B,), generator=torch.Generator().manual_seed(seed))
    ids[: min(B, hi - lo)] = torch.arange(lo, lo + min(B, hi - lo))
    return ids


def reference_flex_chain(o, a, T, ids, R):
    """the reference's chain (tri_mbt_vflexible.py:276-286, bitxt_mbt_vflexible1.py:184-192) in o's dtype: masked_fill(-1e9),
    softmax, the candidate sums, gather.  ids in [0, 4) for R = 3, [0, 2) for R = 2."""
    B = o.shape[1]
    absent = ~torch.tensor([list(r) for r in (TRI_PRESENT if R == 3 else BI_PRESENT[:2])])
    w = a.reshape(R, 1).repeat(1, B).masked_fill(absent[ids.long()].permute(1, 0), -1e9)
    po = o * torch.softmax(w * T, dim=0)
    cands = torch.stack([po.sum(0), po[0] + po[1], po[0] + po[2], po[0]]) if R == 3 else torch.stack([po[0] + po[1], po[0]])
    return cands[ids.long(), torch.arange(B)]


def flex_case(R, B, T, seed=0):
    """(o, a, ids, g) fp32 CPU tensors: ids 0 .. 7 (read as id & 3) for R = 3; 0, 1, 4, 5 (patterns 0 and 1) for R = 2"""
    gen = torch.Generator().manual_seed(7000 + 100 * R + B + seed)
    o, a, g = 2.0 * torch.randn(R, B, generator=gen), 0.7 * torch.randn(R, generator=gen), torch.randn(B, generator=gen)
    ids = mixed_ids(B, 0, 8, seed=B)
    if R == 2:
        ids = (ids & 1) | (ids & 4)
    return o, a, ids, g


def flex_reference(R, B, T, seed=0):
    """float64 model results and e_torch: the error of the reference's chain run by torch in fp32 on the CPU against float64,
    relative to scale, for out and d_o (the head rule: the GPU is held to max(8 e_torch, 16 * 2^-24))"""
    o, a, ids, g = flex_case(R, B, T, seed)
    table = TRI_PRESENT if R == 3 else BI_PRESENT
    out, _ = flex_forward(o.double(), a.double(), T, ids, table)
    d_o, d_a, d_a_abs = flex_backward(o.double(), a.double(), T, ids, table, g.double())
    o32 = o.clone().requires_grad_()
    out32 = reference_flex_chain(o32, a, T, ids & 3, R)
    (do32,) = torch.autograd.grad((out32 * g).sum(), o32)
    e = max(rel(out32, out), rel(do32, d_o))
    return dict(o=o, a=a, ids=ids, g=g, table=table, out=out, d_o=d_o, d_a=d_a, d_a_abs=d_a_abs, bound=max(8 * e, 16 * 2.0 ** -24))
