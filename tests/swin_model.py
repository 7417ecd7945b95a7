"""Float64 references of the Swin image-encoder kernels (csrc/swin.hip, csrc/swin_bwd.hip, csrc/stem.hip) as the C entry points define
them, the same chains in working precision, and the inputs, case tables and probes of tests/test_swin_model_gpu.py.  Plain torch,
device-agnostic (a model runs where its tensors live); nothing here imports the HIP library or any project code for the math: the
formulas are the reference's (builder/models/src/swin_transformer.py, the lines the kernels' comments cite).  Metric and tolerance
rule are those of tests/row_kernels_model.py:

    err(got, ref) = max over elements |got - ref| / (|ref| + rms(ref))     over ONE output tensor of a launch, live rows only
    bound         = max(8 e_chain, 16 * 2^-24)  [+ 2^-8 for a bf16 output],   e_chain = err(working-precision chain, float64 chain)

Every model takes the tensors the entry point takes (operands already rounded to the compute type dt; LayerNorm parameters, biases,
row_scale and the relative-position table in fp32) and a float type ft.  ft = float64 is the reference: the exact operation.
ft = float32 is the yardstick chain: the same formulas in fp32, in the kernels' accumulation steps, and for dt = bfloat16 a rounding
to bf16 where the kernels round on purpose -- read from the sources, not fitted to what the kernels return:

  every product
    P1  the matrix instruction walks the contraction index in k-steps of 16 (bf16) or 2 (fp32) and rounds the running fp32 sum
        after each (gemm_model._mm / _bmm here)
  layernorm_rows (swin.hip ln_rows_kernel), layernorm_rows_bwd (swin_bwd.hip ln_rows_bwd_kernel)
    R1  mean = sum / C, then sum (x - mean)^2 / C, rstd = rsqrt(. + eps), y = fma((x - mean) rstd, w, b): fp32 throughout, no
        rounding point; merge mode gathers x[0::2,0::2], x[1::2,0::2], x[0::2,1::2], x[1::2,1::2] (src[0..3])
    R2  backward, the comment above the kernel: xh = (x - mean) rstd, g = dy w, dx = rstd (g - mean(g) - xh mean(g xh)),
        dw = sum dy xh, db = sum dy; fp32, no rounding point
  gelu (swin_bwd.hip gelu_kernel, gelu_grad<T>; common.hip.h gelu<T>)
    E1  fp32: 0.5 x (1 + erf(x / sqrt 2)) and cdf + x pdf; bf16: x sigmoid(2 z), 2 z = x (1.5957691216 + 0.0713548163 x^2), and
        sig + x sig (1 - sig) (1.5957691216 + 3 * 0.0713548163 x^2).  The reference is always the exact GELU
  window attention (swin.hip swin_wattn_kernel, swin_bwd.hip swin_wattn_bwd_kernel)
    A1  the additive table is read in the compute type (`const T* table`): its values T(bias + mask) are operands
    A2  a pad token's q / k / v are T(qkv_bias) (frag_bias<T>): operands as well
    A3  s = fma(K Q^T, scale, table) on the unscaled q; p = exp(s - max) unnormalised, l = sum p of the UNROUNDED p;
        P is rounded when it becomes the operand of P V (frag_from_acc<T>(st)); the product is multiplied by 1 / l at the store
    A4  backward pass 1: p *= 1 / l; dP = V dO^T; delta = sum p dP; dS = p (dP - delta); dtab += dS in fp32 (atomicAdd, unrounded);
        dS is rounded as the operand of dQ = K^T dS (frag_from_acc<T>), `scale` multiplies the product at the store
    A5  backward pass 2: lse = max + ln l; p2 = exp(s - lse) is rounded as the operand of dV = dO^T p2; dS2 = p2 (dP - delta) (from
        the unrounded p2) is rounded as the operand of dK = Q^T dS2, `scale` at the store
    A6  dbias[C..3C) adds the fp32 accumulators dk * scale / dv of the pad keys (before any store); dbias[0..C) is never written
  attention block (swin.hip swin_attn_block_kernel; bf16 only)
    B1  xn = T(LN(x)) into the LDS tile (frag_store<bf16>(sX ..)); pad tokens and window-pad slots are zero rows (frag_keep)
    B2  q, k, v = T(bias + W xn): the bias is the accumulators' initial value, frag_from_acc<bf16> rounds them
    B3  the heads' outputs o / l are stored to the LDS tile as bf16 (store4<bf16>(po ..))
    B4  the projection starts from bproj; round_as<bf16>(round_as<bf16>(acc) * sc) + x
  swin_mlp (swin.hip swin_mlp_kernel; bf16 only)
    M1  xn = T(LN(x)) (af[c] = from_f32<bf16>(..)); h = T(gelu_bf16(b1 + W1 xn)) (h starts from the bias block; frag_from_acc<bf16>)
    M2  acc2 from zero over the hidden index in order, 16 per step; T(acc2 + b2) through the staging tile (store4<bf16>(sS ..)),
        then * row_scale[row / rows_per_scale], round_as<bf16>(.) + x
  swin_ln_linear (swin.hip swin_ln_linear_kernel; bf16 only)
    N1  xn = T(LN(x)); acc starts from the bias
  stem (stem.hip stem_kernel)
    S1  pixels and conv weights are converted to the compute type for the product (frag_from_f32<T>): one k-step of 16 (bf16) or
        eight of 2 (fp32); the bias is added to the fp32 accumulators; two-pass LayerNorm on them, eps 1e-5

The final store of an output to bf16 is NOT part of the chain: that is the 2^-8 of the bound.
"""
import functools
import math

import torch

from tests import gemm_model as G
from tests.gemm_model import _kstep, _mm, _rounder, e_chain_of  # noqa: F401
from tests.row_kernels_model import BF16, BF16_ROUND, F32, F64, FLOOR, bound, dt_name, err, rnd  # noqa: F401

DTS = (F32, BF16)
WS, L = 7, 49
DH = 32
EPS = 1e-5
PAD_LOGIT = -30000.0
PROBE_BOUND, PROBE_LOSS = 0.25, 0.5


# ------------------------------------------------------------------------------------------ LayerNorm over rows
def _ln(x, w, b, eps):
    """R1 (x already in ft)"""
    C = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / C
    d = x - mean
    rstd = 1.0 / ((d * d).sum(-1, keepdim=True) / C + eps).sqrt()
    return d * rstd * w.to(x.dtype) + b.to(x.dtype), d * rstd, rstd


def merge_gather(x):
    """[n,H,W,Cs] -> [n,H/2,W/2,4Cs]: swin_transformer.py:40-44"""
    return torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1)


def ln_rows_model(x, w, b, eps=EPS, merge_hw=None, *, dt, ft):
    x = x.to(ft)
    if merge_hw is not None:
        assert tuple(x.shape[1:3]) == tuple(merge_hw)
        x = merge_gather(x)
    return dict(y=_ln(x, w, b, eps)[0])


def ln_rows_bwd_model(x, w, dy, eps=EPS, keep=None, *, dt, ft):
    """R2.  keep = (lo, hi): only the rows [lo, hi) add to dw / db -- what is left of them when every other row's term is lost"""
    x, dy = x.to(ft).reshape(-1, x.shape[-1]), dy.to(ft).reshape(-1, x.shape[-1])
    _, xh, rstd = _ln(x, torch.ones_like(w), torch.zeros_like(w), eps)
    g = dy * w.to(ft)
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    if keep is not None:
        dy, xh = dy[keep[0]:keep[1]], xh[keep[0]:keep[1]]
    return dict(dx=dx, dw=(dy * xh).sum(0), db=dy.sum(0))


# ------------------------------------------------------------------------------------------ GELU
def gelu_model(x, *, dt, ft):
    return dict(y=G.gelu_model(x.to(ft), dt, ft))


def gelu_grad_model(x, dy, *, dt, ft):
    """E1"""
    x, dy = x.to(ft), dy.to(ft)
    if ft == F32 and dt == BF16:
        x2 = x * x
        sig = torch.sigmoid(x * (x2 * 0.0713548163 + 1.5957691216))
        return dict(dx=dy * (sig + x * sig * (1.0 - sig) * (x2 * (3.0 * 0.0713548163) + 1.5957691216)))
    cdf = 0.5 * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))
    return dict(dx=dy * (cdf + x * torch.exp(-0.5 * x * x) * (1.0 / math.sqrt(2.0 * math.pi))))


# ------------------------------------------------------------------------------------------ window geometry (the reference's rules)
def rel_index():
    """swin_transformer.py:47-55 / torchvision's relative_position_index: [49 * 49] rows of the (2 ws - 1)^2 table"""
    ax = torch.arange(WS)
    c = torch.stack(torch.meshgrid(ax, ax, indexing="ij")).flatten(1)
    rel = c[:, :, None] - c[:, None, :]
    return ((rel[0] + WS - 1) * (2 * WS - 1) + rel[1] + WS - 1).flatten()


@functools.lru_cache(maxsize=None)
def window_geometry(H, W, shift):
    """swin_transformer.py:150-169, :190-203 -> pix int64 [nW,49]: the flat index y W + x on the UN-padded map of every token of
    every window of the padded, rolled map (-1: a pad token); mask [nW,49,49] of 0 / -100; (shift_h, shift_w) after :155-160"""
    Hp, Wp = -(-H // WS) * WS, -(-W // WS) * WS
    sh, sw = (0 if WS >= Hp else shift), (0 if WS >= Wp else shift)
    pm = torch.full((Hp, Wp), -1, dtype=torch.int64)
    pm[:H, :W] = torch.arange(H * W).view(H, W)
    if sh + sw > 0:
        pm = torch.roll(pm, shifts=(-sh, -sw), dims=(0, 1))
    nWh, nWw = Hp // WS, Wp // WS
    pix = pm.view(nWh, WS, nWw, WS).permute(0, 2, 1, 3).reshape(nWh * nWw, L)
    mask = torch.zeros(nWh * nWw, L, L)
    if sh + sw > 0:
        reg = torch.zeros(Hp, Wp)
        count = 0
        for h in ((0, -WS), (-WS, -sh), (-sh, None)):
            for w in ((0, -WS), (-WS, -sw), (-sw, None)):
                reg[h[0]:h[1], w[0]:w[1]] = count
                count += 1
        reg = reg.view(nWh, WS, nWw, WS).permute(0, 2, 1, 3).reshape(nWh * nWw, L)
        diff = reg.unsqueeze(1) - reg.unsqueeze(2)
        mask = torch.where(diff != 0, torch.full_like(diff, -100.0), torch.zeros_like(diff))
    return pix, mask, (sh, sw)


@functools.lru_cache(maxsize=None)
def window_types(H, W, shift):
    """int64 [nW]: which of the four masks of a 2 x 2-window map (interior, last column, last row, corner) a window carries -- found
    by comparing the masks themselves, not by the window's position"""
    _, mask, s = window_geometry(H, W, shift)
    if sum(s) == 0:
        return torch.zeros(mask.shape[0], dtype=torch.int64)
    canon = window_geometry(2 * WS, 2 * WS, shift)[1]
    out = []
    for m in mask:
        hit = [t for t in range(4) if torch.equal(m, canon[t])]
        if not hit:
            raise ValueError(f"a window of the {H} x {W} map at shift {shift} has none of the four table masks")
        out.append(hit[0])
    return torch.tensor(out, dtype=torch.int64)


def rel_bias(rpb, heads):
    """relative_position_bias_table [169, heads] fp32 -> [heads,49,49]"""
    return rpb.float().cpu()[rel_index()].view(L, L, heads).permute(2, 0, 1)


def table_model(rpb, heads, shift, dt, acc_order=False):
    """the [4][heads][64][64] table the entries take, values of the compute type as fp32 (A1): bias + the mask of the four window
    types, PAD_LOGIT on the 15 pad-slot keys; acc_order (mtmp.h, mtmp_swin_attn_block): position 8 h + j of 16-key group g holds key
    16 g + (j & 3) + 8 (j >> 2) + 4 h"""
    tab = torch.zeros(4, heads, 64, 64)
    tab[..., L:] = PAD_LOGIT
    tab[:, :, :L, :L] = rel_bias(rpb, heads)
    if shift > 0:
        tab[:, :, :L, :L] += window_geometry(2 * WS, 2 * WS, shift)[1].unsqueeze(1)
    if acc_order:
        src = [16 * g + (j & 3) + 8 * (j >> 2) + 4 * h for g in range(4) for h in range(2) for j in range(8)]
        tab = tab[..., torch.tensor(src)]
    return rnd(tab, dt)


def scatter_dtab(dtab, heads):
    """the gradient of relative_position_bias_table [169, heads] from dtab [4,heads,64,64]: the transpose of rel_bias' gather"""
    d = dtab.detach().to("cpu", F64)[:, :, :L, :L].sum(0).permute(1, 2, 0).reshape(L * L, heads)
    return torch.zeros((2 * WS - 1) ** 2, heads, dtype=F64).index_add_(0, rel_index(), d)


# ------------------------------------------------------------------------------------------ window attention
def _bmm(a, b, dt, ft):
    """a b^T over the last index (a [..,M,K], b [..,N,K]) as the matrix pipe forms it (P1); float64: the plain product"""
    bt = b.transpose(-1, -2)
    if ft == F64:
        return a @ bt
    acc, s = None, _kstep(dt)
    for k in range(0, a.shape[-1], s):
        t = a[..., k:k + s] @ bt[..., k:k + s, :]
        acc = t if acc is None else acc + t
    return acc


def _attn_core(qkv, pad, rpb, heads, shift, d_out, dt, ft):
    """qkv [n,H,W,3C] in ft; pad [3C] in ft: the pad tokens' q | k | v (None: the map must be whole windows)"""
    r = _rounder(dt, ft)
    dev = qkv.device
    n, H, W, C3 = qkv.shape
    C = C3 // 3
    dh = C // heads
    scale = dh ** -0.5
    pix, mask, _ = window_geometry(H, W, shift)
    real = (pix >= 0).to(dev)
    pixc = pix.clamp_min(0).to(dev)
    nW = pix.shape[0]
    tok = qkv.reshape(n, H * W, C3)[:, pixc]                                  # [n,nW,49,3C]
    if pad is None:
        assert bool(real.all())
    else:
        tok = torch.where(real[None, :, :, None], tok, pad.to(ft).view(1, 1, 1, C3))
    q, k, v = tok.view(n, nW, L, 3, heads, dh).permute(3, 0, 1, 4, 2, 5)      # each [n,nW,h,49,dh]
    tab = rnd(rel_bias(rpb, heads)[None] + mask[:, None], dt).to(dev, ft)     # A1: [nW,h,49,49]
    s = _bmm(q, k, dt, ft) * scale + tab                                      # A3: [n,nW,h,query,key]
    if ft == F64:
        p = torch.softmax(s, -1)
        o = p @ v
    else:
        m = s.max(-1, keepdim=True).values
        p = torch.exp(s - m)
        l = p.sum(-1, keepdim=True)
        o = _bmm(r(p), v.transpose(-1, -2), dt, ft) * (1.0 / l)

    def to_map(t, width):                                                      # [n,nW,h,49,dh] x k -> [n,H,W,width] at the real tokens
        flat = torch.zeros(n, H * W, width, dtype=ft, device=dev)
        flat[:, pixc[real]] = t[:, real]
        return flat.view(n, H, W, width)

    out = dict(o=to_map(o.permute(0, 1, 3, 2, 4).reshape(n, nW, L, C), C))
    if d_out is None:
        return out
    do = d_out.to(ft).reshape(n, H * W, C)[:, pixc] * real[None, :, :, None].to(ft)
    do = do.view(n, nW, L, heads, dh).permute(0, 1, 3, 2, 4)
    dP = _bmm(do, v, dt, ft)                                                  # [.., query, key]
    if ft == F64:
        delta = (p * dP).sum(-1, keepdim=True)
        dS = p * (dP - delta)
        dq = (dS @ k) * scale
        dk = (dS.transpose(-1, -2) @ q) * scale
        dv = p.transpose(-1, -2) @ do
    else:
        pn = p * (1.0 / l)                                                    # A4
        delta = (pn * dP).sum(-1, keepdim=True)
        dS = pn * (dP - delta)
        dq = _bmm(r(dS), k.transpose(-1, -2), dt, ft) * scale
        p2 = torch.exp(s - (m + torch.log(l)))                                # A5
        dv = _bmm(r(p2).transpose(-1, -2), do.transpose(-1, -2), dt, ft)
        dk = _bmm(r(p2 * (dP - delta)).transpose(-1, -2), q.transpose(-1, -2), dt, ft) * scale
    types = window_types(H, W, shift).to(dev)
    dtab = torch.zeros(4, heads, 64, 64, dtype=ft, device=dev)
    dtab[:, :, :L, :L] = torch.zeros(4, heads, L, L, dtype=ft, device=dev).index_add_(0, types, dS.sum(0))
    cat = torch.cat([t.permute(0, 1, 3, 2, 4).reshape(n, nW, L, C) for t in (dq, dk, dv)], -1)
    padk = (~real)[None, :, None, :, None].to(ft)                             # A6
    dbias = torch.zeros(C3, dtype=ft, device=dev)
    dbias[C:2 * C] = (dk * padk).sum((0, 1, 3)).reshape(C)
    dbias[2 * C:] = (dv * padk).sum((0, 1, 3)).reshape(C)
    out.update(dqkv=to_map(cat, C3), dtab=dtab, dbias=dbias)
    return out


def window_attn_model(qkv, table_params, heads, shift, bias=None, d_out=None, *, dt, ft):
    """mtmp_swin_window_attn(_pad) and their backward on the un-padded [n,H,W,3C] map; table_params: relative_position_bias_table
    [169, heads] fp32; bias: the fp32 qkv bias whose rounded value is a pad token's q | k | v (A2).
    -> o [n,H,W,C] (+ dqkv, dtab [4,heads,64,64], dbias [3C] with d_out)"""
    pad = None if bias is None else rnd(bias, dt)
    return _attn_core(qkv.to(ft), pad, table_params, heads, shift, d_out, dt, ft)


def attn_block_model(x, ln_w, ln_b, eps, wqkv, bqkv, table_params, heads, shift, wproj, bproj, row_scale=None, *, dt=BF16, ft):
    """mtmp_swin_attn_block(_pad): x + row_scale[image] (proj(attention(qkv(norm1 x))) + bproj), B1 - B4"""
    r = _rounder(dt, ft)
    n, H, W, C = x.shape
    xf = x.to(ft)
    xn = r(_ln(xf, ln_w, ln_b, eps)[0])                                                   # B1
    qkv = r(_mm(xn.reshape(-1, C), wqkv, bqkv, dt, ft)).view(n, H, W, 3 * C)              # B2
    a = r(_attn_core(qkv, r(bqkv.to(ft)), table_params, heads, shift, None, dt, ft)["o"])  # B3
    pr = r(_mm(a.reshape(-1, C), wproj, bproj, dt, ft)).view(n, H, W, C)                  # B4
    if row_scale is not None:
        pr = r(pr * row_scale.to(ft).view(n, 1, 1, 1))
    return dict(y=pr + xf)


# ------------------------------------------------------------------------------------------ fused MLP, LayerNorm + projection
def swin_mlp_model(x, ln_w, ln_b, eps, w1, b1, w2, b2, row_scale=None, rows_per_scale=1, *, dt=BF16, ft):
    r = _rounder(dt, ft)
    xf = x.to(ft)
    xn = r(_ln(xf, ln_w, ln_b, eps)[0])                                       # M1
    h = r(G.gelu_model(_mm(xn, w1, b1, dt, ft), dt, ft))
    v = r(_mm(h, w2, None, dt, ft) + b2.to(ft))                               # M2
    if row_scale is not None:
        rows = torch.arange(x.shape[0], device=x.device) // rows_per_scale
        v = r(v * row_scale.to(ft)[rows][:, None])
    return dict(y=v + xf)


def ln_linear_model(x, ln_w, ln_b, eps, w, bias, *, dt=BF16, ft):
    r = _rounder(dt, ft)
    return dict(y=_mm(r(_ln(x.to(ft), ln_w, ln_b, eps)[0]), w, bias, dt, ft))  # N1


# ------------------------------------------------------------------------------------------ stem
def stem_model(img, w, bias, ln_w, ln_b, order=None, *, dt, ft):
    """img [n,1,H,W] fp32, w [96,1,4,4] -> [n,H/4,W/4,96]: swin_transformer.py:559-567; slot b is made from image order[b] (S1)"""
    r = _rounder(dt, ft)
    n, _, H, W = img.shape
    if order is not None:
        img = img[order.long()]
    pat = img.to(ft).reshape(n, H // 4, 4, W // 4, 4).permute(0, 1, 3, 2, 4).reshape(-1, 16)
    acc = _mm(r(pat), r(w.to(ft).reshape(-1, 16)), None, dt, ft) + bias.to(ft)
    return dict(y=_ln(acc, ln_w, ln_b, EPS)[0].view(n, H // 4, W // 4, -1))


# ------------------------------------------------------------------------------------------ inputs (seeded, keyed by case name)
def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def ln_params(C, g):
    return 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)


def ln_inputs(rows, C, dt, seed=0, device="cpu"):
    """rows of std 1 .. 3 around 0.3; dy ~ 1.  Large cases are drawn on the device."""
    g = torch.Generator(device=device).manual_seed(int(_gen(21, rows, C, seed).initial_seed()))
    x = rnd((torch.randn(rows, C, generator=g, device=device) + 0.3) * (1 + 2 * torch.rand(rows, 1, generator=g, device=device)), dt)
    dy = rnd(torch.randn(rows, C, generator=g, device=device), dt)
    w, b = ln_params(C, _gen(22, C, seed))
    return dict(x=x, dy=dy, w=w.to(device), b=b.to(device))


def merge_inputs(n, H, W, Cs, dt, seed=0):
    g = _gen(23, n, H, W, Cs, seed)
    x = rnd(torch.randn(n, H, W, Cs, generator=g) * 1.5 + 0.2, dt)
    w, b = ln_params(4 * Cs, g)
    return dict(x=x, w=w, b=b)


def gelu_inputs(n, dt, seed=0, device="cpu"):
    """|x| up to 6 (a uniform sweep in random order) and dy ~ 1"""
    g = torch.Generator(device=device).manual_seed(int(_gen(24, n % 100003, seed).initial_seed()))
    x = rnd(12 * torch.rand(n, generator=g, device=device) - 6, dt)
    x[:8] = rnd(torch.tensor([-6.0, 6.0, 0.0, -0.75, 0.75, -3.0, 3.0, 1e-3], device=device), dt)
    return dict(x=x, dy=rnd(torch.randn(n, generator=g, device=device), dt))


def rpb_table(heads, g):
    """relative_position_bias_table of a trained encoder's scale (|.| up to ~1)"""
    return 0.4 * torch.randn((2 * WS - 1) ** 2, heads, generator=g)


def attn_inputs(n, H, W, heads, dt, seed=0, pad=False):
    """qkv ~ 1 (logits of std ~ 1 at head_dim 32), d_out ~ 1, the qkv bias ~ 0.5 of a padded map"""
    C = heads * DH
    g = _gen(25, n, H, W, heads, seed)
    return dict(qkv=rnd(torch.randn(n, H, W, 3 * C, generator=g), dt), d_out=rnd(torch.randn(n, H, W, C, generator=g), dt),
                rpb=rpb_table(heads, g), bias=0.5 * torch.randn(3 * C, generator=g) if pad else None)


def mlp_inputs(M, C, dt=BF16, seed=0):
    g = _gen(26, M, C, seed)
    x = rnd((torch.randn(M, C, generator=g) + 0.2) * (1 + torch.rand(M, 1, generator=g)), dt)
    ln_w, ln_b = ln_params(C, g)
    w1 = rnd(torch.randn(4 * C, C, generator=g) / math.sqrt(C), dt)
    w2 = rnd(torch.randn(C, 4 * C, generator=g) / math.sqrt(4 * C), dt)
    return dict(x=x, ln_w=ln_w, ln_b=ln_b, w1=w1, b1=0.3 * torch.randn(4 * C, generator=g), w2=w2, b2=0.3 * torch.randn(C, generator=g))


def row_scales(M, rows_per_scale):
    """StochasticDepth factors 1.25 | 0 | 1 in turn (a 0 included as soon as there are two)"""
    k = (M + rows_per_scale - 1) // rows_per_scale
    return torch.tensor([(1.25, 0.0, 1.0)[i % 3] for i in range(k)])


def ln_linear_inputs(M, C, N, dt=BF16, seed=0, bias=True):
    g = _gen(27, M, C, N, seed)
    x = rnd((torch.randn(M, C, generator=g) + 0.2) * (1 + torch.rand(M, 1, generator=g)), dt)
    ln_w, ln_b = ln_params(C, g)
    return dict(x=x, ln_w=ln_w, ln_b=ln_b, w=rnd(torch.randn(N, C, generator=g) / math.sqrt(C), dt),
                bias=0.3 * torch.randn(N, generator=g) if bias else None)


def block_inputs(n, H, W, C, dt=BF16, seed=0):
    heads = C // DH
    g = _gen(28, n, H, W, C, seed)
    x = rnd(torch.randn(n, H, W, C, generator=g) * 1.5 + 0.2, dt)
    ln_w, ln_b = ln_params(C, g)
    return dict(x=x, ln_w=ln_w, ln_b=ln_b, wqkv=rnd(torch.randn(3 * C, C, generator=g) / math.sqrt(C), dt),
                bqkv=0.3 * torch.randn(3 * C, generator=g), rpb=rpb_table(heads, g),
                wproj=rnd(torch.randn(C, C, generator=g) / math.sqrt(C), dt), bproj=0.3 * torch.randn(C, generator=g))


def stem_inputs(n, H, W, seed=0):
    """pixels in [0, 1) like the normalised chest X-rays; a conv of the trained stem's scale"""
    g = _gen(29, n, H, W, seed)
    ln_w, ln_b = ln_params(96, g)
    return dict(img=torch.rand(n, 1, H, W, generator=g), w=0.5 * torch.randn(96, 1, 4, 4, generator=g),
                bias=0.2 * torch.randn(96, generator=g), ln_w=ln_w, ln_b=ln_b)


# ------------------------------------------------------------------------------------------ launch arithmetic and case tables
def ln_rpw(C):
    """rows per wave of ln_rows(_bwd)_kernel: a group of G = 16 | 32 | 64 lanes owns a row"""
    G_ = 16
    while G_ < C // 8 and G_ < 64:
        G_ <<= 1
    return 64 // G_


def ln_bwd_slab_rows(rows, C):
    """swin_bwd.hip ln_bwd_blocks: one slab row per workgroup of 4 waves, 1024 at the most"""
    rpw = ln_rpw(C)
    return min(((rows + rpw - 1) // rpw + 3) // 4, 1024)


LN_WIDTHS = (8, 96, 192, 384, 768, 1536)
LN_WRAP = [(96, 65536 + 1), (768, 16384 + 1), (1536, 16384 + 1)]              # 4096 workgroups x 4 RPW rows
LN_BWD_WRAP = [(96, 16384 + 1), (768, 4096 + 1)]                              # 1024 workgroups x 4 RPW rows


def ln_rows_cases(C):
    """rows on both sides of RPW and of one workgroup trip (4 RPW)"""
    rpw = ln_rpw(C)
    return sorted({1, rpw - 1, rpw, rpw + 1, 4 * rpw - 1, 4 * rpw, 4 * rpw + 1} - {0})


def ln_bwd_rows_cases(C):
    rpw = ln_rpw(C)
    return sorted({1, rpw - 1, rpw + 1, 4 * rpw - 1, 4 * rpw + 1} - {0})


#              n, H, W, Cs: 4 Cs = 384, 768, 1536; 6 x 10 is not square; at 4 Cs = 96 (four rows per wave) the 15 merged rows end inside a
#              row group, at 384 the 3 merged rows inside a workgroup's four
MERGE_CASES = [(2, 6, 10, 96), (1, 6, 6, 192), (1, 4, 6, 384), (3, 2, 2, 96), (1, 6, 10, 24)]
GELU_N = (8, 2048 + 8, 8192 * 256 * 8 + 8)
#              n, H, W, heads, shift
WATTN_CASES = [(1, 7, 7, 3, 0), (2, 14, 14, 3, 0), (2, 14, 14, 3, 3), (1, 14, 14, 3, 1), (1, 14, 14, 3, 6), (2, 14, 21, 3, 3),
               (2, 21, 14, 3, 3), (1, 14, 14, 6, 3), (1, 14, 14, 24, 3), (1, 14, 21, 6, 0)]
WATTN_PAD_CASES = [(2, 5, 5, 3, 0), (2, 8, 8, 3, 0), (2, 8, 8, 3, 3), (1, 13, 13, 3, 0), (1, 13, 13, 3, 3), (1, 9, 16, 3, 0),
                   (1, 9, 16, 3, 3), (1, 16, 9, 3, 0), (1, 16, 9, 3, 3), (1, 15, 15, 3, 0), (1, 15, 15, 3, 3), (1, 8, 8, 6, 3)]
M_EDGES = (1, 31, 32, 33, 127, 128, 129, 257)
#              n, H, W, shift
BLOCK_CASES = [(2, 7, 7, 0), (2, 14, 14, 0), (3, 14, 14, 3), (1, 14, 21, 3)]            # (three images: the factors 1.25, 0 and 1)
BLOCK_PAD_CASES = [(2, 5, 5, 0), (2, 8, 8, 0), (2, 8, 8, 3), (1, 13, 13, 0), (1, 13, 13, 3), (1, 9, 16, 3)]
#              n, H, W (pixels): 1, 4, 64 x 2, 132 and 40 patches per image
STEM_CASES = [(1, 4, 4), (1, 8, 8), (2, 32, 32), (1, 44, 48), (3, 16, 40)]


# ------------------------------------------------------------------------------------------ probes
MLP_PROBE_M = 129
MLP_PROBE_GAIN = 64.0
MLP_PANEL = {96: 64, 192: 32}                                                 # MlpGeom<C, HP>: hidden units per panel


def mlp_probe_inputs(C, dt=BF16):
    """w2 is zero outside the LAST panel's columns and MLP_PROBE_GAIN times the usual inside; b2 = 0; x is a tenth of the usual:
    the output is that panel's term"""
    p = mlp_inputs(MLP_PROBE_M, C, dt, seed=91)
    w2 = p["w2"].clone()
    w2[:, :4 * C - MLP_PANEL[C]] = 0
    w2[:, 4 * C - MLP_PANEL[C]:] *= MLP_PROBE_GAIN
    return dict(p, w2=rnd(w2, dt), b2=torch.zeros(C), x=rnd(0.1 * p["x"], dt))


def mlp_probe_lost(p):
    return dict(p, w2=torch.zeros_like(p["w2"]))


CORNER_PROBE = dict(n=1, H=14, W=21, heads=3, shift=3)


def corner_probe_windows():
    """the corner window and its two neighbours on the 2 x 3 window grid: (index, name)"""
    return [(2, "last_column"), (4, "last_row"), (5, "corner")]


def corner_probe_inputs(dt):
    """v (forward) and d_out (backward) are zero outside the tokens of the three windows"""
    c = CORNER_PROBE
    p = attn_inputs(c["n"], c["H"], c["W"], c["heads"], dt, seed=92)
    pix = window_geometry(c["H"], c["W"], c["shift"])[0]
    keep = torch.zeros(c["H"] * c["W"], dtype=torch.bool)
    for w, _ in corner_probe_windows():
        keep[pix[w]] = True
    keep = keep.view(1, c["H"], c["W"], 1)
    C = c["heads"] * DH
    qkv = p["qkv"].clone()
    qkv[..., 2 * C:] *= keep
    return dict(p, qkv=qkv, d_out=p["d_out"] * keep)


def window_tokens(H, W, shift, w):
    """bool [H,W]: the pixels of window w's real tokens"""
    pix = window_geometry(H, W, shift)[0][w]
    m = torch.zeros(H * W, dtype=torch.bool)
    m[pix[pix >= 0]] = True
    return m.view(H, W)


PAD_PROBE = dict(n=2, H=8, W=8, heads=3)
PAD_PROBE_GAIN = 4.0


def pad_probe_inputs(dt, shift):
    """v is zero on every real token and the qkv bias is PAD_PROBE_GAIN times the usual: o is what the pad tokens add as keys, and
    in the backward dbias is the pad tokens' gradient alone"""
    c = PAD_PROBE
    p = attn_inputs(c["n"], c["H"], c["W"], c["heads"], dt, seed=93 + shift, pad=True)
    C = c["heads"] * DH
    qkv = p["qkv"].clone()
    qkv[..., 2 * C:] = 0
    return dict(p, qkv=qkv, bias=PAD_PROBE_GAIN * p["bias"])


def pad_probe_lost(p):
    """the pad keys' values removed"""
    C = p["bias"].numel() // 3
    b = p["bias"].clone()
    b[2 * C:] = 0
    return dict(p, bias=b)


LN_BWD_PROBE = dict(rows=16384 + 5, C=96)                                     # second trip: rows 16384 .. 16388


def ln_bwd_probe_inputs(dt, device="cpu"):
    """dy is zero outside the rows of the second grid-stride trip"""
    p = ln_inputs(LN_BWD_PROBE["rows"], LN_BWD_PROBE["C"], dt, seed=94, device=device)
    dy = p["dy"].clone()
    dy[:16384] = 0
    return dict(p, dy=dy)
