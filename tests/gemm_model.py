"""Float64 references of the projection GEMMs of csrc/gemm.hip as the C entry points define them, the same chains in working
precision, the decoder of the sign-bit layout, and the inputs of tests/test_gemm_model_gpu.py.  Plain torch, device-agnostic (a model
runs where its tensors live: the few large-M cases evaluate it in float64 on the GPU); nothing here imports the HIP library.
Metric and tolerance rule are those of tests/row_kernels_model.py (err, bound, FLOOR, BF16_ROUND):

    err(got, ref) = max over elements |got - ref| / (|ref| + rms(ref))     over ONE output tensor of a launch, live rows only
    bound         = max(8 e_chain, 16 * 2^-24)  [+ 2^-8 for a bf16 output],   e_chain = err(working-precision chain, float64 chain)

Every model takes the tensors the entry point takes (operands already rounded to the compute type dt; gamma, beta, bias, row_scale
and stats in fp32) and a float type ft.  ft = float64 is the reference: the exact product and epilogue, no rounding anywhere.
ft = float32 is the yardstick chain: the same formulas in fp32, and for dt = bfloat16 a rounding to bf16 where the kernels round on
purpose -- read from gemm.hip, not fitted to what the kernels return:

  every product (_mm / the token walk of gemm_tn_model)
    P1  the matrix instruction walks the contraction index in k-steps (bf16: 16 per v_mfma_f32_32x32x16_bf16, fp32: 2 per
        v_mfma_f32_32x32x2_f32) and rounds the running fp32 sum after each; the chain accumulates in the same steps, in index order.
        A K tail is zero-filled up to the 64-wide chunk (tile_commit), which changes no sum
    P2  ln_gemm_kernel / ln_gemm_dma_kernel take the bias block as the INITIAL accumulator (bias_fetch into the first MFMA's C operand;
        the sB rows copied into acc at the top of a phase): partial sums are rounded at |bias + sum|.  gemm_nt_kernel starts from zero
        and adds the bias in epilogue()
    P3  the weight-gradient kernels walk the tokens of ONE split in order and write a partial slab; the slabs are summed afterwards
        (reduce_batch_kernel).  The chain walks each split's rows in k-steps and adds the splits' sums (`splits`, the launch's count)
  ln_gemm (ln_gemm_kernel prologue, ln_gemm_dma_kernel prologue: identical arithmetic)
    L1  mean = sum / 256 and sigma = sqrt(sum (x - mean)^2 / 255) in fp32 from the compute-type row; rs = 1 / (sigma + eps)
    L2  xn = T(fma(gamma, (x - mean) * rs, beta)): the normalised row is rounded to the compute type BEFORE the matrix product (it is
        the MFMA's operand fragment `af`), and the stored xn is that same value
    L3  the key-norm table (N = 768, knorm_fold / piece()): for each wave's 32 rows and head h, sqrt(max over rows of sum over the 64
        features 256 + 64 h .. of v^2), v = the fp32 ACCUMULATOR (bias included, before the store to bf16) -- so the table is built from
        the unrounded keys; fp32 launches mtmp_key_norms on the stored fp32 y, the same values.  Rows of a last block past M replicate
        row M-1 (row = min(m_wave + r, M - 1)): the maximum over the block's live rows
    L4  sign bits (SIGNS): v > 0 of the fp32 accumulator after bias; the stored y is T(v) where the bit is set and 0 elsewhere
  gated dH (ln_gemm_dma_kernel<GATE>)
    G1  y = T(acc * gate_scale) where the forward's bit is set, 0 elsewhere: no rounding before the final store
  gemm_nt (gemm_nt_kernel + epilogue())
    N1  phase 1 parks T(act(acc + bias)) in the LDS staging tile; phase 2 reads it back.  With none of gate / row_scale / residual
        that IS the final store; with any of them it is a rounding point in front of them
    N2  y = T(round_T(v) + res): the staged (gated, scaled) value is rounded once more before the residual is added (round_as<T>)
    N3  order of phase 2: gate (gate > 0 ? v * gate_scale : 0), then row_scale[row / rows_per_scale], then the residual
    N4  GELU: fp32 evaluates 0.5 x (1 + erf(x / sqrt 2)) (erf to 1.5e-7); bf16 evaluates x * sigmoid(1.5957691216 x + 0.0713548163 x^3),
        the tanh form (common.hip.h gelu<bf16>).  The reference is the exact GELU; the bf16 chain uses the kernel's form
  gemm_lnbwd (gemm_lnbwd_kernel)
    B1  dxn = T(dy Wt^T): the finished tile is parked in LDS as the compute type before the LayerNorm backward reads it; dz, dgamma
        and dbeta all come from that rounded tile, in fp32, with the VALUES of `stats` (row_kernels_model.ln_bwd_model)
  gemm_tn: no rounding point (fp32 accumulators, fp32 slabs).
  dropout (keep = tests/dropout_model.Keep: the replayed mask and the one fp32 value keep_scale; None = off, nothing changes)
    D1  epilogues of ln_gemm and gemm_nt: v = act(acc + bias) in fp32, then keep ? v * keep_scale : 0, then the rounding of the store
        / of the parked tile (N1), then gate, row scale and residual as above.  The sign bits are "positive and kept"
    D2  dropout_bwd_kernel and the operand drop of the gated dH launch: T(float32(g) * keep_scale) or 0 -- one fp32 product and one
        rounding, both reproduced exactly (dropout_bwd_model); the product of the dH launch takes that ROUNDED operand

The final store of an output to bf16 is NOT part of the chain: that is the 2^-8 of the bound.
No element is left out of any check: ReLU and GELU are continuous, and the one discontinuous step -- the gate of dH -- takes the
kernel's own sign bits (asserted to be exactly y > 0) as the model's boolean input.

Sign bits (gemm.hip, the comment in front of ln_gemm_dma_kernel): one 16-bit word per (32-feature group G = 2 j + g, row, lane half),
signs[((2 j + g) M + row) 2 + half]; a lane collects its 16 accumulator registers t = 0..15 first to last by word = 2 word + bit, so
register t is bit 15 - t; through swz23 register t of lane half `half` is feature 16 (t >> 3) + 8 half + (t & 7) of the group.
"""
import math

import torch

from tests.row_kernels_model import (BF16, BF16_ROUND, F32, F64, FLOOR, LN_EPS, bound, dt_name, err, ln_bwd_model,  # noqa: F401
                                     ln_stats, rnd)

D = 256
DTS = (F32, BF16)
ACTS = (None, "relu", "gelu")


def _rounder(dt, ft):
    """the chain's rounding to the compute type: active only in the working-precision chain of a bf16 kernel"""
    if ft == F32 and dt == BF16:
        return lambda t: t.to(BF16).to(F32)
    return lambda t: t


def _kstep(dt):
    return 16 if dt == BF16 else 2


def _mm(a, w, c0, dt, ft):
    """c0 + a w^T (a [M,K], w [N,K], c0 [N] | None) as the matrix pipe forms it (P1, P2); float64: the plain product"""
    a, w = a.to(ft), w.to(ft)
    if ft == F64:
        y = a @ w.t()
        return y if c0 is None else y + c0.to(ft)
    wt = w.t().contiguous()
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=ft, device=a.device)
    if c0 is not None:
        acc += c0.to(ft)
    for k in range(0, a.shape[1], _kstep(dt)):
        acc.addmm_(a[:, k:k + _kstep(dt)], wt[k:k + _kstep(dt)])
    return acc


def gelu_model(x, dt, ft):
    """N4"""
    if ft == F32 and dt == BF16:
        return x * torch.sigmoid(x * (1.5957691216 + 0.0713548163 * x * x))
    return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


def _drop(v, keep, fault=None):
    """D1 on an fp32 / float64 tensor; fault (tests/dropout_model.MODEL_FAULTS): "no_scale", or "scale_after_round" = the value is
    rounded to bf16 BEFORE the scale"""
    if keep is None:
        return v
    if fault == "scale_after_round":
        v = v.to(BF16).to(v.dtype)
    kept = v if fault == "no_scale" else v * keep.scale
    return torch.where(keep.mask.to(v.device), kept, torch.zeros_like(v))


def _act(v, act, dt, ft):
    if act == "relu":
        return torch.relu(v)
    if act == "gelu":
        return gelu_model(v, dt, ft)
    assert act in (None, "none"), act
    return v


# ------------------------------------------------------------------------------------------ LayerNorm-fed row-panel projection
def knorm_model(y):
    """L3: y [M,768] (unrounded) -> [ceil(M / 32), 4]: per block of 32 rows the largest ||k_h||, k_h = y[:, 256 + 64 h : 320 + 64 h]"""
    M = y.shape[0]
    nrm = y[:, D:2 * D].reshape(M, 4, 64).pow(2).sum(-1).sqrt()
    nblk = (M + 31) // 32
    pad = nrm[M - 1:].expand(32 * nblk - M, 4)                          # rows past M replicate row M-1
    return torch.cat([nrm, pad]).reshape(nblk, 32, 4).max(1).values


def ln_gemm_model(x, gamma, beta, w, bias, act=None, keep=None, fault=None, *, dt, ft):
    """module.py:138-144 (unbiased std, eps added to the std) in front of y = drop(act(xn W^T + b)): x [M,256], w [N,256], bias [N] |
    None, keep: the dropout of D1 over the [M,N] output.
    -> y, xn, mean, rstd (the two columns of `stats`), and for N = 768 the key-norm table knorm."""
    r = _rounder(dt, ft)
    xf = x.to(ft)
    mean = xf.sum(-1, keepdim=True) / D
    d = xf - mean
    rs = 1.0 / ((d * d).sum(-1, keepdim=True) / (D - 1)).sqrt().add(LN_EPS)                                   # L1
    xn = gamma.to(ft) * (d * rs) + beta.to(ft)                                                                # L2
    v = _mm(r(xn), w, bias, dt, ft)                                                                           # P1, P2
    out = dict(y=_drop(_act(v, act, dt, ft), keep, fault), xn=xn, mean=mean[:, 0], rstd=rs[:, 0])                    # D1
    if w.shape[0] == 3 * D:
        out["knorm"] = knorm_model(v)                                                                         # L3
    return out


def gated_model(a, w, gate, gate_scale, *, dt, ft):
    """dH = gate ? (a W^T) * gate_scale : 0 -- a [M,256], w [N,256], gate bool [M,N] (G1)"""
    v = _mm(a, w, None, dt, ft) * gate_scale
    return dict(y=torch.where(gate, v, torch.zeros_like(v)))


def dropout_bwd_model(g, keep, *, dt):
    """D2, exact: g (values of the compute type) -> the values of T(float32(g) * keep_scale) where kept, 0 elsewhere, as fp32"""
    v = (g.to(F32) * keep.scale).to(dt).to(F32)
    return dict(y=torch.where(keep.mask.to(g.device), v, torch.zeros_like(v)))


def operand_drop_model(a, keep, w, gate, gate_scale, *, dt, ft):
    """the gated dH launch with the backward of a dropout folded onto its operand: a' = dropout_bwd_model(a), dH = gated_model(a')"""
    ad = dropout_bwd_model(a, keep, dt=dt)["y"]
    return dict(a=ad, y=gated_model(ad, w, gate, gate_scale, dt=dt, ft=ft)["y"])


# ------------------------------------------------------------------------------------------ the generic NT product
def gemm_nt_model(a, w, bias=None, res=None, act=None, gate=None, gate_scale=1.0, row_scale=None, rows_per_scale=1, keep=None,
                  fault=None, *, dt, ft):
    """y = drop(act(a W^T + b)) [gate > 0 ? * gate_scale : 0] [* row_scale[row // rows_per_scale]] [+ res], in the order of epilogue()"""
    r = _rounder(dt, ft)
    v = _mm(a, w, None, dt, ft)
    if bias is not None:
        v = v + bias.to(ft)
    v = _act(v, act, dt, ft)
    if fault == "behind_residual":                                       # (the fault: drop(v + res) for drop(v) + res)
        return dict(y=_drop(r(v) + res.to(ft), keep))
    v = _drop(v, keep, fault)                                                                                 # D1
    if gate is None and row_scale is None and res is None:
        return dict(y=v)
    v = r(v)                                                                                                  # N1
    if gate is not None:
        v = torch.where(gate.to(ft) > 0, v * gate_scale, torch.zeros_like(v))                                 # N3
    if row_scale is not None:
        rows = torch.arange(a.shape[0], device=a.device) // rows_per_scale
        v = v * row_scale.to(ft)[rows][:, None]
    if res is not None:
        v = r(v) + res.to(ft)                                                                                 # N2
    return dict(y=v)


# ------------------------------------------------------------------------------------------ dX + LayerNorm backward
def gemm_lnbwd_model(dy, wt, z, stats, gamma, d_res, *, dt, ft):
    """dxn = dy Wt^T (dy [M,K], wt [256,K]); dz, dgamma, dbeta = LayerNorm backward of it at (z, stats) (+ d_res).  On the CPU."""
    dxn = _rounder(dt, ft)(_mm(dy, wt, None, dt, ft))                                                         # B1
    return ln_bwd_model(z, stats, gamma, dxn, d_res, ft=ft)


# ------------------------------------------------------------------------------------------ weight gradient
def tn_rows_per_split(M, splits):
    """the token rows of one split (tn_args / the kernels' packed form): the share of M rounded up to the 64-token step"""
    return ((M + splits - 1) // splits + 63) // 64 * 64


def gemm_tn_model(dy, x, splits=1, drop=None, *, dt, ft):
    """dw = dy^T x [N,K], db = column sums of dy [N] (dy [M,N], x [M,K]).  splits: the launch's split count (P3).  drop = (lo, hi): the
    token rows whose term is REMOVED from both sums -- what a kernel that loses that step would return."""
    dy, x = dy.to(ft), x.to(ft)
    if drop is not None:
        keep = torch.ones(dy.shape[0], 1, dtype=ft, device=dy.device)
        keep[drop[0]:drop[1]] = 0
        dy = dy * keep
    if ft == F64:
        return dict(dw=dy.t() @ x, db=dy.sum(0))
    M, step, rps = dy.shape[0], _kstep(dt), tn_rows_per_split(dy.shape[0], splits)
    dyt = dy.t().contiguous()
    dw = torch.zeros(dy.shape[1], x.shape[1], dtype=ft, device=dy.device)
    db = torch.zeros(dy.shape[1], dtype=ft, device=dy.device)
    for lo in range(0, M, rps):
        hi = min(M, lo + rps)
        acc = torch.zeros_like(dw)
        for k in range(lo, hi, step):
            acc.addmm_(dyt[:, k:min(k + step, hi)], x[k:min(k + step, hi)])
        dw += acc
        db += dy[lo:hi].sum(0)
    return dict(dw=dw, db=db)


def tn_last_step(M, splits, step=64):
    """(lo, hi): the token rows of the last `step`-token step of the last split that has rows"""
    rps = tn_rows_per_split(M, splits)
    lo_split = (M - 1) // rps * rps
    lo = lo_split + (M - 1 - lo_split) // step * step
    return lo, M


# ------------------------------------------------------------------------------------------ sign bits
def _sign_place(N, device):
    """per column: (group G, lane half, bit) of its sign"""
    col = torch.arange(N, device=device)
    f = col % 32
    t = 8 * (f >> 4) + (f & 7)
    return col // 32, (f >> 3) & 1, 15 - t


def decode_signs(raw, M, N):
    """raw: the uint8 buffer of mtmp_sign_bits_bytes(M, N) = (N / 32) M 4 bytes (little-endian 16-bit words) -> bool [M,N]"""
    b = raw.reshape(N // 32, M, 2, 2).to(torch.int32)
    words = b[..., 0] | (b[..., 1] << 8)                                 # [G, row, half]
    G, half, bit = _sign_place(N, raw.device)
    return ((words[G, :, half] >> bit[:, None]) & 1).t().bool()


def live_words(raw, M, N, live):
    """bool mask over raw's bytes: the words of rows < live"""
    m = torch.zeros(N // 32, M, 4, dtype=torch.bool, device=raw.device)
    m[:, :live] = True
    return m.reshape(-1)


# ------------------------------------------------------------------------------------------ inputs
def _gen(*key):
    return torch.Generator().manual_seed(hash(tuple(int(k) for k in key)) % (2 ** 31))


def ln_gemm_inputs(M, N, dt, seed=0, bias=True, ldx=D):
    """x [M,256] (a column window [8 : 264] of an [M, ldx] buffer when ldx > 256), gamma, beta, w [N,256], bias [N] | None: scales of
    tests/test_gpu_parity.py (rows of std 1 .. 4 around 0.3, w ~ 0.08, bias ~ 0.3)"""
    g = _gen(11, M, N, seed)
    buf = rnd((torch.randn(M, ldx, generator=g) + 0.3) * (1 + 3 * torch.rand(M, 1, generator=g)), dt)
    x = buf[:, 8:8 + D] if ldx > D else buf
    gam, bet = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    w = rnd(0.08 * torch.randn(N, D, generator=g), dt)
    b = 0.3 * torch.randn(N, generator=g) if bias else None
    return dict(x=x, gamma=gam, beta=bet, w=w, bias=b)


def gated_inputs(M, N, dt, seed=0):
    g = _gen(12, M, N, seed)
    return dict(a=rnd(torch.randn(M, D, generator=g), dt), w=rnd(0.06 * torch.randn(N, D, generator=g), dt))


def nt_inputs(M, N, K, dt, seed=0, bias=True, res=False, gate=False, row_scale=0, lda=None, ldr=None):
    """a [M,K] (window of an [M, lda] buffer), w [N,K] ~ 1 / sqrt(K), bias ~ 0.3, res [M,N] (window of [M, ldr]), gate [M,N] (about
    half positive, exact zeros included), row_scale [ceil(M / row_scale)] in (0.5, 1.5)"""
    g = _gen(13, M, N, K, seed)
    lda, ldr = lda or K, ldr or N
    a = rnd(torch.randn(M, lda, generator=g), dt)[:, lda - K:]
    w = rnd(torch.randn(N, K, generator=g) / math.sqrt(K), dt)
    out = dict(a=a, w=w, bias=0.3 * torch.randn(N, generator=g) if bias else None)
    out["res"] = rnd(torch.randn(M, ldr, generator=g), dt)[:, ldr - N:] if res else None
    if gate:
        gt = torch.randn(M, N, generator=g)
        gt[torch.rand(M, N, generator=g) < 0.05] = 0.0
        out["gate"] = rnd(gt, dt)
    else:
        out["gate"] = None
    out["row_scale"] = 0.5 + torch.rand((M + row_scale - 1) // row_scale, generator=g) if row_scale else None
    return out


def lnbwd_inputs(M, K, dt, seed=0, res=True, ldz=D, ldr=D):
    g = _gen(14, M, K, seed)
    z = rnd(torch.randn(M, ldz, generator=g) * 2 + 0.3, dt)[:, ldz - D:]
    dy = rnd(torch.randn(M, K, generator=g), dt)
    wt = rnd(torch.randn(D, K, generator=g) / math.sqrt(K), dt)
    gam = 1 + 0.1 * torch.randn(D, generator=g)
    d_res = rnd(torch.randn(M, ldr, generator=g), dt)[:, ldr - D:] if res else None
    return dict(dy=dy, wt=wt, z=z, stats=ln_stats(z), gamma=gam, d_res=d_res)


def tn_inputs(M, N, K, dt, seed=0, off=None):
    """dy [M,N], x [M,K]; off = (oy, ox): column windows [o : o + width] of buffers 64 columns wider (row strides stay multiples of 8)"""
    g = _gen(15, M, N, K, seed)
    extra = 0 if off is None else 64
    oy, ox = off or (0, 0)
    wy = rnd(torch.randn(M, N + extra, generator=g), dt)
    wx = rnd(torch.randn(M, K + extra, generator=g), dt)
    return dict(dy=wy[:, oy:oy + N], x=wx[:, ox:ox + K])


# ------------------------------------------------------------------------------------------ one-tile probes
PROBE_BOUND, PROBE_LOSS = 0.25, 0.5           # the bound a probe may have at most; the err losing its piece must cost at least
NT_PROBE = dict(M=65, N=160, K=72)            # K tail chunk of gemm_nt: nk = 2, the second chunk holds 8 columns
NT_PROBE_GAIN = 32.0
PANEL_PROBE = dict(M=8193, N=1024)            # 65 row blocks -> 7 panel shares of 3 | 3 | 3 | 3 | 3 | 1 | 0 panels
PANEL_PROBE_GAIN = 32.0
TN_PROBE = dict(M=6700, N=256, K=1024)        # mode 3, 12 splits of 576 rows: the last has 364 = 5 steps of 64 + 44
TN_PROBE_GAIN = 64.0


def panel_shares(M, N, np_=64, maxp=16):
    """launch_ln_gemm_dma: [(first panel, panels)] of each workgroup share along gridDim.y"""
    mtiles, npanels = (M + 127) // 128, N // np_
    nsplit = max(1, min(npanels, 512 // mtiles))
    nsplit = max(nsplit, (npanels + maxp - 1) // maxp)
    per = (npanels + nsplit - 1) // nsplit
    return [(j0, max(0, min(npanels, j0 + per) - j0)) for j0 in range(0, nsplit * per, per)]


def nt_probe_inputs(dt):
    """the 8 columns of the K tail carry NT_PROBE_GAIN^2 * 8 / 64 = 128 times the mass of the 64 columns in front"""
    p = nt_inputs(dt=dt, seed=77, bias=False, **NT_PROBE)
    a, w = p["a"].clone(), p["w"].clone()
    a[:, 64:] *= NT_PROBE_GAIN
    w[:, 64:] *= NT_PROBE_GAIN
    return dict(p, a=rnd(a, dt), w=rnd(w, dt))


def nt_probe_lost(p):
    """the operands of the product without its K tail chunk"""
    a, w = p["a"].clone(), p["w"].clone()
    a[:, 64:] = 0
    return dict(p, a=a, w=w)


def panel_probe_panels():
    """the LAST panel of every share that holds two or more (per >= 2) -- the panels whose bias rows sit last in a workgroup's LDS block"""
    return [j0 + n - 1 for j0, n in panel_shares(**PANEL_PROBE) if n >= 2]


def panel_probe_inputs(dt):
    """the bias of the probe panels is PANEL_PROBE_GAIN times the usual one (|b| ~ 10 against |xn W^T| ~ 1.3): y there is its bias"""
    p = ln_gemm_inputs(dt=dt, seed=78, **PANEL_PROBE)
    b = p["bias"].clone()
    for j in panel_probe_panels():
        b[64 * j:64 * j + 64] = PANEL_PROBE_GAIN * b[64 * j:64 * j + 64].abs().clamp_min(0.05)         # (positive: it survives the ReLU)
    return dict(p, bias=b)


def panel_probe_lost(p, j):
    b = p["bias"].clone()
    b[64 * j:64 * j + 64] = 0
    return dict(p, bias=b)


def tn_probe_inputs(dt, splits):
    p = tn_inputs(dt=dt, seed=79, **TN_PROBE)
    lo, hi = tn_last_step(TN_PROBE["M"], splits)
    dy = p["dy"].clone()
    dy[lo:hi] *= TN_PROBE_GAIN
    return dict(p, dy=rnd(dy, dt))


def e_chain_of(model, *args, dt, **kw):
    """(float64 outputs, {name: e_chain}) of a model function"""
    ref, ch = model(*args, dt=dt, ft=F64, **kw), model(*args, dt=dt, ft=F32, **kw)
    return ref, {k: err(ch[k], ref[k]) for k in ref}
