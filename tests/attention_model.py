"""Float64 reference of the dense attention kernels and of the CLS-row pair (csrc/attention.hip) as the C entry points define them,
the same chain in working precision, and the inputs of tests/test_attention_model_gpu.py.  Plain torch on the CPU; nothing here
imports the HIP library.  Metric and tolerance rule are those of tests/row_kernels_model.py (err, bound, FLOOR, BF16_ROUND):

    err(got, ref) = max over elements |got - ref| / (|ref| + rms(ref))     over ONE output tensor of a launch, live rows only
    bound         = max(8 e_chain, 16 * 2^-24)  [+ 2^-8 for a bf16 output],   e_chain = err(working-precision chain, float64 chain)

Layout: q|k|v as [B, N, 768], 4 heads of 64, scale 1/8.  kv_len None, ragged, or 0 (the reference's masked_fill(-65504): the
uniform average over all N keys, no gradient to q or k).  PADDED: all N rows are queries (pad queries are live), keys are the
first kv_len rows.  PACKED: a sample's queries are its kv_len rows (the model takes the rows in padded form; the GPU test stores
them back to back).  Optional prefix mask (bool [P, P], True = query i does not attend key j).  lse is in the kernels' unit:
log2 of the sum of exp2 of the scaled scores (scaled by log2(e) / 8).

ft = float64 is the reference: exact softmax attention and its gradient, written out by hand (pinned to the oracle's autograd by
tests/test_attention_model_cpu.py); its only rounding is the one the entry points DEFINE: o_res = round_dt(o) + res.
ft = float32 is the yardstick chain.  For dt = float32 it is the same formulas in fp32.  For dt = bfloat16 it rounds to bf16 where
the kernels round on purpose -- read from the kernels, not fitted to their output:

  every score product (S = K Q^T, S' and dP' of the backward; fp32 and bf16 kernels alike)
    M1  the matrix instruction walks the head dimension in k-steps (fp32: 32 steps of 2, bf16: 4 steps of 16) and rounds the running
        sum to fp32 after each; the chain accumulates in the same steps (_dot).  With a key of norm ~60 the running sum reaches
        several hundred and this order, not the operands, sets the error of the score
    M2  the backward's row constants are the INITIAL accumulator of those products (S' = -lse + sum, dP' = -delta + sum: "row
        constants as the initial accumulator"), so every partial sum is rounded at the magnitude of lse, not of the score
    M3  the forward's row sum l and O are RUNNING sums in key order (l: one score at a time in each of the two half-lanes that
        share a row -- keys 8i..8i+3 / 8i+4..8i+7 -- joined at the end; O: one k-step of the P.V product at a time, 2 keys in fp32,
        16 in bf16): after a dominant first key the later terms are rounded at ITS magnitude (_row_sum, _pv).  The chain takes
        them at the final row maximum; the kernels' rescale by a power-free factor keeps the relative error of what was summed
  forward (attn_fwd_body)
    F1  the bounded body folds log2(e) / 8 into the Q fragments: q' = bf16(q * c2) (frag_scale); the online body scales the fp32
        score instead
    F2  P = bf16(p) before P.V (frag_from_acc); the row sum l is taken from the unrounded p
    F3  O is stored as bf16; o_res = O + res adds the STORED value
  backward, dQ (attn_bwd_dq_body)
    Q1  q' = bf16(q * c2) always (frag_scale), so p = exp2(q'.k - lse) is recomputed from other scores than the forward's
    Q2  delta = sum_d dO * O from the stored (bf16) O, in fp32
    Q3  dS = bf16(p * (dO.v - delta)) before dS.K
  backward, dK / dV (attn_bwd_dkdv_body and the 64-key attn_bwd_dkdv64_body alike)
    K1  k' = bf16(k * c2) (frag_scale): the scale sits on the KEY fragments here, p = exp2(q.k' - lse)
    K2  P = bf16(p) before dO^T P (dV)
    K3  dS = bf16(p * dP') with the unrounded p, before Q^T dS (dK)
  CLS-row pair (attn_cls_fwd_kernel / attn_cls_bwd_kernel): fp32 throughout; only O is stored as bf16 and read back (r1, delta).

The final store of an output (o, dq, dk, dv, o_res to bf16) is NOT part of the chain: that is the 2^-8 of the bound.
Every model function returns padded tensors plus the boolean row sets `qrows` / `krows`; flat() selects the live rows.
"""
import dataclasses
import functools
import math

import torch

from tests.row_kernels_model import BF16, BF16_ROUND, F32, F64, FLOOR, bound, dt_name, err, rnd  # noqa: F401  (re-exported)

H, DH, DM = 4, 64, 256
SCALE = 0.125
LOG2E_F32 = 1.4426950408889634          # the kernels' constant (rounded to fp32 there)
KT = 64                                  # rows of a kernel tile


def _c2(ft):
    """scale * log2(e): exact in float64; the kernels' fp32 product (0.125 * fp32(log2 e), exact) in the chain"""
    return SCALE * math.log2(math.e) if ft == F64 else float(torch.tensor(LOG2E_F32, dtype=F32)) * SCALE


def _rounder(dt, ft):
    """the chain's rounding to the compute type: active only in the working-precision chain of a bf16 kernel"""
    if ft == F32 and dt == BF16:
        return lambda t: t.to(BF16).to(F32)
    return lambda t: t


def _heads(t):
    """[n, 256] -> [4, n, 64]"""
    return t.reshape(t.shape[0], H, DH).transpose(0, 1)


def _merge(t):
    """[4, n, 64] -> [n, 256]"""
    return t.transpose(0, 1).reshape(t.shape[1], DM)


def _dot(a, bT, c0, dt, ft):
    """c0 + a @ bT over the head dimension as the matrix pipe forms it (M1, M2): k-steps of 2 (fp32) or 16 (bf16), the running sum
    -- which starts from c0 -- rounded to fp32 after each.  float64: the plain product."""
    if ft == F64:
        return a @ bT if c0 is None else c0 + a @ bT
    step = 16 if dt == BF16 else 2
    acc = torch.zeros(a.shape[0], a.shape[1], bT.shape[2], dtype=ft) if c0 is None else c0.expand(a.shape[0], a.shape[1], bT.shape[2]).clone()
    for d in range(0, DH, step):
        acc += a[..., d:d + step] @ bT[..., d:d + step, :]
    return acc


def _row_sum(p, ft):
    """l = sum over keys of p as the forward forms it (M3); float64: the plain sum"""
    if ft == F64:
        return p.sum(-1, keepdim=True)
    half = [torch.zeros(p.shape[:-1], dtype=ft), torch.zeros(p.shape[:-1], dtype=ft)]
    for j in range(p.shape[-1]):
        half[(j >> 2) & 1] += p[..., j]
    return (half[0] + half[1]).unsqueeze(-1)


def _pv(P, v, dt, ft):
    """P @ v as the forward's P.V product accumulates it (M3); float64: the plain product"""
    if ft == F64:
        return P @ v
    step = 16 if dt == BF16 else 2
    acc = torch.zeros(P.shape[0], P.shape[1], v.shape[-1], dtype=ft)
    for j in range(0, P.shape[-1], step):
        acc += P[..., j:j + step] @ v[:, j:j + step]
    return acc


def _keep(n, ranges, ft):
    """float[n]: 0 inside the (lo, hi) range that a `drop` argument names, 1 elsewhere"""
    k = torch.ones(n, dtype=ft)
    if ranges is not None:
        k[ranges[0]:ranges[1]] = 0
    return k


# ------------------------------------------------------------------------------------------ dense attention
def attention_model(qkv, kv_len, d_o=None, res=None, *, dt, ft, packed=False, mask=None, bounded=False, drop_k=None, drop_q=None):
    """qkv [B,N,768], kv_len (sequence of B ints | None), d_o [B,N,256] | None (forward only), res [B,N,256] | None.
    bounded: bool, 4 bools (per head) or B x 4 bools (per sample and head): which forward body the waves of that head take.
    drop_k / drop_q: per sample a (lo, hi) range | None -- the keys whose term is REMOVED from the sums over keys (o, dq; the
    softmax normalisation keeps them), the queries whose term is removed from the sums over queries (dk, dv): what a kernel that
    loses that tile would return.
    -> dict: o, o_res (if res), lse [B,4,N], dq, dk, dv (if d_o), qrows / krows bool[B,N]."""
    B, N, _ = qkv.shape
    r = _rounder(dt, ft)
    c2 = _c2(ft)
    if isinstance(bounded, (bool, int)):
        bounded = [[bool(bounded)] * H] * B
    elif isinstance(bounded[0], (bool, int)):
        bounded = [list(bounded)] * B
    z = lambda *s: torch.zeros(*s, dtype=ft)
    out = dict(o=z(B, N, DM), lse=z(B, H, N), qrows=torch.zeros(B, N, dtype=torch.bool), krows=torch.zeros(B, N, dtype=torch.bool))
    if res is not None:
        out["o_res"] = z(B, N, DM)
    if d_o is not None:
        out.update(dq=z(B, N, DM), dk=z(B, N, DM), dv=z(B, N, DM))
    for b in range(B):
        kvl = N if kv_len is None else min(int(kv_len[b]), N)
        Nq = max(kvl, 0) if packed else N
        if Nq == 0:
            continue
        uniform = kvl <= 0
        nk = Nq if uniform else kvl
        out["qrows"][b, :Nq] = True
        out["krows"][b, :nk] = True
        x = qkv[b].to(ft)
        q, k, v = _heads(x[:Nq, :DM]), _heads(x[:nk, DM:2 * DM]), _heads(x[:nk, 2 * DM:])
        if uniform:
            q = torch.zeros_like(q)                                        # every score 0: p = 1 / N
        bflag = torch.tensor([bool(x) for x in bounded[b]])[:, None, None]
        hide = torch.zeros(Nq, nk, dtype=torch.bool)
        if mask is not None:
            pq_, pk_ = min(mask.shape[0], Nq), min(mask.shape[1], nk)
            hide[:pq_, :pk_] = mask[:pq_, :pk_]
        keep_k = _keep(nk, None if drop_k is None else drop_k[b], ft)
        keep_q = _keep(Nq, None if drop_q is None else drop_q[b], ft)
        # ---- forward
        kT = k.transpose(-1, -2)
        s2 = _dot(q, kT, None, dt, ft) * c2 if not bool(bflag.all()) else None
        if bool(bflag.any()):
            s_b = _dot(r(q * c2), kT, None, dt, ft)                                                           # F1
            s2 = s_b if s2 is None else torch.where(bflag, s_b, s2)
        s2 = s2.masked_fill(hide, -math.inf)
        m = torch.where(bflag, torch.zeros(H, Nq, 1, dtype=ft), s2.max(-1, keepdim=True).values)
        p = torch.exp2(s2 - m)
        l = _row_sum(p, ft)                                                                                   # M3
        o_h = _pv(r(p * keep_k), v, dt, ft) / l                                                               # F2, M3
        O = r(o_h)                                                                                            # F3
        lse = (m + torch.log2(l)).squeeze(-1)
        out["o"][b, :Nq] = _merge(o_h)
        out["lse"][b, :, :Nq] = lse
        if res is not None:
            o_def = O if ft == F32 else o_h.to(dt).to(ft)              # the entry's definition: o rounded to the compute type first
            out["o_res"][b, :Nq] = _merge(o_def) + res[b, :Nq].to(ft)
        if d_o is None:
            continue
        # ---- backward
        g = _heads(d_o[b, :Nq].to(ft))
        delta = (g * O).sum(-1, keepdim=True)                                                                 # Q2
        dP = _dot(g, v.transpose(-1, -2), -delta, dt, ft)                                                     # M2
        if not uniform:
            pq = torch.exp2(_dot(r(q * c2), kT, -lse[..., None], dt, ft).masked_fill(hide, -math.inf))        # Q1, M2
            out["dq"][b, :Nq] = _merge(SCALE * ((r(pq * dP) * keep_k) @ k))                                   # Q3
        pk = torch.exp2(_dot(q, r(k * c2).transpose(-1, -2), -lse[..., None], dt, ft).masked_fill(hide, -math.inf))   # K1, M2
        pk = pk * keep_q[:, None]
        out["dv"][b, :nk] = _merge(r(pk).transpose(-1, -2) @ g)                                               # K2
        if not uniform:
            out["dk"][b, :nk] = _merge(SCALE * (r(pk * dP).transpose(-1, -2) @ q))                            # K3
    return out


DENSE_OUT = ("o", "o_res", "lse", "dq", "dk", "dv")


def flat(out):
    """the live rows of every output as one [rows, C] tensor per name (lse: [rows, 4]); dk / dv: the rows of live keys"""
    res = {}
    for name in DENSE_OUT:
        if name not in out:
            continue
        t = out[name].transpose(1, 2) if name == "lse" else out[name]
        res[name] = t[out["krows"] if name in ("dk", "dv") else out["qrows"]]
    return res


# ------------------------------------------------------------------------------------------ CLS-row pair
def attn_cls_model(qkv, z, kv_len, d_o, cls_tok, *, dt, ft, packed=False):
    """One query per sample (row cls_tok): o, r1 = round_dt(o) + z[:, cls_tok], lse [B,4]; for d_o [B,256] the gradient thirds dq
    [B,256] (row cls_tok, every other dq row is zero), dk / dv [B,N,256] (rows of live keys: krows)."""
    B, N, _ = qkv.shape
    r = _rounder(dt, ft)
    c2 = _c2(ft)
    zz = lambda *s: torch.zeros(*s, dtype=ft)
    out = dict(o=zz(B, DM), r1=zz(B, DM), lse=zz(B, H), dq=zz(B, DM), dk=zz(B, N, DM), dv=zz(B, N, DM), krows=torch.zeros(B, N, dtype=torch.bool))
    for b in range(B):
        kv_raw = N if kv_len is None else int(kv_len[b])
        assert not (packed and kv_raw <= cls_tok), "a packed sample without its CLS row"
        uniform = kv_raw <= 0
        nk = N if uniform else min(kv_raw, N)
        out["krows"][b, :nk] = True
        x = qkv[b].to(ft)
        q0 = x[cls_tok, :DM].reshape(H, 1, DH)
        k, v = _heads(x[:nk, DM:2 * DM]), _heads(x[:nk, 2 * DM:])
        s = ((q0 * (0.0 if uniform else c2)) @ k.transpose(-1, -2))                  # [4,1,nk]
        m = s.max(-1, keepdim=True).values
        p = torch.exp2(s - m)
        l = p.sum(-1, keepdim=True)
        o_h = (p @ v) / l
        O = r(o_h)
        lse = (m + torch.log2(l))
        out["o"][b] = _merge(o_h)[0]
        out["lse"][b] = lse.reshape(H)
        o_def = O if ft == F32 else o_h.to(dt).to(ft)
        out["r1"][b] = _merge(o_def)[0] + z[b, cls_tok].to(ft)
        g = d_o[b].to(ft).reshape(H, 1, DH)
        delta = (g * O).sum(-1, keepdim=True)
        pk = torch.exp2(s - lse)
        dS = torch.zeros_like(pk) if uniform else pk * (g @ v.transpose(-1, -2) - delta)
        out["dq"][b] = _merge(SCALE * (dS @ k))[0]
        out["dk"][b, :nk] = _merge(dS.transpose(-1, -2) @ (q0 * SCALE))
        out["dv"][b, :nk] = _merge(pk.transpose(-1, -2) @ g)
    return out


CLS_OUT = ("o", "r1", "lse", "dq", "dk", "dv")


def flat_cls(out):
    return {n: (out[n][out["krows"]] if n in ("dk", "dv") else out[n]) for n in CLS_OUT}


# ------------------------------------------------------------------------------------------ prefix masks (mbt_encoder.py:64-94)
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


def mask_words(mask):
    return [sum(int(mask[i, j]) << j for j in range(mask.shape[1])) for i in range(mask.shape[0])]


# ------------------------------------------------------------------------------------------ the cases (inputs + reference, made once)
DTS = (F32, BF16)
EDGES = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
PROBE_TILES = ("first", "middle", "last_full", "ragged", "row0", "rowlast")
PROBE_KINDS = ("fwd", "dq", "dkdv")


def tile_range(name, n):
    """(lo, hi) of the spotlighted rows among n rows in 64-row tiles"""
    nt = (n + KT - 1) // KT
    if name == "first":
        return 0, min(KT, n)
    if name == "middle":
        return KT * (nt // 2), min(KT * (nt // 2) + KT, n)
    if name == "last_full":
        t = max(n // KT - 1, 0)
        return KT * t, min(KT * t + KT, n)
    if name == "ragged":
        lo = KT * (n // KT) if n % KT else n - KT
        return lo, n
    if name == "row0":
        return 0, 1
    assert name == "rowlast", name
    return n - 1, n


@dataclasses.dataclass(frozen=True)
class Case:
    """one launch: B samples of N rows.  probe = (kind, tile): zero all but the spotlighted rows of one operand (see
    probe_ranges); outlier = (sample, row, head): that key row scaled to a norm of ~60; amp: scale of q | k | v."""
    name: str
    N: int
    B: int
    kv: tuple = None
    packed: bool = False
    mask: str = None
    probe: tuple = None
    outlier: tuple = None
    fwd_only: bool = False
    amp: float = 1.0

    def rows(self, b):
        """(query rows, key rows) of sample b"""
        kvl = self.N if self.kv is None else min(self.kv[b], self.N)
        nq = max(kvl, 0) if self.packed else self.N
        return nq, (nq if kvl <= 0 else kvl)


def probe_ranges(c):
    """per sample the spotlighted rows of a probe case: keys for the `fwd` / `dq` probes, queries for `dkdv`"""
    kind, tile = c.probe
    return [tile_range(tile, c.rows(b)[0 if kind == "dkdv" else 1]) for b in range(c.B)]


OUTLIER_NORM = 60.0


@functools.lru_cache(maxsize=None)
def inputs(c, dt):
    """qkv, res, d_o of a case, rounded to the compute type"""
    g = torch.Generator().manual_seed(sum(map(ord, c.name)) * 7919 + c.N)
    qkv = torch.randn(c.B, c.N, 3 * DM, generator=g) * c.amp
    res = torch.randn(c.B, c.N, DM, generator=g)
    d_o = torch.randn(c.B, c.N, DM, generator=g)
    if c.outlier is not None:
        b, row, hd = c.outlier
        kr = qkv[b, row, DM + DH * hd:DM + DH * (hd + 1)]
        kr *= OUTLIER_NORM / kr.norm()
    if c.probe is not None:
        kind = c.probe[0]
        for b, (lo, hi) in enumerate(probe_ranges(c)):
            t, c0 = {"fwd": (qkv, 2 * DM), "dq": (qkv, DM), "dkdv": (d_o, 0)}[kind]
            t[b, :lo, c0:c0 + DM] = 0
            t[b, hi:, c0:c0 + DM] = 0
    return dict(qkv=rnd(qkv, dt), res=rnd(res, dt), d_o=rnd(d_o, dt))


def _model(c, dt, ft, bounded, drop=False):
    x = inputs(c, dt)
    kw = {}
    if bounded and c.outlier is not None:
        bounded = knorm_bodies(c)
    if drop:
        kw["drop_q" if c.probe[0] == "dkdv" else "drop_k"] = probe_ranges(c)
    return attention_model(x["qkv"], c.kv, None if c.fwd_only else x["d_o"], x["res"], dt=dt, ft=ft, packed=c.packed,
                           mask=None if c.mask is None else MASKS[c.mask], bounded=bounded, **kw)


@functools.lru_cache(maxsize=None)
def reference(c, dt):
    """float64 outputs on the live rows (the same for both forward bodies)"""
    return flat(_model(c, dt, F64, False))


@functools.lru_cache(maxsize=None)
def chain(c, dt, bounded=False):
    """working-precision outputs on the live rows; bounded: the forward was given the key-norm table"""
    return flat(_model(c, dt, F32, bounded))


@functools.lru_cache(maxsize=None)
def e_chain(c, dt, bounded=False):
    """{output: err(working-precision chain, float64 chain)}"""
    ref, ch = reference(c, dt), chain(c, dt, bounded)
    return {k: err(ch[k], ref[k]) for k in ref}


def row_sets(c):
    """(qrows, krows) bool[B, N] of a case: the rows flat() selects"""
    q, k = torch.zeros(c.B, c.N, dtype=torch.bool), torch.zeros(c.B, c.N, dtype=torch.bool)
    for b in range(c.B):
        nq, nk = c.rows(b)
        q[b, :nq] = True
        k[b, :nk] = True
    return q, k


@functools.lru_cache(maxsize=None)
def dropped(c, dt):
    """float64 outputs of a probe case with the spotlighted tile's term removed"""
    return flat(_model(c, dt, F64, False, drop=True))


PROBE_OUT = {"fwd": ("o",), "dq": ("dq",), "dkdv": ("dk", "dv")}
PROBE_BODIES = {"fwd": (False, True), "dq": (True,), "dkdv": (True,)}     # forward bodies a probe runs with (True: the bounded one)
PROBE_SHAPES = ((300, False, DTS), (300, True, DTS), (1537, False, (BF16,)))     # N, packed, compute types
PROBE_AMP = 0.5          # |score| ~ 0.25 rms: the single-term outputs of the one-row probes keep e_chain small (bound <= 0.25)


def probe_case(kind, tile, N, packed):
    kv = None
    if packed:
        kv = (N, 170) if N == 300 else (N,)
    return Case(f"probe_{kind}_{tile}", N, 2 if N == 300 else 1, kv=kv, packed=packed, probe=(kind, tile), amp=PROBE_AMP,
                fwd_only=kind == "fwd")


# a. dense, at every loop edge
DENSE_CASES = [Case("padded257", 257, 14, kv=(0,) + EDGES)]
DENSE_CASES += [Case(f"nomask{n}", n, 2) for n in (1, 64, 65, 128, 129, 256, 257)]
DENSE_CASES += [Case("packed300", 300, 14, kv=EDGES + (300,), packed=True)]
PREFIX_CASES = [Case("prefix_v16", 20, 3, kv=(16, 17, 20), mask="v16"), Case("prefix_i12", 61, 3, mask="i12"),
                Case("prefix_t12", 140, 3, kv=(12, 13, 140), mask="t12")]
# b. the 64-key backward (N >= 1536, bf16)
LONG_CASES = [Case("long1536", 1536, 1), Case("long1537", 1537, 1), Case("long1600", 1600, 1, kv=(1500,)),
              Case("long_packed", 1536, 9, kv=(1536, 1, 63, 64, 65, 255, 256, 257, 1281), packed=True),
              Case("long_uniform", 1536, 2, kv=(0, 1536)),
              Case("long_prefix", 1536, 1, kv=(1500,), mask="v16")]
GROUPS = {"g54_133": [Case("grp_a_v", 1536, 2), Case("grp_a_i", 54, 2), Case("grp_a_t", 133, 2, kv=(133, 4))],
          "g128_200": [Case("grp_b_v", 1536, 2), Case("grp_b_i", 128, 2), Case("grp_b_t", 200, 2, kv=(200, 4))]}
# d. key-norm table edges: one key of head 1 with ||k|| ~ 60 -- every wave of that head leaves the bounded body
KNORM_HEAD = 1
KNORM_CASES = [Case("knorm2100", 2100, 1, outlier=(0, 2090, KNORM_HEAD), fwd_only=True),
               Case("knorm_packed_last", 2100, 3, kv=(45, 2100, 7), packed=True, outlier=(1, 2099, KNORM_HEAD), fwd_only=True),
               Case("knorm_packed_first", 2100, 3, kv=(45, 2100, 7), packed=True, outlier=(1, 0, KNORM_HEAD), fwd_only=True)]


def knorm_bodies(c):
    """per sample the forward body of each head (True = bounded) when the key-norm table is given: a sample whose table blocks
    hold the outlier key takes the online body in that head (packed: blocks are 32 rows of the PACKED buffer, so a neighbour
    that shares the outlier's block falls back too)"""
    starts = [0]
    for b in range(c.B):
        starts.append(starts[-1] + (c.rows(b)[0] if c.packed else c.N))
    ob, orow, ohd = c.outlier
    blk = (starts[ob] + orow) >> 5
    res = []
    for b in range(c.B):
        hit = (starts[b] >> 5) <= blk <= ((starts[b + 1] - 1) >> 5) and starts[b + 1] > starts[b]
        res.append([not (hit and hd == ohd) for hd in range(H)])
    return res


# e. CLS-row kernels: 256 threads walk the keys (k += 256: edges 256, 512), 32 key lanes walk them again (k += 32: edge 32)
CLS_N = 600
CLS_LENS = (5, 31, 32, 33, 63, 64, 65, 255, 256, 257, 512, 513, 600)


@functools.lru_cache(maxsize=None)
def cls_case(cls_tok, packed, dt):
    lens = CLS_LENS if packed else CLS_LENS + (0,)
    B = len(lens)
    g = torch.Generator().manual_seed(500 + cls_tok + 10 * packed)
    qkv = rnd(torch.randn(B, CLS_N, 3 * DM, generator=g) * 0.7, dt)
    z = rnd(torch.randn(B, CLS_N, DM, generator=g), dt)
    d_o = rnd(torch.randn(B, DM, generator=g), dt)
    ref = flat_cls(attn_cls_model(qkv, z, lens, d_o, cls_tok, dt=dt, ft=F64, packed=packed))
    ch = flat_cls(attn_cls_model(qkv, z, lens, d_o, cls_tok, dt=dt, ft=F32, packed=packed))
    return dict(qkv=qkv, z=z, d_o=d_o, lens=lens, ref=ref, e_chain={k: err(ch[k], ref[k]) for k in ref})


def long_stream_drop_figures():
    """per dense single-stream long case and output (dk, dv): err of the float64 result without the last query tile's term,
    and the bound of that check"""
    rows = []
    for c in LONG_CASES[:3]:
        x = inputs(c, BF16)
        drop = [tile_range("ragged", c.rows(b)[0]) for b in range(c.B)]
        lost = flat(attention_model(x["qkv"], c.kv, x["d_o"], x["res"], dt=BF16, ft=F64, drop_q=drop))
        ref, e = reference(c, BF16), e_chain(c, BF16, True)
        for name in ("dk", "dv"):
            rows.append(dict(case=c.name, name=name, moved=err(lost[name], ref[name]), bound=bound(e[name], True), rows=drop[0][1] - drop[0][0]))
    return rows


def single_key(c):
    """every sample of the launch has exactly one key: dq and dk are zero by cancellation (see single_key_noise)"""
    return all(c.rows(b)[1] == 1 and (c.kv is None or c.kv[b] > 0) for b in range(c.B))


def single_key_noise(c, dt):
    """Element-wise limits for dq and dk of a launch whose samples all have ONE key (N = 1).  There p = 1 and dS = p (dO.v - delta)
    is a difference of two sums of the same 64 products, so the float64 dq and dk are identically zero, err() has no scale and
    what a kernel returns is the round-off of that cancellation.  Each fp32 sum of 64 products is within 64 * 2^-24 * sum |dO v|
    of the exact value whatever its order, hence |dS| <= p * 2 * 64 * 2^-24 * sum_d |dO_d v_d|, |dq| <= |dS| |k| / 8 and
    |dk| <= sum over the queries of |dS| |q| / 8.  bf16 adds, from the chain's rounding points: the bounded forward body divides
    bf16(p) v by the unrounded l = p and stores O in bf16 (F2, F3: O = v (1 + e), |e| <= 2 * 2^-9), which delta inherits (Q2) and
    dO.v does not; p = exp2(q'.k - lse) is recomputed from rounded operands and is not exactly 1 (a score moves by far less
    than 1: p <= 2); dS and the stored result are rounded once each (1 + 2^-7)."""
    assert single_key(c), "only for launches whose samples have one key each"
    x = inputs(c, dt)
    gam = 2 * DH * 2.0 ** -24
    if dt == BF16:
        gam = (gam + 2 * 2.0 ** -9) * 2.0 * (1 + 2.0 ** -7)
    out = dict(dq=torch.zeros(c.B, c.N, DM, dtype=F64), dk=torch.zeros(c.B, c.N, DM, dtype=F64))
    for b in range(c.B):
        nq, nk = c.rows(b)
        row = x["qkv"][b].to(F64)
        q, k, v = _heads(row[:nq, :DM]), _heads(row[:1, DM:2 * DM]), _heads(row[:1, 2 * DM:])
        dS = gam * (_heads(x["d_o"][b, :nq].to(F64)).abs() * v.abs()).sum(-1, keepdim=True)          # [4, nq, 1]
        out["dq"][b, :nq] = _merge(SCALE * dS * k.abs())
        out["dk"][b, :1] = _merge((SCALE * dS * q.abs()).sum(1, keepdim=True))
    qrows, krows = row_sets(c)
    return dict(dq=out["dq"][qrows], dk=out["dk"][krows])
