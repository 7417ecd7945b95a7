"""-m gpu: the attention kernels of csrc/attention.hip against the float64 model of tests/attention_model.py, element by element:
every loop edge of the forward, dQ and dK / dV kernels in both layouts and both forward bodies, the 64-key backward of long
streams (alone, packed, and with short streams in the same launch), one-tile probes, the key-norm table of samples of more than
2048 rows, and the CLS-row pair.  Metric and bound: see attention_model.py -- every output tensor of a launch (live rows only) meets
max(8 e_chain, 16 * 2^-24) (+ 2^-8 for a bf16 output), e_chain being the error of the working-precision chain on the CPU; nothing is
fitted to what the kernels return.  Inputs are rounded to the compute type on both sides; dead rows of packed buffers are NaN.
Every check appends {err, e_chain, bound} to a report: build/attention_model_report.json, or the file MTMP_ATTENTION_REPORT names.
"""
import contextlib
import json
import math
import os

import pytest
import torch

from tests import attention_model as A

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
REPORT = {}
SENTINEL = 768.0                       # (exact in bf16) what the wrappers' output buffers hold before a launch


@pytest.fixture(scope="module")
def ops():
    from medical_tri_modal_pilot_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module", autouse=True)
def _dump_report():
    yield
    path = os.environ.get("MTMP_ATTENTION_REPORT") or os.path.join(ROOT, "build", "attention_model_report.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


class Checks:
    """collects the checks of one test: every figure is printed and recorded before the test asserts"""

    def __init__(self, tag):
        self.tag, self.failed = tag, []

    def close(self, name, got, ref, e_chain, bf16_out=False):
        e, b = A.err(got, ref), A.bound(e_chain, bf16_out)
        key = f"{self.tag}.{name}"
        assert key not in REPORT, key
        REPORT[key] = {"err": e, "e_chain": e_chain, "bound": b}
        print(f"{key}: err {e:.3e} e_chain {e_chain:.3e} bound {b:.3e} ratio {e / b:.3f}")
        if not (math.isfinite(e) and e <= b):
            self.failed.append(f"{key}: err {e:.3e} > bound {b:.3e} (e_chain {e_chain:.3e})")

    def noise(self, name, got, limit):
        """an output whose float64 reference is identically zero: element-wise against the limits of the cancellation's round-off"""
        got, key = got.detach().to("cpu", F64).abs(), f"{self.tag}.{name}"
        worst = float(torch.where(limit > 0, got / limit.clamp_min(1e-300), torch.where(got > 0, math.inf, 0.0).to(F64)).max())
        REPORT[key] = {"err": worst, "e_chain": 0.0, "bound": 1.0, "zero_reference": True}
        print(f"{key}: zero reference, max |got| {float(got.max()):.3e}, worst |got| / limit {worst:.3f}")
        if not worst <= 1.0:
            self.failed.append(f"{key}: |got| / limit {worst:.3e} > 1 where the reference is identically zero")

    def done(self):
        assert not self.failed, "\n".join(self.failed)


def dn(dt):
    return A.dt_name(dt)


def body(bounded):
    return "bounded" if bounded else "online"


@contextlib.contextmanager
def sentinel_outputs():
    """the buffers that the wrappers allocate for a launch start out as SENTINEL, so a row the kernels do not write shows"""
    empty, empty_like = torch.empty, torch.empty_like
    fill = lambda t: t.fill_(SENTINEL) if t.is_floating_point() else t
    torch.empty = lambda *a, **k: fill(empty(*a, **k))
    torch.empty_like = lambda *a, **k: fill(empty_like(*a, **k))
    try:
        yield
    finally:
        torch.empty, torch.empty_like = empty, empty_like


def _pack_rows(t, kv, pack):
    """padded [B, N, C] -> the packed layout inside a same-sized buffer (rows behind the live ones poisoned)"""
    B, N, C = t.shape
    out = torch.full((B * N, C), float("nan"), dtype=t.dtype, device=t.device)
    for b in range(B):
        out[int(pack[b]):int(pack[b]) + int(kv[b])] = t[b, :int(kv[b])]
    return out.view(B, N, C)


def _unpack_rows(t, kv, pack):
    B, N, C = t.shape
    out = torch.zeros(B, N, C, dtype=t.dtype, device=t.device)
    flat = t.reshape(B * N, C)
    for b in range(B):
        out[b, :int(kv[b])] = flat[int(pack[b]):int(pack[b]) + int(kv[b])]
    return out


def run(ops, cases, dt, bounded):
    """ONE forward launch and one backward (dQ, dK / dV) over the streams `cases` -> per stream the outputs on the live rows
    (attention_model.flat's row sets, float64 on the CPU) and the padded forward outputs `o`, `o_res`, `lse` for bit comparisons.
    Asserts on the way: rows behind a packed stream's live rows are untouched in every output; dK / dV of keys at or behind
    kv_len (padded layout) are exactly zero."""
    qs, rs, ws, kvs, packs, kns, mws = [], [], [], [], [], [], []
    for c in cases:
        x = A.inputs(c, dt)
        kv = None if c.kv is None else torch.tensor(c.kv, dtype=torch.int32, device=DEV)
        q, r_, w = (x[k].to(DEV, dt) for k in ("qkv", "res", "d_o"))
        pack = None
        if c.packed:
            pack = ops.row_starts(kv, c.N)
            q, r_, w = (_pack_rows(t, c.kv, pack.cpu()) for t in (q, r_, w))
        qs.append(q), rs.append(r_), ws.append(torch.nan_to_num(w)), kvs.append(kv), packs.append(pack)
        kns.append(ops.key_norms(torch.nan_to_num(q)) if bounded else None)     # (the table is taken over the buffer's rows)
        mws.append(None if c.mask is None else A.mask_words(A.MASKS[c.mask]))
    pk = packs if any(p is not None for p in packs) else None
    mk = mws if any(m is not None for m in mws) else None
    fwd_only = cases[0].fwd_only
    with sentinel_outputs():
        o, o_res, lse = ops.attn_fwd_grouped(qs, kvs, rs, kns, pk, qk_masks=mk)
        dqkv = None if fwd_only else ops.attn_bwd_grouped(qs, o, ws, lse, kvs, pk, qk_masks=mk)
    torch.cuda.synchronize()
    res = []
    for i, c in enumerate(cases):
        qrows, krows = A.row_sets(c)
        pad = dict(o=o[i], o_res=o_res[i])
        if dqkv is not None:
            pad.update(dq=dqkv[i][..., :256], dk=dqkv[i][..., 256:512], dv=dqkv[i][..., 512:])
        if c.packed:
            pc, live = packs[i].cpu(), int(packs[i][c.B])
            assert pc[:c.B + 1].tolist() == [0] + torch.tensor(c.kv).clamp(0, c.N).cumsum(0).tolist()
            for name, t in pad.items():
                dead = t.reshape(c.B * c.N, -1)[live:].float()
                assert bool((dead == SENTINEL).all()), f"{c.name}.{name}: rows behind the live ones were written"
            assert bool((lse[i].transpose(1, 2)[~qrows.to(DEV)] == SENTINEL).all()), f"{c.name}.lse: entries of rows that do not exist were written"
            pad = {k: _unpack_rows(t, c.kv, pc) for k, t in pad.items()}
        pad = {k: t.detach().to("cpu", F64) for k, t in pad.items()}
        pad["lse"] = lse[i].detach().to("cpu", F64)
        if dqkv is not None and not c.packed:
            for name in ("dk", "dv"):
                assert float(pad[name][~krows].abs().max() if bool((~krows).any()) else 0.0) == 0.0, f"{c.name}.{name}: keys behind kv_len"
        got = A.flat(dict(pad, qrows=qrows, krows=krows))
        res.append(dict(got=got, o=o[i], o_res=o_res[i], lse=lse[i]))
    return res


def check_all(ck, c, dt, bounded, got, prefix="", names=None):
    ref, e = A.reference(c, dt), A.e_chain(c, dt, bounded)
    for name in names or [n for n in A.DENSE_OUT if n in ref]:
        assert bool(torch.isfinite(got[name]).all()), f"{c.name}.{name}: not finite"
        if name in ("dq", "dk") and A.single_key(c):                             # (N = 1: see attention_model.single_key_noise)
            ck.noise(prefix + name, got[name], A.single_key_noise(c, dt)[name])
            continue
        ck.close(prefix + name, got[name], ref[name], e[name], dt == BF16 and name != "lse")


# ------------------------------------------------------------------------------------------ a. dense, at every loop edge
@pytest.mark.parametrize("bounded", [False, True], ids=body)
@pytest.mark.parametrize("dt", A.DTS, ids=dn)
@pytest.mark.parametrize("c", A.DENSE_CASES + A.PREFIX_CASES, ids=lambda c: c.name)
def test_dense_at_every_loop_edge(ops, c, dt, bounded):
    """Key lengths 0 / 1 and both sides of 32, 64, 128, 256 as samples of one launch (padded: 257 live queries each; packed: the
    sample's own rows), N on both sides of the 64-row tile, the 128-row backward and the 256-row forward workgroups, and the three
    prefix masks at their smallest N: o, o_res, lse, dq, dk, dv each against its own bound."""
    r = run(ops, [c], dt, bounded)[0]
    ck = Checks(f"dense.{c.name}[{dn(dt)},{body(bounded)}]")
    check_all(ck, c, dt, bounded, r["got"])
    ck.done()


# ------------------------------------------------------------------------------------------ b. the 64-key backward (bf16, N >= 1536)
@pytest.mark.parametrize("c", A.LONG_CASES, ids=lambda c: c.name)
def test_long_stream_64_key_backward(ops, c):
    """attn_bwd_dkdv64_kernel element by element: six full workgroups (1536), a one-key workgroup and a one-row query tile (1537),
    kv_len inside the last workgroup (1600 / 1500), a packed stream whose samples leave whole waves and workgroups without a live
    key, the `uniform` path (kv_len 0) and the prefix-masked instantiation -- there also the prefix's own rows and keys 0..15 as
    tensors of their own, so that their scale is the prefix's and not the stream's."""
    dt, bounded = BF16, True
    r = run(ops, [c], dt, bounded)[0]
    ck = Checks(f"long.{c.name}[bf16]")
    check_all(ck, c, dt, bounded, r["got"])
    if c.mask is not None:
        P = A.MASKS[c.mask].shape[0]
        ref, ch = A.reference(c, dt), A.chain(c, dt, bounded)
        for name in ("o", "dq", "dk", "dv"):                        # (B = 1: the first P live rows are rows 0..P-1)
            ck.close(f"{name}[:{P}]", r["got"][name][:P], ref[name][:P], A.err(ch[name][:P], ref[name][:P]), True)
    ck.done()


@pytest.mark.parametrize("gname", list(A.GROUPS), ids=str)
def test_short_streams_inside_a_long_launch(ops, gname):
    """A grouped backward whose longest stream has N >= 1536 sends EVERY stream through the 64-key kernel: the short ones run as one
    partly filled 256-key workgroup with 1..4 query tiles against a three-stage ring.  Every stream against the model (no
    bit-equality with single launches: those take the 32-key kernel)."""
    dt, bounded = BF16, True
    cases = A.GROUPS[gname]
    ck = Checks(f"group.{gname}[bf16]")
    for c, r in zip(cases, run(ops, cases, dt, bounded)):
        check_all(ck, c, dt, bounded, r["got"], prefix=f"{c.name}.")
    ck.done()


# ------------------------------------------------------------------------------------------ c. one-tile probes
def _probes():
    for kind in A.PROBE_KINDS:
        for tile in A.PROBE_TILES:
            for N, packed, dts in A.PROBE_SHAPES:
                for dt in dts:
                    yield pytest.param(kind, tile, N, packed, dt, id=f"{kind}-{tile}-{N}{'p' if packed else ''}-{dn(dt)}")


@pytest.mark.parametrize("kind,tile,N,packed,dt", list(_probes()))
def test_one_tile_probe(ops, kind, tile, N, packed, dt):
    """All but one 64-row tile (or one row) of one operand is zero, so an output is that tile's term alone: V for the forward
    (O = sum over the tile's keys of p v), K for dQ (dQ = scale * sum over the tile's keys of dS k), dO for dK / dV (only the
    tile's queries have non-zero delta, dP and dS).  tests/test_attention_model_cpu.py proves on the reference that losing the
    tile costs err >= 0.5 against a bound <= 0.25.  N 1537 (bf16) goes through the 64-key backward."""
    c = A.probe_case(kind, tile, N, packed)
    ck = Checks(f"probe.{kind}.{tile}[N={N},{'packed' if packed else 'padded'},{dn(dt)}]")
    for bounded in A.PROBE_BODIES[kind]:
        r = run(ops, [c], dt, bounded)[0]
        check_all(ck, c, dt, bounded, r["got"], prefix=f"{body(bounded)}.", names=A.PROBE_OUT[kind])
    ck.done()


# ------------------------------------------------------------------------------------------ d. key-norm table edges (forward)
@pytest.mark.parametrize("dt", A.DTS, ids=dn)
@pytest.mark.parametrize("c", A.KNORM_CASES, ids=lambda c: c.name)
def test_key_norm_table_of_long_samples(ops, c, dt):
    """A sample of 2100 rows has 66 table blocks: a wave's 64 lanes take the first 64, the `+ 64` walk the rest.  One key of head 1
    in a block that only the walk reaches (or, packed, in the sample's last / first row, the first row not a multiple of 32) has
    ||k|| ~ 60: every wave of that head must leave the bounded body, so head 1 of the call with the table is the online call to the
    bit; all outputs of both calls meet their bounds."""
    ck = Checks(f"knorm.{c.name}[{dn(dt)}]")
    rs = {}
    for bounded in (False, True):
        rs[bounded] = r = run(ops, [c], dt, bounded)[0]
        check_all(ck, c, dt, bounded, r["got"], prefix=f"{body(bounded)}.")
    b, _, hd = c.outlier
    assert A.knorm_bodies(c)[b][hd] is False
    live = A.row_sets(c)[0].reshape(-1).to(DEV)
    if c.packed:                                                      # rows of sample b inside the packed buffer
        start = sum(c.rows(i)[0] for i in range(b))
        live = torch.zeros_like(live)
        live[start:start + c.rows(b)[0]] = True
    else:
        live = live & (torch.arange(c.B * c.N, device=DEV) // c.N == b)
    cols = slice(64 * hd, 64 * hd + 64)
    for name in ("o", "o_res"):
        x, y = (rs[k][name].reshape(c.B * c.N, 256)[live][:, cols] for k in (True, False))
        assert torch.equal(x, y), f"{name}: head {hd} of the bounded call is not the online call"
    nq = c.rows(b)[0]
    assert torch.equal(rs[True]["lse"][b, hd, :nq], rs[False]["lse"][b, hd, :nq])
    ck.done()


# ------------------------------------------------------------------------------------------ e. CLS-row kernels
@pytest.mark.parametrize("dt", A.DTS, ids=dn)
@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
@pytest.mark.parametrize("cls_tok", [0, 4])
def test_cls_row_kernels(ops, cls_tok, packed, dt):
    """attn_cls_fwd_kernel / attn_cls_bwd_kernel: key counts on both sides of the 256-thread score loop's trips (256, 512), of the
    32-key-lane walk (32) and of 64, the all-masked sample in the padded layout: o, r1, lse and the three gradient thirds."""
    c = A.cls_case(cls_tok, packed, dt)
    lens, N, B = c["lens"], A.CLS_N, len(c["lens"])
    kv = torch.tensor(lens, dtype=torch.int32, device=DEV)
    qkv, z, d_o = c["qkv"].to(DEV, dt), c["z"].to(DEV, dt), c["d_o"].to(DEV, dt)
    pack = pc = None
    if packed:
        pack = ops.row_starts(kv, N)
        pc = pack.cpu()
        qkv, z = _pack_rows(qkv, lens, pc), _pack_rows(z, lens, pc)
    with sentinel_outputs():
        o, r1, lse = ops.attn_cls_fwd(qkv, z, kv, pack, cls_tok)
        dqkv = ops.attn_cls_bwd(qkv, o, d_o, lse, kv, pack, cls_tok)
    torch.cuda.synchronize()
    if packed:
        assert bool((dqkv.reshape(B * N, 768)[int(pack[B]):].float() == SENTINEL).all()), "rows behind the live ones were written"
        dqkv = _unpack_rows(dqkv, lens, pc)
    dqkv = dqkv.detach().to("cpu", F64)
    krows = torch.arange(N)[None, :] < torch.tensor([n if n > 0 else N for n in lens])[:, None]
    rows = krows if packed else torch.ones(B, N, dtype=torch.bool)                     # rows of the dense gradient buffers
    assert bool(torch.isfinite(dqkv[rows]).all())
    other = rows.clone()
    other[:, cls_tok] = False
    assert float(dqkv[..., :256][other].abs().max()) == 0.0, "dq outside the CLS row"
    if not packed:
        assert float(dqkv[..., 256:][~krows].abs().max()) == 0.0, "dk / dv of keys behind kv_len"
    got = dict(o=o, r1=r1, lse=lse, dq=dqkv[:, cls_tok, :256], dk=dqkv[..., 256:512][krows], dv=dqkv[..., 512:][krows])
    ck = Checks(f"cls[tok={cls_tok},{'packed' if packed else 'padded'},{dn(dt)}]")
    for name in A.CLS_OUT:
        ck.close(name, got[name], c["ref"][name], c["e_chain"][name], dt == BF16 and name != "lse")
    ck.done()
