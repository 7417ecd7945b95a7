"""-m gpu: the row-streaming kernels of csrc/elementwise.hip and the slab reductions of csrc/gemm.hip against the float64 models of
tests/row_kernels_model.py, element by element, at every shape where their grid-stride loops, row prefetch and reduction trees
change form (the thresholds are those of the launch code).  Metric and bound: see row_kernels_model.py -- the bound of every check
is max(8 e_torch, 16 * 2^-24) (+ 2^-8 for a bf16 output) with e_torch the error of the same torch chain in fp32 on the CPU; nothing
is fitted to what the kernels return.  Only valid calls are made; dropout is off throughout.
Every check appends {err, e_torch, bound} to a report: build/row_kernels_report.json, or the file MTMP_ROW_KERNELS_REPORT names.
"""
import ctypes
import json
import math
import os

import pytest
import torch

from tests import row_kernels_model as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
DT = [F32, BF16]
REPORT = {}


@pytest.fixture(scope="module")
def ops():
    from medical_tri_modal_pilot_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module", autouse=True)
def _dump_report():
    yield
    path = os.environ.get("MTMP_ROW_KERNELS_REPORT") or os.path.join(ROOT, "build", "row_kernels_report.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


class Checks:
    """collects the checks of one test: every figure is printed and recorded before the test asserts"""

    def __init__(self, tag):
        self.tag, self.failed = tag, []

    def close(self, name, got, ref, e_torch, bf16_out=False):
        e, b = R.err(got, ref), R.bound(e_torch, bf16_out)
        self.record(name, e, e_torch, b)

    def record(self, name, e, e_torch, b):
        key = f"{self.tag}.{name}"
        assert key not in REPORT, key
        REPORT[key] = {"err": e, "e_torch": e_torch, "bound": b}
        print(f"{key}: err {e:.3e} e_torch {e_torch:.3e} bound {b:.3e} ratio {e / b:.3f}")
        if not (math.isfinite(e) and e <= b):
            self.failed.append(f"{key}: err {e:.3e} > bound {b:.3e} (e_torch {e_torch:.3e})")

    def done(self):
        assert not self.failed, "\n".join(self.failed)


def dn(dt):
    return R.dt_name(dt)


def dev(t, dt=None):
    return None if t is None else (t.to(DEV) if dt is None else t.to(DEV, dt))


# ------------------------------------------------------------------------------------------ custom LayerNorm backward
@pytest.mark.parametrize("dt", DT, ids=dn)
@pytest.mark.parametrize("M,variant", R.LN_CASES)
def test_ln_bwd(ops, dt, M, variant):
    """grid min(ceil(M / 16), 2048), 16 rows per block and trip, single-level reduce while blocks <= 64: M = 1024 is the last
    single-level size, 1025 the first two-level one, 32787 = 32768 + 19 a second trip with a ragged end."""
    c = R.ln_case(M, variant, dt)
    z, dres = dev(c["z"], dt), dev(c["d_res"], dt)
    if variant == "ldz320":
        buf = torch.full((M, 320), 7.0, device=DEV, dtype=dt)
        buf[:, :256] = z
        z = buf[:, :256]
    if variant == "ldr264":
        buf = torch.full((M, 264), -3.0, device=DEV, dtype=dt)
        buf[:, :256] = dres
        dres = buf[:, :256]
    dz, dg, db = ops.ln_bwd(z, dev(c["stats"]), dev(c["gamma"]), dev(c["dy"], dt), dres)
    ck = Checks(f"ln_bwd[{M},{variant},{dn(dt)}]")
    ck.close("dz", dz, c["ref"]["dz"], c["e_torch"]["dz"], dt == BF16)
    ck.close("dgamma", dg, c["ref"]["dgamma"], c["e_torch"]["dgamma"])
    ck.close("dbeta", db, c["ref"]["dbeta"], c["e_torch"]["dbeta"])
    ck.done()


# ------------------------------------------------------------------------------------------ stream input
def _stream_run(ops, c, dt, packed=False, flat=False):
    B, N, _ = c["x"].shape
    nb = 0 if c["bott"] is None else c["bott"].shape[-2]
    Rr = nb + 1 + N
    xd = dev(c["x"], dt).requires_grad_()
    mk = (lambda t: torch.nn.Parameter(dev(t))) if flat else (lambda t: dev(t).requires_grad_())
    cd, gd, bd = mk(c["cls"]), mk(c["gamma"]), mk(c["beta"])
    td = None if c["bott"] is None else dev(c["bott"]).requires_grad_()
    fp = None
    if flat:
        from medical_tri_modal_pilot_amd.optim import FlatParams
        fp = FlatParams([("cls", cd), ("w", gd), ("b", bd)])
        fp.zero_grad()
    live = c["ref"]["live"]
    if packed:
        kv = dev(c["kv_len"])
        pack = ops.row_starts(kv, Rr)
        starts = torch.cat([torch.zeros(1, dtype=torch.int64), c["kv_len"].long().cumsum(0)])
        assert pack[:B].cpu().tolist() == starts[:B].tolist() and int(pack[B]) == int(starts[B])
        z = ops.StreamInputFn.apply(xd, cd, gd, bd, dev(c["pe"]), td, 1e-5, 0.0, 0, pack, kv)
        rows = torch.cat([starts[b] + torch.arange(int(c["kv_len"][b])) for b in range(B)]).to(DEV)
        z_live = z.view(-1, 256)[rows]
    else:
        z = ops.StreamInputFn.apply(xd, cd, gd, bd, dev(c["pe"]), td, 1e-5, 0.0, 0)
        z_live = z[dev(live)]
    assert z.dtype == dt and z.shape == (B, Rr, 256)
    (z_live.float() * dev(c["w"][live])).sum().backward()
    if flat:
        assert fp.written == {0, 1, 2}, "the gradients did not take the partial-slab + reduce_scatter path"
    grads = dict(dx=xd.grad, dcls=cd.grad.view(-1), dgamma=gd.grad, dbeta=bd.grad)
    if td is not None:
        grads["dbott"] = td.grad.view(nb, 256)
    return z_live.detach(), grads


def _stream_checks(ck, c, dt, z_live, grads):
    ref, et = c["ref"], c["e_torch"]
    ck.close("z", z_live, ref["z"][ref["live"]], et["z"], dt == BF16)
    ck.close("dx", grads["dx"], ref["dx"], et["dx"], dt == BF16)
    for k in ("dcls", "dgamma", "dbeta", "dbott"):
        if k in ref:
            assert grads[k].dtype == F32
            ck.close(k, grads[k], ref[k], et[k])


@pytest.mark.parametrize("dt", DT, ids=dn)
@pytest.mark.parametrize("B,N,nb,use_pe", R.STREAM_CASES)
def test_stream_input(ops, dt, B, N, nb, use_pe):
    """rows = B (nb + 1 + N); forward 4 rows per block up to 2048 blocks (8192 rows), backward 16 rows per block up to 1024 blocks with
    two rows in flight, two-level reduce above 1024 rows: 1057 rows is past the reduce threshold, 17025 past both caps."""
    c = R.stream_case(B, N, nb, use_pe, dt)
    z_live, grads = _stream_run(ops, c, dt)
    ck = Checks(f"stream_in[{B}x{N}+{nb},{dn(dt)}]")
    _stream_checks(ck, c, dt, z_live, grads)
    ck.done()


@pytest.mark.parametrize("dt", DT, ids=dn)
def test_stream_input_flat_gradient_path(ops, dt):
    """the same node with its parameters in optim.FlatParams: partial slab + ONE mtmp_reduce_scatter into the flat gradient"""
    c = R.stream_case(7, 146, 4, False, dt)
    z_live, grads = _stream_run(ops, c, dt, flat=True)
    ck = Checks(f"stream_in_flat[7x146+4,{dn(dt)}]")
    _stream_checks(ck, c, dt, z_live, grads)
    ck.done()


@pytest.mark.parametrize("dt", DT, ids=dn)
@pytest.mark.parametrize("flat", [False, True], ids=["grads", "flat"])
def test_stream_input_packed(ops, dt, flat):
    """kv_len 42 = a full sample, 5 = bottleneck + CLS rows only (the shortest the trainer produces): live output rows against the
    model, dx exactly zero on pad tokens, every parameter gradient over live rows only"""
    B, N, nb, kv = R.STREAM_PACKED
    c = R.stream_case(B, N, nb, False, dt, kv)
    z_live, grads = _stream_run(ops, c, dt, packed=True, flat=flat)
    pad_tok = ~c["ref"]["live"][:, nb + 1:]
    assert int(pad_tok.sum()) == B * N - sum(k - nb - 1 for k in kv)
    assert float(grads["dx"][dev(pad_tok)].float().abs().sum()) == 0.0
    ck = Checks(f"stream_in_packed[{'flat' if flat else 'grads'},{dn(dt)}]")
    _stream_checks(ck, c, dt, z_live, grads)
    ck.done()


# ------------------------------------------------------------------------------------------ TIE / time embedding
def _tie_grad_checks(ck, c, grads):
    for name, g in zip(R.TIE_NAMES, grads):
        assert g.dtype == F32
        ck.close(name, g.reshape(c["ref"][name].shape), c["ref"][name], c["e_torch"][name])


@pytest.mark.parametrize("dt", DT, ids=dn)
@pytest.mark.parametrize("n", R.TIE_SIZES)
def test_tie_embed_all_nine_gradients(ops, dt, n):
    """backward: 4 rows per block up to 512 blocks, four rows in flight at stride 4 * blocks, two-level reduce above 64 blocks (256 /
    257 events); 2049: the second in-flight row is live for one row; 8197: second trip of both directions (forward cap 8192)."""
    c = R.tie_case(n, dt)
    idx = c["ev"][:, 2].long()
    if n >= 5:
        assert int((idx == 0).sum()) >= 1 and int((idx == 19).sum()) >= 1 and int((idx == 5).sum()) == 1
    if n >= 64:
        assert set(idx.tolist()) == set(range(20))
    prm = [dev(p).requires_grad_() for p in c["prm"]]
    emb = ops.TieEmbed.apply(dev(c["ev"]).view(1, n, 3), *prm, dt)
    assert emb.dtype == dt
    (emb.float() * dev(c["w"]).view(1, n, 256)).sum().backward()
    ck = Checks(f"tie[{n},{dn(dt)}]")
    ck.close("out", emb[0], c["ref"]["out"], c["e_torch"]["out"], dt == BF16)
    _tie_grad_checks(ck, c, [p.grad for p in prm])
    ck.done()


@pytest.mark.parametrize("dt", DT, ids=dn)
@pytest.mark.parametrize("n", R.TIME_SIZES)
def test_time_embed(ops, dt, n):
    c = R.tie_case(n, dt, False)
    prm = [dev(p).requires_grad_() for p in c["prm"]]
    emb = ops.TimeEmbed.apply(dev(c["ev"]), *prm[4:], dt)
    (emb.float() * dev(c["w"])).sum().backward()
    ck = Checks(f"time[{n},{dn(dt)}]")
    ck.close("out", emb, c["ref"]["out"], c["e_torch"]["out"], dt == BF16)
    for name, p in zip(R.TIE_NAMES[4:], prm[4:]):
        ck.close(name, p.grad, c["ref"][name], c["e_torch"][name])
    # the kernel's own gradient block: the value chain's four rows are written, and exactly zero
    from medical_tri_modal_pilot_amd import _lib
    z = torch.zeros(256, device=DEV)
    flatp = torch.stack([z, z, z, z, prm[4].detach().reshape(-1), prm[5].detach(), prm[6].detach(), prm[7].detach()]).contiguous()
    grads = torch.full((28, 256), float("nan"), device=DEV)
    ws = torch.empty(_lib.lib().mtmp_tie_bwd_ws_floats(n), dtype=F32, device=DEV)
    d_out = dev(c["w"], dt).contiguous()
    ops.call("mtmp_time_embed_bwd", ops._dt(d_out), ops._p(dev(c["ev"])), ops._p(flatp), ops._p(d_out), ops._p(grads), ops._p(ws), n,
             ops._stream())
    assert float(grads[:4].abs().sum()) == 0.0
    assert torch.equal(grads[4:8].reshape(-1), torch.cat([p.grad.reshape(-1) for p in prm[4:8]])) and torch.equal(grads[8:], prm[8].grad)
    ck.done()


@pytest.mark.parametrize("dt", DT, ids=dn)
def test_tie_embed_packed(ops, dt):
    """the ragged layout (cu_seqlens row map) against the model on the packed events -- not only against the padded call"""
    c = R.tie_packed_case(dt)
    B, T = len(R.TIE_PACKED_LENS), R.TIE_PACKED_TPAD
    prm = [dev(p).requires_grad_() for p in c["prm"]]
    emb = ops.TieEmbedPacked.apply(dev(c["ev"]), dev(c["cu"]), T, *prm, dt)
    assert emb.shape == (B, T, 256) and emb.dtype == dt
    valid = dev(c["valid"])
    assert float(emb.detach()[~valid].float().abs().sum()) == 0.0                 # pad rows are exactly 0
    (emb.float() * dev(c["w"])).sum().backward()                           # (pad rows carry no gradient by construction)
    ck = Checks(f"tie_packed[{dn(dt)}]")
    ck.close("out", emb[valid], c["ref"]["out"], c["e_torch"]["out"], dt == BF16)
    _tie_grad_checks(ck, c, [p.grad for p in prm])
    ck.done()


@pytest.mark.parametrize("dt", DT, ids=dn)
@pytest.mark.parametrize("n,n_time,n_img", R.TIE_TIME_CASES)
def test_tie_time_embed_one_slab(ops, dt, n, n_time, n_img):
    """ops.TieTimeEmbed with its parameters in optim.FlatParams: events and time events in ONE backward launch into one slab (the time
    rows' gradient split 0 / all / in the middle between its two tensors), one mtmp_reduce_scatter into the nine slices.  n + n_time =
    2056 puts the time rows on either side of the first in-flight row set (2048 rows)."""
    from medical_tri_modal_pilot_amd.optim import FlatParams
    c = R.tie_case(n, dt, True, n_time)
    prm = [torch.nn.Parameter(dev(p)) for p in c["prm"]]
    fp = FlatParams([(f"p{i}", p) for i, p in enumerate(prm)])
    fp.zero_grad()
    out, it, tt = ops.TieTimeEmbed.apply(dev(c["ev"]).view(1, n, 3), dev(c["tev"]), n_img, *prm, dt)
    assert it.shape[0] == n_img and tt.shape[0] == n_time - n_img
    w_t = dev(c["w_t"])
    ((out.float() * dev(c["w"]).view(1, n, 256)).sum() + (it.float() * w_t[:n_img]).sum() + (tt.float() * w_t[n_img:]).sum()).backward()
    assert fp.written == set(range(9)), "the gradients did not take the one-slab path"
    ck = Checks(f"tie_time[{n}+{n_time},img={n_img},{dn(dt)}]")
    ck.close("out", out[0], c["ref"]["out"], c["e_torch"]["out"], dt == BF16)
    ck.close("emb", torch.cat([it, tt]), c["ref"]["emb"], c["e_torch"]["emb"], dt == BF16)
    _tie_grad_checks(ck, c, [p.grad for p in prm])
    ck.done()


# ------------------------------------------------------------------------------------------ slab reductions
def _colsum(slab, c0, ncols):
    ref, et = R.e_torch_of(R.column_sum_model, slab[:, c0:c0 + ncols])
    return ref["sum"], et["sum"]


TAIL = 5


def _dst(ncols):
    """a destination longer than its range: the tail must come back bit for bit"""
    return torch.arange(ncols + TAIL, dtype=F32, device=DEV) * 0.5 - 3.0


def _tail_kept(d, ncols):
    return torch.equal(d[ncols:], _dst(ncols)[ncols:])


@pytest.mark.parametrize("rows", R.REDUCE_ROWS)
def test_reduce_batch_and_scatter_vs_column_sum(ops, rows):
    """the three row-lane layouts of reduce_batch_kernel (rows < 64, < 256, >= 256) on the 16-byte path, a split inside a quad, the
    scalar path (770 columns; a base that is not 16-byte aligned) and a column range of a wider slab"""
    ck = Checks(f"reduce[rows={rows}]")
    s512, s770, s1792 = (R.reduce_case(rows, ld)["slab"] for ld in (512, 770, 1792))
    d512, d770, d1792 = dev(s512), dev(s770), dev(s1792)
    # reduce_batch: (slab, rows, cols, out_a, split, out_b)
    for tag, slab, dslab, cols, split in (("512/256", s512, d512, 512, 256), ("512/258", s512, d512, 512, 258), ("770/500", s770, d770, 770, 500)):
        a, b = _dst(split), _dst(cols - split)
        ops.reduce_batch([(dslab, rows, cols, a, split, b)])
        ref, et = _colsum(slab, 0, cols)
        ck.close(tag, torch.cat([a[:split], b[:cols - split]]), ref, et)
        assert _tail_kept(a, split) and _tail_kept(b, cols - split), tag
    a = _dst(770)
    ops.reduce_batch([(d770, rows, 770, a, 770, None)])
    ref, et = _colsum(s770, 0, 770)
    ck.close("770/all", a[:770], ref, et)
    assert _tail_kept(a, 770)
    # reduce_scatter: (slab, rows, col0, ncols, dst)
    for col0 in (256, 257):
        d = _dst(768)
        ops.reduce_scatter([(d1792, rows, col0, 768, d)])
        ref, et = _colsum(s1792, col0, 768)
        ck.close(f"scatter@{col0}", d[:768], ref, et)
        assert _tail_kept(d, 768), col0
    ck.done()


def test_reduce_wide_entry_past_the_block_cap(ops):
    """786 432 + 768 columns at 256 rows: 16 columns per block, so the 4096-block cap makes every block walk 12-13 column trips"""
    cols = R.REDUCE_WIDE_COLS
    c = R.reduce_case(256, cols)
    d = dev(c["slab"])
    a, b = _dst(786432), _dst(768)
    ops.reduce_batch([(d, 256, cols, a, 786432, b)])
    ck = Checks("reduce[256 x wide]")
    ck.close("batch", torch.cat([a[:786432], b[:768]]), c["ref"], c["e_torch"])
    assert _tail_kept(a, 786432) and _tail_kept(b, 768)
    o = _dst(cols)
    ops.reduce_scatter([(d, 256, 0, cols, o)])
    ck.close("scatter", o[:cols], c["ref"], c["e_torch"])
    assert _tail_kept(o, cols)
    ck.done()


def test_reduce_thirteen_entries_split_the_launch(ops):
    """more entries than one launch takes (8 for reduce_batch, 12 for reduce_scatter): the wrappers cut the list, every entry is summed"""
    ck = Checks("reduce[13 entries]")
    slabs = [R.reduce_case(r, 1792, seed=k) for k, r in enumerate((63, 3, 257, 64, 1, 255, 256, 63, 3, 257, 64, 2053, 255))]
    ds = [dev(c["slab"]) for c in slabs]
    dsts = [_dst(64 * (k + 1)) for k in range(13)]
    ops.reduce_scatter([(ds[k], slabs[k]["slab"].shape[0], 4 * k, 64 * (k + 1), dsts[k]) for k in range(13)])
    for k in range(13):
        ref, et = _colsum(slabs[k]["slab"], 4 * k, 64 * (k + 1))
        ck.close(f"scatter{k}", dsts[k][:64 * (k + 1)], ref, et)
        assert _tail_kept(dsts[k], 64 * (k + 1))
    outs = [(_dst(1000 + k), _dst(792 - k)) for k in range(13)]
    pending = [(ds[k], slabs[k]["slab"].shape[0], 1792, outs[k][0], 1000 + k, outs[k][1]) for k in range(13)]
    ops.reduce_batch(pending)
    assert pending == []
    for k in range(13):
        ck.close(f"batch{k}", torch.cat([outs[k][0][:1000 + k], outs[k][1][:792 - k]]), slabs[k]["ref"], slabs[k]["e_torch"])
        assert _tail_kept(outs[k][0], 1000 + k) and _tail_kept(outs[k][1], 792 - k)
    ck.done()


# ------------------------------------------------------------------------------------------ token-group sums
def _token_sums(ops, dxs, Ls):
    """mtmp_token_sums has no wrapper of its own (ops.StreamInputsFn calls it): out[j] = sum of the L rows of group j, <= 2 tensors"""
    k = len(dxs)
    outs = [torch.full((d.shape[0] // L, 256), float("nan"), dtype=d.dtype, device=DEV) for d, L in zip(dxs, Ls)]
    ops.call("mtmp_token_sums", ops._dt(dxs[0]), k, (ctypes.c_void_p * k)(*[d.data_ptr() for d in dxs]),
             (ctypes.c_void_p * k)(*[o.data_ptr() for o in outs]), (ctypes.c_int * k)(*[o.shape[0] for o in outs]),
             (ctypes.c_int * k)(*Ls), ops._stream())
    return outs


@pytest.mark.parametrize("dt", DT, ids=dn)
@pytest.mark.parametrize("L", R.TOKEN_L)
def test_token_sums(ops, dt, L):
    """two rows in flight per wave, four waves: L = 1, 4 | 5, 8 | 9 are the edges of the loop and its tail, 49 and 128 the product's sizes"""
    c = R.token_case(L, 3, dt)
    L2 = 4 if L == 9 else 9
    c2 = R.token_case(L2, 2, dt)
    dx, dx2 = dev(c["dx"], dt), dev(c2["dx"], dt)
    one, = _token_sums(ops, [dx], [L])
    two_a, two_b = _token_sums(ops, [dx, dx2], [L, L2])
    rev_b, rev_a = _token_sums(ops, [dx2, dx], [L2, L])
    alone_b, = _token_sums(ops, [dx2], [L2])
    assert torch.equal(one, two_a) and torch.equal(one, rev_a) and torch.equal(alone_b, two_b) and torch.equal(alone_b, rev_b)
    ck = Checks(f"token_sums[L={L},{dn(dt)}]")
    ck.close("sum", one, c["ref"], c["e_torch"], dt == BF16)
    ck.close("second", two_b, c2["ref"], c2["e_torch"], dt == BF16)
    ck.done()


# ------------------------------------------------------------------------------------------ bottleneck exchange
EXCHANGE_KV0 = (7, 4, 5, 6, 7)            # lengths of a packed first stream (n_v = 7)


def _pack0(ops, t):
    """stream 0 [B,7,256] in the packed layout: (buffer of the same allocation, flat row of every sample's first row, row_starts)"""
    B = t.shape[0]
    kv = torch.tensor(EXCHANGE_KV0, dtype=torch.int32)
    pack = ops.row_starts(kv.to(DEV), 7)
    starts = torch.cat([torch.zeros(1, dtype=torch.int64), kv.long().cumsum(0)])[:B]
    assert pack[:B].cpu().tolist() == starts.tolist()
    buf = t.flip(0).contiguous().clone()                                    # (rows behind the packed ones hold other values)
    flat = buf.view(-1, 256)
    for b in range(B):
        flat[starts[b]:starts[b] + EXCHANGE_KV0[b]] = t[b, :EXCHANGE_KV0[b]]
    return buf, starts.to(DEV), pack


def _rows03(t, starts=None):
    """rows 0..3 of every sample [B,4,256], and a mask of those rows over the flat buffer"""
    B = t.shape[0]
    flat = t.view(-1, 256)
    first = torch.arange(B, device=DEV) * t.shape[1] if starts is None else starts
    idx = (first[:, None] + torch.arange(4, device=DEV)[None, :]).reshape(-1)
    mask = torch.zeros(flat.shape[0], dtype=torch.bool, device=DEV)
    mask[idx] = True
    return flat[idx].view(B, 4, 256), mask


@pytest.mark.parametrize("dt", DT, ids=dn)
@pytest.mark.parametrize("n_rows,resbottle,prev_in,two,packed", [
    ((7, 5, 13), 0, 0, 0, 0), ((7, 5, 13), 1, 0, 0, 0), ((7, 5, 13), 1, 1, 0, 0), ((7, 5, 13), 0, 0, 1, 0), ((7, 5, 13), 1, 1, 0, 1),
    ((7, 5, 13), 0, 0, 1, 1), ((4, 4, 4), 0, 0, 0, 0), ((4, 4, 4), 1, 0, 0, 0), ((4, 4, 4), 1, 1, 0, 0), ((4, 4, 4), 0, 0, 1, 0)])
def test_bottleneck_exchange(ops, dt, n_rows, resbottle, prev_in, two, packed):
    """mbt_encoder.py:764-779, both directions, in place: three streams (patterns 0..3) and two (z[2] = None, patterns {1, 3}), with and
    without the residual (prev / keep, d_prev_in), buffers with and without token rows, first stream padded and packed"""
    c = R.exchange_case(n_rows, resbottle, prev_in, two, dt)
    ref, et = c["ref"], c["e_torch"]
    missing = dev(c["missing"])
    ck = Checks(f"exchange[{n_rows},res={resbottle},prev_in={prev_in},two={two},packed={packed},{dn(dt)}]")
    for direction in ("fwd", "bwd"):
        src = c["z"] if direction == "fwd" else c["dz"]
        bufs = [dev(t, dt).contiguous() for t in src]
        starts = pack = None
        if packed:
            bufs[0], starts, pack = _pack0(ops, bufs[0])
        before = [b.clone() for b in bufs]
        zs = bufs + [None] * (3 - len(bufs))
        if direction == "fwd":
            keep = torch.full((len(c["missing"]), 4, 256), float("nan"), device=DEV) if resbottle else None
            ops.bottleneck_exchange_fwd(zs, missing, bool(resbottle), dev(c["prev"]), keep, pack)
        else:
            d_prev_out = torch.full((len(c["missing"]), 4, 256), float("nan"), device=DEV) if resbottle else None
            ops.bottleneck_exchange_bwd(zs, missing, bool(resbottle), dev(c["d_prev_in"]), d_prev_out, pack)
        got = []
        for m, (b, b0) in enumerate(zip(bufs, before)):
            rows, mask = _rows03(b, starts if m == 0 else None)
            got.append(rows)
            assert torch.equal(b.view(-1, 256)[~mask], b0.view(-1, 256)[~mask]), f"{direction}: a row >= 4 of stream {m} changed"
        if direction == "fwd":
            for m, rows in enumerate(got):
                ck.close(f"new{m}", rows, ref["new"], et["new"], dt == BF16)
                assert torch.equal(rows, got[0])                          # the buffers' rows 0..3 are bit-equal to each other
            if keep is not None:
                assert keep.dtype == F32
                ck.close("keep", keep, ref["new"], et["new"])
                assert torch.equal(got[0], keep.to(dt))                   # the rows are keep's rounding
        else:
            for m, rows in enumerate(got):
                ck.close(f"d{m}", rows, ref[f"d{m}"], et[f"d{m}"], dt == BF16)
            if d_prev_out is not None:
                ck.close("d_prev", d_prev_out, ref["d_prev"], et["d_prev"])
    ck.done()


# ------------------------------------------------------------------------------------------ AdamW
@pytest.mark.parametrize("n", R.ADAMW_N)
def test_adamw_step(ops, n):
    """1024 elements per block, 2048 blocks: n = 2 097 152 + 1028 is a second trip with a ragged end.  exp_avg / exp_avg_sq to the fp32
    bound; param to |p - p_ref| <= 2 * 2^-24 |p_ref| + bound |p_ref - p_old| (the update to the bound, the sum to its own rounding);
    the bf16 shadow bit-equal to the new parameters' rounding."""
    ck = Checks(f"adamw[{n}]")
    for step, wd, gs, shadow in R.ADAMW_RUNS:
        c = R.adamw_case(n, step, wd, gs)
        lr, b1, b2, eps, wd32, _, gs32 = c["args"]
        p, g, m, v = (dev(c[k]).clone() for k in ("p", "g", "m", "v"))
        sh = torch.full((n,), 7.0, dtype=BF16, device=DEV) if shadow else None
        g0 = g.clone()
        ops.adamw_step(p, g, m, v, sh, lr, b1, b2, eps, wd32, step, gs32)
        tag = f"step={step},wd={wd},gs={gs}"
        ref, et = c["ref"], c["e_torch"]
        ck.close(f"{tag}.exp_avg", m, ref["exp_avg"], et["exp_avg"])
        ck.close(f"{tag}.exp_avg_sq", v, ref["exp_avg_sq"], et["exp_avg_sq"])
        b = R.bound(et["update"])
        allowed = 2 * 2.0 ** -24 * ref["param"].abs() + b * (ref["param"] - c["p"].double()).abs()
        ratio = float(((p.cpu().double() - ref["param"]).abs() / allowed).max())
        ck.record(f"{tag}.param", ratio * b, et["update"], b)
        assert torch.equal(g, g0)
        if shadow:
            assert torch.equal(sh, p.to(BF16))
    ck.done()
