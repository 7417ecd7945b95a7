"""-m gpu: dropout ON.  The three mask sites of the training step and their backwards against float64 references that replay the
kernels' masks on the host (tests/dropout_model.py: a stateless counter hash), element by element, no element left out:

  a  the mask itself and dropout_bwd_kernel, bit for bit (one fp32 product, one rounding: dropout_bwd_model is exact)
  b  stream input: the `if (thr)` branches of stream_in_fwd_kernel / stream_in_bwd_body, single (ops.StreamInputFn), packed, and three
     streams with the time embeddings added in the kernels and ONE grouped backward launch (ops.StreamInputsFn)
  c  FFN1: the DROP instantiations of ln_gemm_dma_kernel (bf16, sign bits "positive and kept") and ln_gemm_kernel (fp32)
  d  FFN2: gemm_nt_kernel<DROP> at both tile heights, under a live-row word, and into a column window of a wider buffer
  e  the operand drop of the gated dH launch (mtmp_gemm_nt_signs_drop)
  f  the grouped FFN chain, where three launches must agree on two masks, down to the weight gradients
  g  a captured forward replayed under three seed words

Through the wrappers of ops.py, as test_gemm_model_gpu.py (whose helpers are used here) and test_row_kernels_gpu.py do with dropout off.
Metric and bound are theirs: err = max |got - ref| / (|ref| + rms(ref)) against max(8 e_chain, 16 * 2^-24) (+ 2^-8 for a bf16 output),
e_chain the error of the same masked chain in working precision; a dropped element must be exactly zero.  The mask, keep_scale and the
places of the mask in the chains are read from the code (gemm_model.py D1, D2; row_kernels_model.stream_input_model); nothing is fitted
to what the kernels return.  p = 0.1 unless a test says otherwise.
Every check appends to a report: build/dropout_model_report.json, or the file MTMP_DROPOUT_MODEL_REPORT names -- per group the number of
checks and the worst err / bound, and the wall time of this file.
"""
import ctypes
import json
import math
import os
import time

import pytest
import torch

from tests import dropout_model as DM
from tests import gemm_model as G
from tests import row_kernels_model as R
from tests.test_gemm_model_gpu import (GROUPS, SENTINEL, _lives, _packs, dead_rows_untouched, fl, poison, put, sentinel_outputs,
                                       signs_are_the_outputs_sign)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
P, WORD = DM.P, DM.WORD
REPORT = {}
GROUP_STATS = {}
KEPT_ALIVE = []                          # captured graphs and what they point to are never released (graph.py: a later replay crashes)


@pytest.fixture(scope="module")
def ops():
    from medical_tri_modal_pilot_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def lib():
    from medical_tri_modal_pilot_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module", autouse=True)
def _dump_report():
    t0 = time.time()
    yield
    path = os.environ.get("MTMP_DROPOUT_MODEL_REPORT") or os.path.join(ROOT, "build", "dropout_model_report.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    REPORT["_groups"] = GROUP_STATS
    REPORT["_wall_seconds"] = time.time() - t0
    with open(path, "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)
    print(f"tests/test_dropout_model_gpu.py: {REPORT['_wall_seconds']:.1f} s")
    for g, s in sorted(GROUP_STATS.items()):
        print(f"group {g}: {s['checks']} checks, worst err / bound {s['worst_ratio']:.3f}, {s['exact']} exact comparisons")


@pytest.fixture(autouse=True)
def _no_seed_word_left_over(ops):
    """a trainer of an earlier test file may have left its step word in place (graph.GraphedTrainStep sets it and nobody clears it): the
    tests here start without one, and hand back what they found"""
    found = ops._seed_word
    ops.set_seed_word(None)
    yield
    ops.set_seed_word(found)


def _count(group, ratio=None):
    s = GROUP_STATS.setdefault(group, {"checks": 0, "worst_ratio": 0.0, "exact": 0})
    if ratio is None:
        s["exact"] += 1
    else:
        s["checks"] += 1
        s["worst_ratio"] = max(s["worst_ratio"], ratio if math.isfinite(ratio) else 1e30)


class Checks:
    """the checks of one test, as in test_gemm_model_gpu.py: every figure is printed and recorded before the test asserts"""

    def __init__(self, group, tag):
        self.group, self.tag, self.failed = group, f"{group}.{tag}", []

    def close(self, name, got, ref, e_chain, bf16_out=False):
        assert bool(torch.isfinite(got).all()), f"{self.tag}.{name}: not finite"
        e, b = G.err(got, ref), G.bound(e_chain, bf16_out)
        key = f"{self.tag}.{name}"
        assert key not in REPORT, key
        REPORT[key] = {"err": e, "e_chain": e_chain, "bound": b, "ratio": e / b}
        _count(self.group, e / b)
        print(f"{key}: err {e:.3e} e_chain {e_chain:.3e} bound {b:.3e} ratio {e / b:.3f}")
        if not (math.isfinite(e) and e <= b):
            self.failed.append(f"{key}: err {e:.3e} > bound {b:.3e} (e_chain {e_chain:.3e})")

    def all(self, prefix, got, ref, e, bf16_names=()):
        for name in ref:
            self.close(prefix + name, got[name], ref[name], e[name], name in bf16_names)

    def exact(self, name, ok, what):
        """a comparison that allows nothing: bit equality, a dropped element that is not zero"""
        _count(self.group)
        if not ok:
            self.failed.append(f"{self.tag}.{name}: {what}")

    def dropped_are_zero(self, name, got, mask):
        bad = int((got[~mask.to(got.device)] != 0).sum())
        self.exact(name, bad == 0, f"{bad} dropped elements are not exactly zero")

    def done(self):
        assert not self.failed, "\n".join(self.failed)


def dn(dt):
    return G.dt_name(dt)


def on_dev(keep):
    return DM.Keep(keep.mask.to(DEV), keep.scale)


def rows_of(keep, L):
    return DM.Keep(keep.mask[:L], keep.scale)


class seed_word:
    """ops.set_seed_word for the time of a block: a device int64 word whose bits above bit 31 must not count"""

    def __init__(self, ops, value):
        self.ops, self.value = ops, value

    def __enter__(self):
        self.t = None if self.value is None else torch.full((1,), self.value, dtype=torch.int64, device=DEV)
        self.ops.set_seed_word(self.t)
        return self

    def __exit__(self, *exc):
        self.ops.set_seed_word(None)


# ------------------------------------------------------------------------------------------ a. the mask and dropout_bwd, bit for bit
DROP_N = (4, 1020, 1024, 1028, 4096 * 256 * 4 + 4)      # the last: the first group of the grid-stride loop's second trip
DROP_P = (0.1, 0.5, 2.0 ** -16, 0.999)
DROP_SEEDS = (0, 1234, 0xFFFFFFFF)


@pytest.mark.parametrize("dt", G.DTS, ids=dn)
@pytest.mark.parametrize("n", DROP_N)
def test_dropout_bwd_is_the_replayed_mask_bit_for_bit(ops, n, dt):
    """ones and a random tensor, every p, seed and with / without a seed word: out == T(float32(g) * keep_scale) where the host's mask
    keeps, +0 elsewhere, nothing allowed"""
    gen = torch.Generator().manual_seed(n)
    gs = {"ones": torch.ones(n, device=DEV, dtype=dt), "randn": torch.randn(n, generator=gen).to(DEV, dt)}
    ck = Checks("a", f"dropout_bwd[n={n},{dn(dt)}]")
    for word in (None, WORD):
        with seed_word(ops, word):
            for p in DROP_P:
                for seed in DROP_SEEDS:
                    keep = on_dev(DM.keep((n,), p, seed, word))
                    for name, g in gs.items():
                        got = ops.dropout_bwd(g, seed, p)
                        want = G.dropout_bwd_model(g.float(), keep, dt=dt)["y"]
                        diff = int((got.float() != want).sum())
                        ck.exact(f"{name}[p={p:.3g},seed={seed},word={word is not None}]", got.dtype == dt and diff == 0,
                                 f"{diff} of {n} elements differ from the model")
    ck.done()


# ------------------------------------------------------------------------------------------ b. stream input
def stream_keep(B, N, p, seed, word=None):
    return DM.Keep(DM.keep_of_elements(DM.stream_input_elements(B, N), p, seed, word), DM.keep_scale(p))


def stream_launch(ops, c, dt, p, seed, kv=None):
    """-> z (live rows), grads, the LayerNorm statistics the node saved, the live mask"""
    B, N, _ = c["x"].shape
    nb = 0 if c["bott"] is None else c["bott"].shape[-2]
    Rr = nb + 1 + N
    xd = c["x"].to(DEV, dt).requires_grad_()
    cd, gd, bd = (c[k].to(DEV).requires_grad_() for k in ("cls", "gamma", "beta"))
    td = None if c["bott"] is None else c["bott"].to(DEV).requires_grad_()
    pe = None if c["pe"] is None else c["pe"].to(DEV)
    live = torch.ones(B, Rr, dtype=torch.bool) if kv is None else torch.arange(Rr)[None, :] < torch.tensor(kv)[:, None]
    if kv is not None:
        kvd = torch.tensor(kv, dtype=torch.int32, device=DEV)
        pack = ops.row_starts(kvd, Rr)
        z = ops.StreamInputFn.apply(xd, cd, gd, bd, pe, td, 1e-5, p, seed, pack, kvd)
        starts = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(kv).cumsum(0)])
        rows = torch.cat([starts[b] + torch.arange(kv[b]) for b in range(B)]).to(DEV)
        z_live = z.view(-1, 256)[rows]
    else:
        z = ops.StreamInputFn.apply(xd, cd, gd, bd, pe, td, 1e-5, p, seed)
        z_live = z[live.to(DEV)]
    stats = z.grad_fn.saved_tensors[3].clone()
    (z_live.float() * c["w"][live].to(DEV)).sum().backward()
    grads = dict(dx=xd.grad, dcls=cd.grad.view(-1), dgamma=gd.grad, dbeta=bd.grad)
    if td is not None:
        grads["dbott"] = td.grad.view(nb, 256)
    return z_live.detach(), grads, stats, live


def stream_checks(ck, prefix, dt, z_live, grads, ref, et, keep, nb):
    live = ref["live"]
    ck.close(prefix + "z", z_live, ref["z"][live], et["z"], dt == BF16)
    ck.dropped_are_zero(prefix + "z", z_live, torch.cat([torch.ones(live.shape[0], nb, 256, dtype=torch.bool), keep.mask], 1)[live])
    ck.close(prefix + "dx", grads["dx"], ref["dx"], et["dx"], dt == BF16)
    for k in ("dcls", "dgamma", "dbeta", "dbott"):
        if k in ref and k in grads:
            assert grads[k].dtype == F32
            ck.close(prefix + k, grads[k], ref[k], et[k])


@pytest.mark.parametrize("dt", G.DTS, ids=dn)
@pytest.mark.parametrize("B,N,nb,use_pe,kv", [c + (None,) for c in DM.STREAM_DROP_CASES] + [R.STREAM_PACKED[:3] + (False, R.STREAM_PACKED[3])])
def test_stream_input_with_dropout(ops, B, N, nb, use_pe, kv, dt):
    """z, dx and the gradients of CLS, gamma, beta and the bottleneck rows; the LayerNorm statistics are those of the p = 0 launch on
    the same input, bit for bit; packed: rows that do not exist change no numbering"""
    c = R.stream_case(B, N, nb, use_pe, dt, kv)
    keep = stream_keep(B, N, P, DM.STREAM_SEED)
    ref, et = R.e_torch_of(R.stream_input_model, c["x"], c["cls"], c["gamma"], c["beta"], c["pe"], c["bott"], c["w"], c["kv_len"], keep, dt=dt)
    z_live, grads, stats, live = stream_launch(ops, c, dt, P, DM.STREAM_SEED, kv)
    _, _, stats0, _ = stream_launch(ops, c, dt, 0.0, DM.STREAM_SEED, kv)
    ck = Checks("b", f"stream_in[{B}x{N}+{nb},{'packed' if kv else 'dense'},{dn(dt)}]")
    assert torch.equal(live, ref["live"])
    ln_live = live[:, nb:].reshape(-1).to(DEV)
    ck.exact("stats", torch.equal(stats[ln_live], stats0[ln_live]), "the LayerNorm statistics differ from the p = 0 launch")
    stream_checks(ck, "", dt, z_live, grads, ref, et, keep, nb)
    ck.done()


@pytest.mark.parametrize("dt", G.DTS, ids=dn)
def test_three_stream_inputs_three_seeds_one_backward_launch(ops, dt):
    """ops.StreamInputsFn: mtmp_stream_input_fwd_add per stream (the time embeddings added inside the kernel, the sum rounded to the
    compute type), stream 0 packed, and ONE mtmp_stream_input_bwd_grouped -- every stream against the model with ITS seed's mask"""
    S = DM.STREAMS3
    B, nb, K, Ns, kv, seeds = (S[k] for k in ("B", "nb", "K", "Ns", "kv", "seeds"))
    g = torch.Generator().manual_seed(11)
    rn = lambda *sh: torch.randn(*sh, generator=g)
    xs = [R.rnd(rn(B, n, 256) * 1.5 + 0.2, dt) for n in Ns]
    add_i, add_t = R.rnd(rn(B * K, 256), dt), R.rnd(rn(B, 256), dt)
    cls, gam, bet = [rn(1, 1, 256) for _ in Ns], [1 + 0.1 * rn(256) for _ in Ns], [0.1 * rn(256) for _ in Ns]
    bott = rn(1, nb, 256)
    pes = [None, R.sinusoid_table(Ns[1] + 1), None]
    ws = [R.rnd(rn(B, nb + 1 + n, 256), dt) for n in Ns]
    kvs = [torch.tensor(kv, dtype=torch.int32), None, None]
    # the rows the LayerNorm sees: x + its group's embedding, rounded to the compute type
    xin = [xs[0], R.rnd((xs[1].view(B * K, Ns[1] // K, 256) + add_i[:, None]).view(B, Ns[1], 256), dt), R.rnd(xs[2] + add_t[:, None], dt)]
    keeps = [stream_keep(B, n, P, s) for n, s in zip(Ns, seeds)]
    n0 = B * (min(Ns) + 1) * 256
    masks0 = [DM.keep_mask((n0,), P, s) for s in seeds]
    assert not any(torch.equal(masks0[i], masks0[j]) for i, j in ((0, 1), (0, 2), (1, 2)))
    refs = [R.e_torch_of(R.stream_input_model, xin[m], cls[m], gam[m], bet[m], pes[m], bott, ws[m], kvs[m], keeps[m], dt=dt) for m in range(3)]
    xd = [x.to(DEV, dt).requires_grad_() for x in xs]
    prm = [t.to(DEV).requires_grad_() for m in range(3) for t in (cls[m], gam[m], bet[m])]
    bd = bott.to(DEV).requires_grad_()
    kvd = kvs[0].to(DEV)
    pack = ops.row_starts(kvd, nb + 1 + Ns[0])
    meta = dict(pe=[None if q is None else q.to(DEV) for q in pes], seeds=list(seeds), pack=(pack, kvd), streams=None)
    zs = ops.StreamInputsFn.apply(xd[0], xd[1], xd[2], bd, add_i.to(DEV, dt), add_t.to(DEV, dt), 1e-5, 1e-5, 1e-5, P, meta, *prm)
    starts = torch.cat([torch.zeros(1, dtype=torch.int64), kvs[0].long().cumsum(0)])
    rows0 = torch.cat([starts[b] + torch.arange(kv[b]) for b in range(B)]).to(DEV)
    z_live = [zs[0].view(-1, 256)[rows0]] + [zs[m][refs[m][0]["live"].to(DEV)] for m in (1, 2)]
    sum((z.float() * ws[m][refs[m][0]["live"]].to(DEV)).sum() for m, z in enumerate(z_live)).backward()
    ck = Checks("b", f"stream_inputs_node[{dn(dt)}]")
    for m in range(3):
        grads = dict(dx=xd[m].grad, dcls=prm[3 * m].grad.view(-1), dgamma=prm[3 * m + 1].grad, dbeta=prm[3 * m + 2].grad)
        stream_checks(ck, f"s{m}.", dt, z_live[m].detach(), grads, refs[m][0], refs[m][1], keeps[m], nb)
    # the bottleneck rows feed all three streams: one gradient, the sum of the three
    chain = lambda ft: sum(R.stream_input_model(xin[m], cls[m], gam[m], bet[m], pes[m], bott, ws[m], kvs[m], keeps[m], dt=dt, ft=ft)["dbott"] for m in range(3))
    ref_b = chain(F64)
    ck.close("dbott", bd.grad.view(nb, 256), ref_b, G.err(chain(F32), ref_b))
    ck.done()


# ------------------------------------------------------------------------------------------ c. FFN1
def run_ffn1(ops, ck, prefix, M, dt, seed, p=P, word=None, relu=True, ld_seed=0):
    """ops.ln_gemm with dropout (sign bits with the ReLU) -> the outputs and the mask (device)"""
    N = 1024
    q = G.ln_gemm_inputs(M, N, dt, seed=ld_seed)
    x, w = put(q["x"], dt), put(q["w"], dt)
    gam, bet, b = put(q["gamma"]), put(q["beta"]), put(q["bias"])
    keep = on_dev(DM.keep((M, N), p, seed, word))
    with sentinel_outputs():
        y, xn, st, *sg = ops.ln_gemm(x, gam, bet, w, b, N, relu=relu, drop_p=p, seed=seed, want_signs=relu)
        y0, xn0, st0, *_ = ops.ln_gemm(x, gam, bet, w, b, N, relu=relu, want_signs=relu)
    ref, e = G.e_chain_of(G.ln_gemm_model, fl(x), gam, bet, fl(w), b, "relu" if relu else None, keep, dt=dt)
    ck.all(prefix, dict(y=y, xn=xn, mean=st[:, 0], rstd=st[:, 1]), ref, e, bf16_names=("y", "xn") if dt == BF16 else ())
    ck.dropped_are_zero(prefix + "y", y, keep.mask)
    ck.exact(prefix + "xn,stats", torch.equal(xn, xn0) and torch.equal(st, st0), "xn / mean / rstd differ from the p = 0 launch")
    gate = None
    if relu and dt == BF16:
        gate = signs_are_the_outputs_sign(ck.tag, sg[0], y, M)
        ck.exact(prefix + "signs", not bool((gate & ~keep.mask).any()), "a sign bit is set where the mask drops")
    elif relu:
        assert sg[0] is None
    return dict(y=y, signs=sg[0] if relu else None, gate=gate, keep=keep)


@pytest.mark.parametrize("dt", G.DTS, ids=dn)
@pytest.mark.parametrize("M", DM.FFN1_M + (8193,))
def test_ffn1_with_dropout(ops, M, dt):
    """M on both sides of the wave's 32 and the workgroup's 128 rows, and the panel walk of (8193, 1024): three panels per workgroup"""
    ck = Checks("c", f"ffn1[M={M},{dn(dt)}]")
    run_ffn1(ops, ck, "", M, dt, DM.FFN1_SEED, ld_seed=1 if M == 8193 else 0)
    ck.done()


@pytest.mark.parametrize("dt", G.DTS, ids=dn)
def test_ffn1_without_relu(ops, dt):
    """ln_gemm_kernel<T, false, true> (fp32) / ln_gemm_dma_kernel<false, true, false, false>: negative values under the mask"""
    ck = Checks("c", f"ffn1.norelu[M=129,{dn(dt)}]")
    run_ffn1(ops, ck, "", 129, dt, DM.FFN1_SEED + 2, relu=False)
    ck.done()


@pytest.mark.parametrize("dt", G.DTS, ids=dn)
@pytest.mark.parametrize("M", DM.FFN1_M)
def test_ffn1_field_equal_to_the_threshold_is_kept(ops, M, dt):
    """SEEDS_EQ[M]: a seed with an element whose field EQUALS the threshold where the output is well above zero (searched on the CPU,
    tests/test_dropout_model_cpu.py) -- `>` for `>=` drops it"""
    seed = DM.SEEDS_EQ[M]
    ck = Checks("c", f"ffn1.seeds_eq[M={M},{dn(dt)}]")
    out = run_ffn1(ops, ck, "", M, dt, seed)
    eq = DM.equal_fields((M, 1024), P, seed).to(DEV)
    ck.exact("kept", bool((out["y"][eq] > 0).any()), "no element with field == thr came out positive")
    ck.done()


@pytest.mark.parametrize("dt", G.DTS, ids=dn)
def test_ffn1_under_a_seed_word(ops, dt):
    ck = Checks("c", f"ffn1.word[M=129,{dn(dt)}]")
    with seed_word(ops, WORD):
        run_ffn1(ops, ck, "", 129, dt, DM.FFN1_SEED, word=WORD)
    ck.done()


# ------------------------------------------------------------------------------------------ d. FFN2
def run_ffn2(ops, ck, prefix, M, N, K, dt, o, seed=DM.FFN2_SEED, p=P, live=None, ldy=None, word=None):
    q = G.nt_inputs(M, N, K, dt, bias=o.get("bias", True), res=o.get("res", False), row_scale=o.get("row_scale", 0), lda=o.get("lda"),
                    ldr=o.get("ldr"))
    a, w, res = (put(q[k], dt) for k in ("a", "w", "res"))
    b, rsc = put(q["bias"]), put(q["row_scale"])
    rps, act = o.get("row_scale", 0) or 1, o.get("act")
    L = M if live is None else live
    keep = on_dev(DM.keep((M, N), p, seed, word))
    ref, e = G.e_chain_of(G.gemm_nt_model, fl(a)[:L], fl(w), b, None if res is None else fl(res)[:L], act, None, 1.0, rsc, rps,
                          rows_of(keep, L), dt=dt)
    if live is not None:
        poison(a, live), poison(res, live)
    table = None if live is None else torch.tensor([M, live, 0, 0], dtype=torch.int32, device=DEV)
    if ldy is None:
        with sentinel_outputs(), ops.rows_live(table, 1):
            y = ops.gemm_nt(a, w, b, res, act, drop_p=p, seed=seed, row_scale=rsc, rows_per_scale=rps)
    else:                                  # the entry point itself: y is columns [0, N) of an [M, ldy] buffer (no wrapper passes ldy != N)
        buf = torch.full((M, ldy), SENTINEL, dtype=dt, device=DEV)
        ops.call("mtmp_gemm_nt_live", ops._dt(a), ops._p(a), ops._p(w), ops._p(b), ops._p(res), ops._p(buf), M, N, K, a.stride(0), ldy,
                 0 if res is None else res.stride(0), ops.ACT[act], float(p), seed & 0xFFFFFFFF, ops._p(ops._seed_word), None, 1.0,
                 ops._p(rsc), rps, None, ops._stream())
        assert bool((buf[:, N:] == SENTINEL).all()), "columns behind the window were written"
        y = buf[:, :N]
    if live is not None:
        dead_rows_untouched(ck.tag, y, live)
    ck.close(prefix + "y", y[:L], ref["y"], e["y"], dt == BF16)
    if res is None and rsc is None:
        ck.dropped_are_zero(prefix + "y", y[:L], keep.mask[:L])
    else:                                  # behind the residual a dropped element IS the residual: T(0 + res), exact
        want = fl(res)[:L] if rsc is None else None
        if want is not None:
            bad = int((y[:L].float()[~keep.mask[:L]] != want[~keep.mask[:L]]).sum())
            ck.exact(prefix + "y.dropped", bad == 0, f"{bad} dropped elements are not exactly the residual")
    return y


def _nt_id(c):
    return f"{c[0]}x{c[1]}x{c[2]}-" + "+".join(f"{k}={v}" if not isinstance(v, bool) else k for k, v in sorted(c[3].items()))


@pytest.mark.parametrize("dt", G.DTS, ids=dn)
@pytest.mark.parametrize("c", DM.NT_DROP_CASES, ids=_nt_id)
def test_ffn2_with_dropout(ops, c, dt):
    M, N, K, o = c
    ck = Checks("d", f"ffn2[{_nt_id(c)},{dn(dt)}]")
    run_ffn2(ops, ck, "", M, N, K, dt, o)
    ck.done()


@pytest.mark.parametrize("dt", G.DTS, ids=dn)
def test_ffn2_with_dropout_under_a_live_row_word(ops, dt):
    M, N, K, o, live = DM.NT_LIVE_CASE
    ck = Checks("d", f"ffn2.live[M={M},live={live},{dn(dt)}]")
    run_ffn2(ops, ck, "", M, N, K, dt, o, live=live)
    ck.done()


@pytest.mark.parametrize("dt", G.DTS, ids=dn)
def test_ffn2_with_dropout_into_a_column_window(ops, dt):
    """ldy = 176 for N = 160: the mask is numbered by row * N + col, not by the output's row stride"""
    M, N, K, o, ldy = DM.NT_WINDOW_CASE
    ck = Checks("d", f"ffn2.window[{M}x{N}x{K},ldy={ldy},{dn(dt)}]")
    run_ffn2(ops, ck, "", M, N, K, dt, o, ldy=ldy)
    ck.done()


# ------------------------------------------------------------------------------------------ e. gated dH with the operand drop
@pytest.mark.parametrize("M", DM.FFN1_M)
def test_gated_dh_with_the_operand_drop(ops, M):
    """bf16: the forward's own sign bits (with drop1 folded in) gate dH = dropout_bwd(dY2) W2 * 1 / (1 - p); the masked operand comes
    back bit-equal to dropout_bwd_model, and the product takes that ROUNDED operand"""
    dt, N = BF16, 1024
    ck = Checks("e", f"gated_dh[M={M},bf16]")
    fwd = run_ffn1(ops, ck, "ffn1.", M, dt, DM.FFN1_SEED)
    q = G.gated_inputs(M, N, dt, seed=5)
    a, w2 = put(q["a"], dt), put(q["w"], dt)
    keep2 = on_dev(DM.keep((M, 256), P, DM.FFN2_SEED))
    gs = DM.keep_scale(P)
    with sentinel_outputs():
        dh, ad = ops.gemm_nt_signs(a, w2, fwd["signs"], gs, drop_p=P, seed=DM.FFN2_SEED)
    ref, e = G.e_chain_of(G.operand_drop_model, fl(a), keep2, fl(w2), fwd["gate"], gs, dt=dt)
    ck.exact("a_dropped", ad.dtype == dt and torch.equal(ad.float(), ref["a"].float()), "the masked operand differs from dropout_bwd_model")
    ck.close("dh", dh, ref["y"], e["y"], True)
    ck.dropped_are_zero("dh", dh, fwd["gate"])
    ck.done()


# ------------------------------------------------------------------------------------------ f. the grouped FFN chain
SEEDS1, SEEDS2 = (101, 102, 103), (201, 202, 203)


def _tn_splits(lib, Ms, Ls, packed, N, K, dt):
    if dt == BF16:
        plan = (ctypes.c_int * 3)()
        if lib.mtmp_gemm_tn_group_plan(3, (ctypes.c_int * 3)(*Ms), N, K, plan) == 0:
            return list(plan)
        return [lib.mtmp_gemm_tn_slab_rows(1, M, N, K) for M in Ms]
    return [lib.mtmp_gemm_tn_slab_rows(0, L if packed else M, N, K) for M, L in zip(Ms, Ls)]


def run_chain(ops, lib, ck, gname, dt, p, word=None):
    Ms, lives = GROUPS[gname]
    Ls, N = _lives(Ms, lives), 1024
    ps = [G.ln_gemm_inputs(M, N, dt, seed=30 + i) for i, M in enumerate(Ms)]
    qs = [G.nt_inputs(M, 256, N, dt, seed=40 + i, res=True) for i, M in enumerate(Ms)]
    gen = torch.Generator().manual_seed(50)
    xs, w1s = [put(q["x"], dt) for q in ps], [put(q["w"], dt) for q in ps]
    gms, bts, c1s = ([put(q[k]) for q in ps] for k in ("gamma", "beta", "bias"))
    w2s, r1s, c2s = [put(q["w"], dt) for q in qs], [put(q["res"], dt) for q in qs], [put(q["bias"]) for q in qs]
    w2ts = [w.t().contiguous() for w in w2s]
    douts = [torch.randn(M, 256, generator=gen).to(DEV, dt) for M in Ms]
    keep1 = [on_dev(DM.keep((M, N), p, s, word)) for M, s in zip(Ms, SEEDS1)]
    keep2 = [on_dev(DM.keep((M, 256), p, s, word)) for M, s in zip(Ms, SEEDS2)]
    assert not torch.equal(keep1[1].mask[:1], keep1[2].mask[:1]) and not torch.equal(keep2[1].mask[:1], keep2[2].mask[:1])
    x_live, r_live, d_live = ([fl(t)[:L] for t, L in zip(ts, Ls)] for ts in (xs, r1s, douts))
    for t, L in zip(xs + r1s + douts, Ls * 3):
        poison(t, L)
    packs, gs = _packs(lives, dt), DM.keep_scale(p)
    with sentinel_outputs():
        h, xn, st, sg = ops.ln_gemm_signs_grouped(xs, gms, bts, w1s, c1s, N, p, list(SEEDS1), packs)
        out = ops.gemm_nt_grouped(h, w2s, c2s, r1s, p, list(SEEDS2), packs)
        dh, dy2 = ops.gemm_nt_signs_drop_grouped(douts, w2ts, sg, gs, p, list(SEEDS2), packs, gates=h)
        d2, d1 = [[] for _ in Ms], [[] for _ in Ms]
        g2 = ops.gemm_tn_grouped(dy2, h, [None] * 3, d2, packs)
        g1 = ops.gemm_tn_grouped(dh, xn, [None] * 3, d1, packs)
        ops.reduce_batch([e for d in d2 + d1 for e in d])
    s2, s1 = _tn_splits(lib, Ms, Ls, lives is not None, 256, N, dt), _tn_splits(lib, Ms, Ls, lives is not None, N, 256, dt)
    bf = dt == BF16
    for i, (M, L) in enumerate(zip(Ms, Ls)):
        pre = f"s{i}."
        for name, t in (("h", h[i]), ("out", out[i]), ("dh", dh[i])):
            dead_rows_untouched(f"{ck.tag}.{pre}{name}", t, L)
        k1, k2 = rows_of(keep1[i], L), rows_of(keep2[i], L)
        ref, e = G.e_chain_of(G.ln_gemm_model, x_live[i], gms[i], bts[i], fl(w1s[i]), c1s[i], "relu", k1, dt=dt)
        ck.close(pre + "h", h[i][:L], ref["y"], e["y"], bf)
        ck.dropped_are_zero(pre + "h", h[i][:L], k1.mask)
        gate = signs_are_the_outputs_sign(f"{ck.tag}.{pre}", sg[i], h[i], M, L) if bf else h[i][:L] > 0
        ref, e = G.e_chain_of(G.gemm_nt_model, fl(h[i])[:L], fl(w2s[i]), c2s[i], r_live[i], keep=k2, dt=dt)
        ck.close(pre + "out", out[i][:L], ref["y"], e["y"], bf)
        ref, e = G.e_chain_of(G.operand_drop_model, d_live[i], k2, fl(w2ts[i]), gate, gs, dt=dt)
        ck.exact(pre + "dy2", torch.equal(dy2[i][:L].float(), ref["a"].float()), "the masked dY2 differs from dropout_bwd_model")
        ck.close(pre + "dh", dh[i][:L], ref["y"], e["y"], bf)
        ck.dropped_are_zero(pre + "dh", dh[i][:L], gate)
        ref, e = G.e_chain_of(G.gemm_tn_model, fl(dy2[i])[:L], fl(h[i])[:L], s2[i], dt=dt)
        ck.all(pre + "ffn2.", dict(dw=g2[i][0], db=g2[i][1]), ref, e)
        ref, e = G.e_chain_of(G.gemm_tn_model, fl(dh[i])[:L], fl(xn[i])[:L], s1[i], dt=dt)
        ck.all(pre + "ffn1.", dict(dw=g1[i][0], db=g1[i][1]), ref, e)


@pytest.mark.parametrize("dt", G.DTS, ids=dn)
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("gname", ["dense", "packedA"])
def test_grouped_ffn_chain_with_dropout(ops, lib, gname, p, dt):
    """ln_gemm_signs_grouped -> gemm_nt_grouped -> gemm_nt_signs_drop_grouped -> gemm_tn_grouped on three streams with six different
    seeds: h (drop1), out (drop2), the masked dY2 (drop2's mask again, bit for bit), dH (drop1 through the sign bits; fp32: dropout_bwd
    + the gated gemm_nt), dW2, db2, dW1, db1.  Every launch takes the launches' own outputs in front of it as its operands."""
    ck = Checks("f", f"chain.{gname}[p={p},{dn(dt)}]")
    run_chain(ops, lib, ck, gname, dt, p)
    ck.done()


@pytest.mark.parametrize("dt", G.DTS, ids=dn)
def test_grouped_ffn_chain_under_a_seed_word(ops, lib, dt):
    ck = Checks("f", f"chain.word.packedA[p={P},{dn(dt)}]")
    with seed_word(ops, WORD):
        run_chain(ops, lib, ck, "packedA", dt, P, word=WORD)
    ck.done()


# ------------------------------------------------------------------------------------------ g. graph replay
@pytest.mark.parametrize("dt", G.DTS, ids=dn)
def test_replays_draw_the_mask_of_the_word_they_find(ops, dt):
    """one FFN1 forward and one dropout_bwd of ones, captured once with the seed word in place and replayed under three words (bits
    above bit 31 set; the scalar seed is frozen in the graph): each replay's mask is the model's for THAT word, exactly"""
    M, N, seed = 129, 1024, DM.FFN1_SEED
    q = G.ln_gemm_inputs(M, N, dt)
    x, w = put(q["x"], dt), put(q["w"], dt)
    gam, bet, b = put(q["gamma"]), put(q["beta"]), put(q["bias"])
    ones = torch.ones(M, N, device=DEV, dtype=dt)
    word = torch.zeros(1, dtype=torch.int64, device=DEV)
    words = [WORD, WORD + 0x9E3779B1, (WORD ^ 0x7FFFFFFF00000000) + 1]
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    KEPT_ALIVE.append((graph, word, x, w, gam, bet, b, ones, side))
    fn = lambda: (ops.ln_gemm(x, gam, bet, w, b, N, relu=True, drop_p=P, seed=seed)[0], ops.dropout_bwd(ones, seed, P))
    ck = Checks("g", f"replay[M={M},{dn(dt)}]")
    ops.set_seed_word(word)
    try:
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()                                          # (eager once: nothing lazy inside the capture)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            y, gm = fn()
        masks = []
        for k, wv in enumerate(words):
            with torch.cuda.stream(side):
                word.fill_(wv)
                graph.replay()
            side.synchronize()
            keep = on_dev(DM.keep((M, N), P, seed, wv))
            masks.append(keep.mask)
            ck.exact(f"r{k}.mask", torch.equal(gm != 0, keep.mask), "dropout_bwd's mask is not the model's for this word")
            ref, e = G.e_chain_of(G.ln_gemm_model, fl(x), gam, bet, fl(w), b, "relu", keep, dt=dt)
            ck.close(f"r{k}.y", y, ref["y"], e["y"], dt == BF16)
            ck.dropped_are_zero(f"r{k}.y", y, keep.mask)
        assert not torch.equal(masks[0], masks[1]) and not torch.equal(masks[1], masks[2]) and not torch.equal(masks[0], masks[2])
    finally:
        ops.set_seed_word(None)
    ck.done()
