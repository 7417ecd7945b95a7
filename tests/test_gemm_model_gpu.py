"""-m gpu: the projection GEMMs of csrc/gemm.hip against the float64 models of tests/gemm_model.py, element by element, through the
wrappers of ops.py (single and `_grouped` forms), dropout off.  Metric and bound: see gemm_model.py -- every output tensor of a launch
(live rows only) meets max(8 e_chain, 16 * 2^-24) (+ 2^-8 for a bf16 output), e_chain being the error of the working-precision chain
against the float64 chain; nothing is fitted to what the kernels return.  Operands are rounded to the compute type on both sides.  The
models run on the device (float64 and fp32 torch there), the LayerNorm backward's on the CPU.  Rows behind a packed stream's live rows
are NaN on the way in and must hold the sentinel bit for bit on the way out.
Every check appends {err, e_chain, bound, ratio} to a report: build/gemm_model_report.json, or the file MTMP_GEMM_MODEL_REPORT names.

Shapes, from the launchers (gemm.hip):
  ln_gemm / ln_gemm_dma: a wave owns 32 rows, a workgroup 128 -> M on both sides of 32 and 128, 257 = a third block of one row.  N: 768
      (key norms), 1024 (ReLU + sign bits), one panel (64 bf16 / 32 fp32: Panel<T>::NP, the launcher's N % NP == 0), three panels
      (192 / 96: an odd count, so the two-buffer walk ends on buffer 0).  gridDim.y = nsplit = clamp(512 / mtiles, need, npanels),
      per = ceil(npanels / nsplit): up to M = 4096 (32 row blocks) every workgroup has one panel; 4097: per 2; 8193: per 3 with shares
      3 3 3 3 3 1 and one workgroup without a panel; 32769: one workgroup walks all 16 (= MAXP) or 12 (gemm_model.panel_shares).
  gemm_nt: 64-row tiles while ceil(M / 128) * ceil(N / 128) < 512, else 128-row tiles: (8064, 1024) is the last 64-row shape, (8193,
      1024) takes 128.  nk = ceil(K / 64) k-steps; bf16 64-row tiles keep two steps in flight and leave the loop by its `break` when nk
      is odd (K 8, 56, 64, 192) and by its condition when even (72, 96, 128, 200 -> 4, 1024 -> 16).  K % 64 != 0 masks the tail chunk.
      An N that is no multiple of 128 leaves column pieces past N inside the last block (gcolc = min(gcol, N - 8)).
  gemm_lnbwd: 128 rows per workgroup, four waves of 32 rows in trips of 4: M = 129 is a second slab with one row, 257 a third.
  gemm_tn (tn_launch_splits): N, K multiples of 128.  fp32 is always mode 0; bf16 takes two token groups (mode 1) once
      tn_splits(M, N, K, 192) * 512 <= M, and the LDS-DMA kernel (mode 3) if then K >= 256.  With 16 tiles (256 x 1024, 2048 x 128) that
      is 12 splits and M >= 6144: 6143 is mode 0 (24 splits), 6144 the smallest mode 1 / 3, 6181 ends 37 rows into a 64-token stage of
      split 10 and leaves split 11 without rows.  Mode 0 leaves a split empty only when the split count is capped by the tiles
      (fp32: 640 / 64 tiles = 10 splits at 1024 x 1024, M = 2561: 9 * 320 >= M) or, packed, when the live rows are few.
"""
import contextlib
import json
import math
import os
import time

import pytest
import torch

from tests import gemm_model as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
REPORT = {}
SENTINEL = 768.0                       # (exact in bf16) what the wrappers' float buffers hold before a launch
SENTINEL_BYTE = 0xA5                   # ... and their uint8 buffers (the sign bits)
GATE_SCALE = 1.25                      # 1 / (1 - 0.2): the factor a dropout of 0.2 folds into the gate
T0 = time.time()


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
    yield
    path = os.environ.get("MTMP_GEMM_MODEL_REPORT") or os.path.join(ROOT, "build", "gemm_model_report.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    REPORT["_wall_seconds"] = time.time() - T0
    with open(path, "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


class Checks:
    """collects the checks of one test: every figure is printed and recorded before the test asserts"""

    def __init__(self, tag):
        self.tag, self.failed = tag, []

    def close(self, name, got, ref, e_chain, bf16_out=False):
        assert bool(torch.isfinite(got).all()), f"{self.tag}.{name}: not finite"
        e, b = G.err(got, ref), G.bound(e_chain, bf16_out)
        key = f"{self.tag}.{name}"
        assert key not in REPORT, key
        REPORT[key] = {"err": e, "e_chain": e_chain, "bound": b, "ratio": e / b}
        print(f"{key}: err {e:.3e} e_chain {e_chain:.3e} bound {b:.3e} ratio {e / b:.3f}")
        if not (math.isfinite(e) and e <= b):
            self.failed.append(f"{key}: err {e:.3e} > bound {b:.3e} (e_chain {e_chain:.3e})")

    def all(self, prefix, got, ref, e, bf16_names=()):
        for name in ref:
            self.close(prefix + name, got[name], ref[name], e[name], name in bf16_names)

    def done(self):
        assert not self.failed, "\n".join(self.failed)


def dn(dt):
    return G.dt_name(dt)


@contextlib.contextmanager
def sentinel_outputs():
    """the buffers that the wrappers allocate for a launch start out as SENTINEL, so a row the kernels do not write shows"""
    empty, empty_like = torch.empty, torch.empty_like

    def fill(t):
        if t.is_floating_point():
            t.fill_(SENTINEL)
        elif t.dtype == torch.uint8:
            t.fill_(SENTINEL_BYTE)
        return t

    torch.empty = lambda *a, **k: fill(empty(*a, **k))
    torch.empty_like = lambda *a, **k: fill(empty_like(*a, **k))
    try:
        yield
    finally:
        torch.empty, torch.empty_like = empty, empty_like


def put(t, dt=F32):
    """a CPU tensor of the models' inputs -> the device in the compute type; a column window of a wider buffer stays one"""
    if t is None:
        return None
    if t.dim() == 2 and t._base is not None and not t.is_contiguous():
        off = t.storage_offset()
        return t._base.to(DEV, dt)[:, off:off + t.shape[1]]
    return t.to(DEV, dt)


def fl(t):
    """the values of a device operand as the models take them"""
    return None if t is None else t.float()


def pack_word(live):
    """a row_starts() tensor of one sample: [0, rows in use, order]"""
    return torch.tensor([0, live, 0], dtype=torch.int32, device=DEV)


def poison(t, live):
    """rows behind the live ones are NaN: reading one shows in the output"""
    if t is not None and live < t.shape[0]:
        t[live:] = float("nan")
    return t


def dead_rows_untouched(name, t, live):
    dead = t[live:]
    want = SENTINEL_BYTE if t.dtype == torch.uint8 else SENTINEL
    assert bool((dead == want).all()), f"{name}: rows at and behind the live count were written"


def dtcode(dt):
    return 1 if dt == BF16 else 0


# ------------------------------------------------------------------------------------------ 1 + 2. ln_gemm, sign bits, gated dH
LN_M = (1, 31, 32, 33, 127, 128, 129, 257)
LN_WALK = [(4097, 1024), (8193, 1024), (32769, 1024), (8193, 768), (32769, 768)]
LN_VARIANTS = ("qkv", "ffn", "one_panel", "three_panels")


def ln_variant(v, dt, M):
    """-> N, act, bias, ldx"""
    if v == "qkv":
        return 768, None, True, 320 if M == 129 else 256
    if v == "ffn":
        return 1024, "relu", True, 256
    if v == "one_panel":
        return (64 if dt == BF16 else 32), None, False, 256
    return (192 if dt == BF16 else 96), "relu", True, 320


def ln_forward(ops, v, N, act, x, gam, bet, w, b):
    """-> dict of outputs as the model names them (+ signs)"""
    if v == "qkv":
        y, xn, st, kn = ops.ln_gemm_qkv(x, gam, bet, w, b)
        return dict(y=y, xn=xn, mean=st[:, 0], rstd=st[:, 1], knorm=kn)
    if v == "ffn":
        y, xn, st, sg = ops.ln_gemm(x, gam, bet, w, b, N, relu=True, want_signs=True)
        return dict(y=y, xn=xn, mean=st[:, 0], rstd=st[:, 1], signs=sg)
    y, xn, st = ops.ln_gemm(x, gam, bet, w, b, N, relu=act == "relu")
    return dict(y=y, xn=xn, mean=st[:, 0], rstd=st[:, 1])


def signs_are_the_outputs_sign(name, signs, y, M_buf, live=None):
    """exact: the decoded bit of every live element is y > 0 -> the gate (bool [live, N])"""
    live = y.shape[0] if live is None else live
    gate = G.decode_signs(signs, M_buf, y.shape[1])[:live]
    assert torch.equal(gate, y[:live] > 0), f"{name}: sign bits differ from y > 0 in {int((gate != (y[:live] > 0)).sum())} places"
    return gate


def run_ln(ops, ck, M, dt, v, seed=0):
    N, act, bias, ldx = ln_variant(v, dt, M)
    p = G.ln_gemm_inputs(M, N, dt, seed=seed, bias=bias, ldx=ldx)
    x, w = put(p["x"], dt), put(p["w"], dt)
    gam, bet, b = put(p["gamma"]), put(p["beta"]), put(p["bias"])
    with sentinel_outputs():
        got = ln_forward(ops, v, N, act, x, gam, bet, w, b)
    ref, e = G.e_chain_of(G.ln_gemm_model, fl(x), gam, bet, fl(w), b, act, dt=dt)
    ck.all("", got, ref, e, bf16_names=("y", "xn") if dt == BF16 else ())
    if v != "ffn":
        return
    # the FFN backward's dH = dY W2 through the ReLU: the gate is the forward's own output (its sign bits in bf16, h itself in fp32)
    q = G.gated_inputs(M, N, dt, seed=seed)
    a, w2 = put(q["a"], dt), put(q["w"], dt)
    if dt == BF16:
        gate = signs_are_the_outputs_sign(ck.tag, got["signs"], got["y"], M)
        with sentinel_outputs():
            dh = ops.gemm_nt_signs(a, w2, got["signs"], GATE_SCALE)
        ref, e = G.e_chain_of(G.gated_model, fl(a), fl(w2), gate, GATE_SCALE, dt=dt)
    else:
        assert got["signs"] is None
        with sentinel_outputs():
            dh = ops.gemm_nt(a, w2, gate=got["y"], gate_scale=GATE_SCALE)
        ref, e = G.e_chain_of(G.gemm_nt_model, fl(a), fl(w2), gate=fl(got["y"]), gate_scale=GATE_SCALE, dt=dt)
    ck.close("dh", dh, ref["y"], e["y"], dt == BF16)


@pytest.mark.parametrize("dt", G.DTS, ids=dn)
@pytest.mark.parametrize("v", LN_VARIANTS)
@pytest.mark.parametrize("M", LN_M)
def test_ln_gemm_at_every_row_edge(ops, M, v, dt):
    """y, xn, mean, 1 / (std + eps) (and the key-norm table, the sign bits and the gated dH) at M on both sides of the wave's 32 and the
    workgroup's 128 rows; bias None (one_panel), x as a column window of a 320-wide buffer (three_panels; qkv at M = 129)"""
    ck = Checks(f"ln_gemm.{v}[M={M},{dn(dt)}]")
    run_ln(ops, ck, M, dt, v)
    ck.done()


@pytest.mark.parametrize("dt", G.DTS, ids=dn)
@pytest.mark.parametrize("M,N", LN_WALK)
def test_ln_gemm_panel_walk(ops, M, N, dt):
    """per = 2, 3 (uneven shares, one workgroup without a panel) and MAXP panels per workgroup: see the module docstring"""
    ck = Checks(f"ln_gemm.walk[M={M},N={N},{dn(dt)}]")
    run_ln(ops, ck, M, dt, "ffn" if N == 1024 else "qkv", seed=1)
    ck.done()


# ------------------------------------------------------------------------------------------ 3. gemm_nt
#          M,   N,    K,   options
NT_CASES = [
    (1, 32, 8, dict(bias=False)),                                          # nk 1, masked: one row, one 32-column piece
    (63, 96, 56, dict(act="relu")),                                        # nk 1, masked
    (64, 128, 64, dict(res=True, ldr=136)),                                # nk 1, whole chunk; residual rows wider than N
    (65, 160, 72, dict(act="gelu", lda=88)),                               # nk 2, tail of 8; A rows wider than K; N tail inside a block
    (128, 256, 96, dict(gate=True)),                                       # nk 2, tail of 32
    (129, 160, 128, dict(row_scale=49)),                                   # nk 2; 129 = 2 * 49 + 31 rows
    (129, 96, 192, dict(res=True, lda=208, ldr=104, act="relu")),          # nk 3: the `break` of the two-in-flight loop
    (65, 32, 200, dict(act="gelu", row_scale=49, res=True)),               # nk 4, tail of 8
    (63, 256, 1024, dict(gate=True, act="relu", bias=False)),              # nk 16
    (1, 160, 192, dict(gate=True, row_scale=49, res=True, ldr=168)),       # every phase-2 option at once
    (64, 96, 72, dict(gate=True, res=True)),
    (128, 128, 200, dict(act="gelu", bias=False, row_scale=49)),
    (129, 256, 56, dict(res=True)),
    (8064, 1024, 72, dict(res=True)),                                      # 63 * 8 = 504 workgroups of 128 rows: the last 64-row launch
    (8193, 1024, 72, dict(res=True)),                                      # 65 * 8 = 520: 128-row tiles, the last one with one row
    (8193, 1024, 72, dict(act="gelu", gate=True, row_scale=49)),
]


def run_nt(ops, ck, prefix, M, N, K, dt, o, live=None, seed=0):
    p = G.nt_inputs(M, N, K, dt, seed=seed, bias=o.get("bias", True), res=o.get("res", False), gate=o.get("gate", False),
                    row_scale=o.get("row_scale", 0), lda=o.get("lda"), ldr=o.get("ldr"))
    a, w, res, gate = (put(p[k], dt) for k in ("a", "w", "res", "gate"))
    b, rsc = put(p["bias"]), put(p["row_scale"])
    rps, gs, act = o.get("row_scale", 0) or 1, GATE_SCALE if o.get("gate") else 1.0, o.get("act")
    L = M if live is None else live
    ref, e = G.e_chain_of(G.gemm_nt_model, fl(a)[:L], fl(w), b, None if res is None else fl(res)[:L], act,
                          None if gate is None else fl(gate)[:L], gs, rsc, rps, dt=dt)
    if live is not None:
        for t in (a, res, gate):
            poison(t, live)
    table = None if live is None else torch.tensor([M, live, 0, 0], dtype=torch.int32, device=DEV)
    with sentinel_outputs(), ops.rows_live(table, 1):
        y = ops.gemm_nt(a, w, b, res, act, gate=gate, gate_scale=gs, row_scale=rsc, rows_per_scale=rps)
    if live is not None:
        dead_rows_untouched(ck.tag, y, live)
    ck.close(prefix + "y", y[:L], ref["y"], e["y"], dt == BF16)


def _nt_id(c):
    M, N, K, o = c
    return f"{M}x{N}x{K}-" + ("+".join(f"{k}={v}" if not isinstance(v, bool) else (k if v else "no" + k) for k, v in sorted(o.items())) or "plain")


@pytest.mark.parametrize("dt", G.DTS, ids=dn)
@pytest.mark.parametrize("c", NT_CASES, ids=_nt_id)
def test_gemm_nt_covering_set(ops, c, dt):
    M, N, K, o = c
    ck = Checks(f"gemm_nt[{_nt_id(c)},{dn(dt)}]")
    run_nt(ops, ck, "", M, N, K, dt, o)
    ck.done()


@pytest.mark.parametrize("dt", G.DTS, ids=dn)
@pytest.mark.parametrize("M,live", [(129, 129), (129, 128), (129, 65), (129, 64), (129, 1)])
def test_gemm_nt_live_row_word(ops, M, live, dt):
    """the rows-in-use word of the frozen encoder's launches (ops.rows_live): M, M - 1, both sides of the 64-row tile, 1"""
    ck = Checks(f"gemm_nt.live[M={M},live={live},{dn(dt)}]")
    run_nt(ops, ck, "", M, 160, 200, dt, dict(act="gelu", row_scale=49, res=True, ldr=168), live=live, seed=3)
    ck.done()


# ------------------------------------------------------------------------------------------ 4. gemm_lnbwd
#             M,   K,  d_res, ldz, ldr
LNBWD_CASES = [(1, 64, True, 256, 256), (63, 72, False, 256, 256), (64, 768, True, 256, 264), (65, 1024, True, 320, 256),
               (127, 72, True, 256, 256), (128, 64, False, 320, 256), (129, 1024, True, 320, 264), (257, 768, True, 256, 256),
               (129, 72, True, 256, 264), (257, 64, False, 256, 256)]


def lnbwd_ref(p, dt, L=None):
    L = p["z"].shape[0] if L is None else L
    return G.e_chain_of(G.gemm_lnbwd_model, p["dy"][:L], p["wt"], p["z"][:L], p["stats"][:L], p["gamma"],
                        None if p["d_res"] is None else p["d_res"][:L], dt=dt)


@pytest.mark.parametrize("dt", G.DTS, ids=dn)
@pytest.mark.parametrize("M,K,res,ldz,ldr", LNBWD_CASES)
def test_gemm_lnbwd_at_every_slab_edge(ops, M, K, res, ldz, ldr, dt):
    """dz, dgamma, dbeta with the partials reduced inside the call and deferred through reduce_batch"""
    p = G.lnbwd_inputs(M, K, dt, res=res, ldz=ldz, ldr=ldr)
    dy, wt, z, d_res = (put(p[k], dt) for k in ("dy", "wt", "z", "d_res"))
    st, gam = put(p["stats"]), put(p["gamma"])
    ref, e = lnbwd_ref(p, dt)
    ck = Checks(f"gemm_lnbwd[M={M},K={K},{'res' if res else 'nores'},ldz={ldz},ldr={ldr},{dn(dt)}]")
    for form in ("now", "deferred"):
        defer = None if form == "now" else []
        with sentinel_outputs():
            dz, dg, db = ops.gemm_lnbwd(dy, wt, z, st, gam, d_res, defer=defer)
            if defer is not None:
                assert len(defer) == 1
                ops.reduce_batch(defer)
        ck.all(form + ".", dict(dz=dz, dgamma=dg, dbeta=db), ref, e, bf16_names=("dz",) if dt == BF16 else ())
    ck.done()


# ------------------------------------------------------------------------------------------ 5. gemm_tn, 128-multiple kernels
def run_tn(ops, lib, ck, prefix, M, N, K, dt, off=None, live=None, seed=0, want_splits=None, p=None):
    p = p or G.tn_inputs(M, N, K, dt, seed=seed, off=off)
    dy, x = put(p["dy"], dt), put(p["x"], dt)
    splits = lib.mtmp_gemm_tn_slab_rows(dtcode(dt), M, N, K)
    if want_splits is not None:
        assert splits == want_splits, (splits, want_splits)
    L = M if live is None else live
    ref, e = G.e_chain_of(G.gemm_tn_model, fl(dy)[:L], fl(x)[:L], splits, dt=dt)
    poison(dy, L), poison(x, L)
    with sentinel_outputs():
        dw, db = ops.gemm_tn(dy, x, pack=None if live is None else pack_word(live))
    ck.all(prefix, dict(dw=dw, db=db), ref, e)
    return dw, db


@pytest.mark.parametrize("dt", G.DTS, ids=dn)
@pytest.mark.parametrize("M", [1, 63, 64, 65, 255, 256, 257])
def test_gemm_tn_mode0_token_edges(ops, lib, M, dt):
    """one 128 x 128 tile; fp32: gemm_tn_kernel, bf16: the transposing-read kernel with one token group (two 64-token stages in
    flight: 1 .. 5 steps, odd and even; M = 257: two splits of 192 and 65 rows)"""
    ck = Checks(f"gemm_tn.mode0[M={M},{dn(dt)}]")
    run_tn(ops, lib, ck, "", M, 128, 128, dt, want_splits=(M + 255) // 256)
    ck.done()


@pytest.mark.parametrize("dt", G.DTS, ids=dn)
@pytest.mark.parametrize("live", [257, 256, 65, 64, 1])
def test_gemm_tn_mode0_packed_and_empty_split(ops, lib, live, dt):
    """the splits share the LIVE rows: live 64 and 1 leave split 1 without rows (its slab row must be zeros)"""
    ck = Checks(f"gemm_tn.mode0.packed[M=257,live={live},{dn(dt)}]")
    run_tn(ops, lib, ck, "", 257, 128, 128, dt, live=live, seed=2, want_splits=2)
    ck.done()


def test_gemm_tn_fp32_split_without_rows(ops, lib):
    """64 tiles cap the split count at 10: rows per split 320, 9 * 320 >= 2561 -- split 8 has one row, split 9 none"""
    ck = Checks("gemm_tn.mode0.capped[M=2561,1024x1024,fp32]")
    run_tn(ops, lib, ck, "", 2561, 1024, 1024, F32, want_splits=10)
    ck.done()


#           mode, N,    K
TN_LARGE = [(3, 256, 1024), (1, 2048, 128)]


@pytest.mark.parametrize("M,splits", [(6143, 24), (6144, 12), (6181, 12)])
@pytest.mark.parametrize("mode,N,K", TN_LARGE)
def test_gemm_tn_two_group_and_dma_kernels(ops, lib, mode, N, K, M, splits):
    """bf16: M = 6144 is the smallest that selects mode 1 (K < 256) / mode 3 (the LDS-DMA kernel), 6143 still runs one token group at 24
    splits, 6181 ends 37 rows into a stage of split 10 and leaves split 11 without rows"""
    ck = Checks(f"gemm_tn.mode{mode}[M={M},{N}x{K},bf16]")
    run_tn(ops, lib, ck, "", M, N, K, BF16, want_splits=splits)
    ck.done()


def test_gemm_tn_window_that_falls_back_from_the_dma_kernel(ops, lib):
    """16-byte aligned column windows go through the DMA kernel; windows that start 4 bytes into a row cannot: the two-group
    register-staged kernel at the same split count"""
    ck = Checks("gemm_tn.mode3.window[M=6181,256x1024,bf16]")
    run_tn(ops, lib, ck, "aligned.", 6181, 256, 1024, BF16, off=(64, 64), seed=4, want_splits=12)
    run_tn(ops, lib, ck, "by4bytes.", 6181, 256, 1024, BF16, off=(2, 6), seed=4, want_splits=12)
    ck.done()


# ------------------------------------------------------------------------------------------ 6. grouped launches, packed streams
#           name -> (M per stream, rows in use per stream | None)
GROUPS = {"dense": ((129, 1, 64), None),
          "packedA": ((257, 129, 64), (257, 128, 1)),          # M, M - 1 = a tile edge, 1
          "packedB": ((257, 129, 64), (128, 1, 63))}           # a tile edge, 1, M - 1
TN_GROUPS = {"dense": ((6181, 129, 64), None),
             "packedA": ((6181, 129, 64), (6181, 128, 1)),
             "packedB": ((6181, 129, 64), (6144, 1, 63))}


def _packs(lives, dt):
    """per stream what the grouped wrappers take: bf16 the row_starts() tensor, fp32 the live count itself"""
    if lives is None:
        return None
    return [pack_word(L) if dt == BF16 else L for L in lives]


def _lives(Ms, lives):
    return list(Ms) if lives is None else list(lives)


@pytest.mark.parametrize("dt", G.DTS, ids=dn)
@pytest.mark.parametrize("gname", list(GROUPS))
def test_grouped_qkv_projection(ops, gname, dt):
    Ms, lives = GROUPS[gname]
    Ls = _lives(Ms, lives)
    ps = [G.ln_gemm_inputs(M, 768, dt, seed=20 + i, ldx=320 if i == 0 else 256) for i, M in enumerate(Ms)]
    xs, ws = [put(p["x"], dt) for p in ps], [put(p["w"], dt) for p in ps]
    gs, bs, cs = ([put(p[k]) for p in ps] for k in ("gamma", "beta", "bias"))
    refs = [G.e_chain_of(G.ln_gemm_model, fl(x)[:L], g, b, fl(w), c, dt=dt) for x, g, b, w, c, L in zip(xs, gs, bs, ws, cs, Ls)]
    for x, L in zip(xs, Ls):
        poison(x, L)
    with sentinel_outputs():
        y, xn, st, kn = ops.ln_gemm_qkv_grouped(xs, gs, bs, ws, cs, _packs(lives, dt))
    ck = Checks(f"grouped.qkv.{gname}[{dn(dt)}]")
    for i, L in enumerate(Ls):
        nb = (L + 31) // 32
        for name, t in (("y", y[i]), ("xn", xn[i]), ("stats", st[i])):
            dead_rows_untouched(f"{ck.tag}.s{i}.{name}", t, L)
        if kn[i].shape[0] > nb:                                   # (the table of a packed bf16 stream keeps the buffer's block count)
            dead_rows_untouched(f"{ck.tag}.s{i}.knorm", kn[i], nb)
        got = dict(y=y[i][:L], xn=xn[i][:L], mean=st[i][:L, 0], rstd=st[i][:L, 1], knorm=kn[i][:nb])
        ck.all(f"s{i}.", got, refs[i][0], refs[i][1], bf16_names=("y", "xn") if dt == BF16 else ())
    ck.done()


@pytest.mark.parametrize("dt", G.DTS, ids=dn)
@pytest.mark.parametrize("gname", list(GROUPS))
def test_grouped_ffn1_signs_and_gated_dh(ops, gname, dt):
    """FFN1 with sign bits and the gated dH behind it, three streams per launch: every stream against the model of its live rows; the
    sign words of rows behind the live count keep the sentinel"""
    Ms, lives = GROUPS[gname]
    Ls, N = _lives(Ms, lives), 1024
    ps = [G.ln_gemm_inputs(M, N, dt, seed=30 + i) for i, M in enumerate(Ms)]
    qs = [G.gated_inputs(M, N, dt, seed=30 + i) for i, M in enumerate(Ms)]
    xs, ws = [put(p["x"], dt) for p in ps], [put(p["w"], dt) for p in ps]
    gs, bs, cs = ([put(p[k]) for p in ps] for k in ("gamma", "beta", "bias"))
    as_, w2s = [put(q["a"], dt) for q in qs], [put(q["w"], dt) for q in qs]
    refs = [G.e_chain_of(G.ln_gemm_model, fl(x)[:L], g, b, fl(w), c, "relu", dt=dt) for x, g, b, w, c, L in zip(xs, gs, bs, ws, cs, Ls)]
    a_live = [fl(a)[:L] for a, L in zip(as_, Ls)]
    for t, L in zip(xs + as_, Ls + Ls):
        poison(t, L)
    packs = _packs(lives, dt)
    with sentinel_outputs():
        y, xn, st, sg = ops.ln_gemm_signs_grouped(xs, gs, bs, ws, cs, N, 0.0, [1, 2, 3], packs)
        dh, ad = ops.gemm_nt_signs_drop_grouped(as_, w2s, sg, GATE_SCALE, 0.0, [1, 2, 3], packs, gates=y)
    ck = Checks(f"grouped.ffn1.{gname}[{dn(dt)}]")
    for i, (M, L) in enumerate(zip(Ms, Ls)):
        for name, t in (("y", y[i]), ("xn", xn[i]), ("stats", st[i]), ("dh", dh[i])):
            dead_rows_untouched(f"{ck.tag}.s{i}.{name}", t, L)
        got = dict(y=y[i][:L], xn=xn[i][:L], mean=st[i][:L, 0], rstd=st[i][:L, 1])
        ck.all(f"s{i}.", got, refs[i][0], refs[i][1], bf16_names=("y", "xn") if dt == BF16 else ())
        if dt == BF16:
            gate = signs_are_the_outputs_sign(f"{ck.tag}.s{i}", sg[i], y[i], M, L)
            assert bool((sg[i][~G.live_words(sg[i], M, N, L)] == SENTINEL_BYTE).all()), f"s{i}: sign words of dead rows were written"
            assert ad[i] is as_[i]                                # (no dropout: the operand itself is the weight gradient's)
        else:
            assert sg[i] is None
            gate = y[i][:L] > 0
        ref, e = G.e_chain_of(G.gated_model, a_live[i], fl(w2s[i]), gate, GATE_SCALE, dt=dt)
        ck.close(f"s{i}.dh", dh[i][:L], ref["y"], e["y"], dt == BF16)
    ck.done()


@pytest.mark.parametrize("dt", G.DTS, ids=dn)
@pytest.mark.parametrize("gname", list(GROUPS))
def test_grouped_ffn2(ops, gname, dt):
    """gemm_nt_grouped: y = a W^T + b + res at K = 1024, N = 256 (the 64-row tiles of the grouped grid)"""
    Ms, lives = GROUPS[gname]
    Ls = _lives(Ms, lives)
    ps = [G.nt_inputs(M, 256, 1024, dt, seed=40 + i, res=True, lda=1040 if i == 0 else None) for i, M in enumerate(Ms)]
    as_, ws, rs = ([put(p[k], dt) for p in ps] for k in ("a", "w", "res"))
    bs = [put(p["bias"]) for p in ps]
    refs = [G.e_chain_of(G.gemm_nt_model, fl(a)[:L], fl(w), b, fl(r)[:L], dt=dt) for a, w, b, r, L in zip(as_, ws, bs, rs, Ls)]
    for t, L in zip(as_ + rs, Ls + Ls):
        poison(t, L)
    with sentinel_outputs():
        y = ops.gemm_nt_grouped(as_, ws, bs, rs, 0.0, [1, 2, 3], _packs(lives, dt))
    ck = Checks(f"grouped.ffn2.{gname}[{dn(dt)}]")
    for i, L in enumerate(Ls):
        dead_rows_untouched(f"{ck.tag}.s{i}.y", y[i], L)
        ck.close(f"s{i}.y", y[i][:L], refs[i][0]["y"], refs[i][1]["y"], dt == BF16)
    ck.done()


@pytest.mark.parametrize("dt", G.DTS, ids=dn)
@pytest.mark.parametrize("gname", list(GROUPS))
def test_grouped_gemm_lnbwd(ops, gname, dt):
    """three streams, partials deferred: the row blocks behind a packed stream's live rows contribute zeros to dgamma / dbeta"""
    Ms, lives = GROUPS[gname]
    Ls, K = _lives(Ms, lives), 768
    ps = [G.lnbwd_inputs(M, K, dt, seed=50 + i, res=i != 1, ldz=320 if i == 0 else 256, ldr=264 if i == 2 else 256) for i, M in enumerate(Ms)]
    dys, wts, zs, drs = ([put(p[k], dt) for p in ps] for k in ("dy", "wt", "z", "d_res"))
    sts, gms = [put(p["stats"]) for p in ps], [put(p["gamma"]) for p in ps]
    for t, L in zip(dys + zs + drs + sts, Ls * 4):
        poison(t, L)
    defers = [[] for _ in Ms]
    with sentinel_outputs():
        out = ops.gemm_lnbwd_grouped(dys, wts, zs, sts, gms, drs, [None] * 3, defers, _packs(lives, dt))
        pending = [e for d in defers for e in d]
        assert len(pending) == 3
        ops.reduce_batch(pending)
    ck = Checks(f"grouped.lnbwd.{gname}[{dn(dt)}]")
    for i, L in enumerate(Ls):
        dz, dg, db = out[i]
        dead_rows_untouched(f"{ck.tag}.s{i}.dz", dz, L)
        ref, e = lnbwd_ref(ps[i], dt, L)
        ck.all(f"s{i}.", dict(dz=dz[:L], dgamma=dg, dbeta=db), ref, e, bf16_names=("dz",) if dt == BF16 else ())
    ck.done()


@pytest.mark.parametrize("dt", G.DTS, ids=dn)
@pytest.mark.parametrize("gname", list(TN_GROUPS))
def test_grouped_gemm_tn(ops, lib, gname, dt):
    """the longest stream takes mode 3, so the bf16 launch is ONE grid of the LDS-DMA kernel over all three streams (the short ones as
    single splits of 1 .. 3 stages); packed: every split takes its share of the live rows"""
    import ctypes
    Ms, lives = TN_GROUPS[gname]
    Ls, N, K = _lives(Ms, lives), 256, 1024
    ps = [G.tn_inputs(M, N, K, dt, seed=60 + i, off=(64, 0) if i == 0 else None) for i, M in enumerate(Ms)]
    dys, xs = [put(p["dy"], dt) for p in ps], [put(p["x"], dt) for p in ps]
    if dt == BF16:
        plan = (ctypes.c_int * 3)()
        assert lib.mtmp_gemm_tn_group_plan(3, (ctypes.c_int * 3)(*Ms), N, K, plan) == 0
        splits = list(plan)
        assert splits == [12, 1, 1], splits
    else:                                                       # fp32: one gemm_tn per stream, on its live rows when packed
        splits = [lib.mtmp_gemm_tn_slab_rows(0, L if lives is not None else M, N, K) for M, L in zip(Ms, Ls)]
    refs = [G.e_chain_of(G.gemm_tn_model, fl(dy)[:L], fl(x)[:L], s, dt=dt) for dy, x, L, s in zip(dys, xs, Ls, splits)]
    for t, L in zip(dys + xs, Ls + Ls):
        poison(t, L)
    defers = [[] for _ in Ms]
    with sentinel_outputs():
        out = ops.gemm_tn_grouped(dys, xs, [None] * 3, defers, _packs(lives, dt))
        pending = [e for d in defers for e in d]
        assert len(pending) == 3
        ops.reduce_batch(pending)
    ck = Checks(f"grouped.tn.{gname}[{dn(dt)}]")
    for i in range(3):
        ck.all(f"s{i}.", dict(dw=out[i][0], db=out[i][1]), refs[i][0], refs[i][1])
    ck.done()


# ------------------------------------------------------------------------------------------ 7. one-tile probes
@pytest.mark.parametrize("dt", G.DTS, ids=dn)
def test_probe_k_tail_chunk_of_gemm_nt(ops, dt):
    """the 8 columns of the K tail carry 128 times the mass of the chunk in front (tests/test_gemm_model_cpu.py: bound <= 0.25, err >= 0.5
    without them); the one row of the last row tile also as a tensor of its own"""
    p = G.nt_probe_inputs(dt)
    a, w = put(p["a"], dt), put(p["w"], dt)
    y = ops.gemm_nt(a, w)
    ref, ch = (G.gemm_nt_model(fl(a), fl(w), dt=dt, ft=ft)["y"] for ft in (F64, F32))
    ck = Checks(f"probe.nt_k_tail[{dn(dt)}]")
    ck.close("y", y, ref, G.err(ch, ref), dt == BF16)
    ck.close("y[64:]", y[64:], ref[64:], G.err(ch[64:], ref[64:]), dt == BF16)
    assert REPORT[f"{ck.tag}.y"]["bound"] <= G.PROBE_BOUND
    ck.done()


def test_probe_last_panel_of_a_share(ops):
    """ln_gemm_dma_kernel at M = 8193, N = 1024 (shares of 3 3 3 3 3 1 panels): y in the last panel of every share of three is its bias
    (32 times the usual); those panels' columns also as tensors of their own"""
    dt = BF16
    p = G.panel_probe_inputs(dt)
    x, w = put(p["x"], dt), put(p["w"], dt)
    gam, bet, b = put(p["gamma"]), put(p["beta"]), put(p["bias"])
    y, _, _, sg = ops.ln_gemm(x, gam, bet, w, b, 1024, relu=True, want_signs=True)
    ref, ch = (G.ln_gemm_model(fl(x), gam, bet, fl(w), b, "relu", dt=dt, ft=ft)["y"] for ft in (F64, F32))
    ck = Checks("probe.ln_gemm_last_panel[bf16]")
    ck.close("y", y, ref, G.err(ch, ref), True)
    assert REPORT[f"{ck.tag}.y"]["bound"] <= G.PROBE_BOUND
    for j in G.panel_probe_panels():
        c = slice(64 * j, 64 * j + 64)
        ck.close(f"y[panel {j}]", y[:, c], ref[:, c], G.err(ch[:, c], ref[:, c]), True)
    signs_are_the_outputs_sign(ck.tag, sg, y, G.PANEL_PROBE["M"])
    ck.done()


def test_probe_last_token_step_of_a_gemm_tn_split(ops, lib):
    """mode 3 at M = 6700: the 44 rows of the last stage of the last split carry 64^2 times the mass of a row in front"""
    M, N, K = (G.TN_PROBE[k] for k in ("M", "N", "K"))
    splits = lib.mtmp_gemm_tn_slab_rows(1, M, N, K)
    assert splits == 12
    ck = Checks("probe.tn_last_step[bf16]")
    run_tn(ops, lib, ck, "", M, N, K, BF16, want_splits=12, p=G.tn_probe_inputs(BF16, splits))
    assert REPORT[f"{ck.tag}.dw"]["bound"] <= G.PROBE_BOUND and REPORT[f"{ck.tag}.db"]["bound"] <= G.PROBE_BOUND
    ck.done()
