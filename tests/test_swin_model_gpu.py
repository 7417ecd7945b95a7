"""-m gpu: the Swin image-encoder kernels of csrc/swin.hip, csrc/swin_bwd.hip and csrc/stem.hip against the float64 models of
tests/swin_model.py, element by element, through the wrappers of ops.py.  Metric and bound: see swin_model.py -- every output tensor
of a launch (live rows only) meets max(8 e_chain, 16 * 2^-24) (+ 2^-8 for a bf16 output), e_chain being the error of the
working-precision chain against the float64 chain; nothing is fitted to what the kernels return.  Operands are rounded to the
compute type on both sides.  The models run on the CPU, those of the grid-stride wraps on the device.  Buffers the wrappers allocate
start as a sentinel; rows or images past a live word are NaN on the way in and must hold the sentinel bit for bit on the way out.
Every check appends {err, e_chain, bound, ratio} to a report: build/swin_model_report.json, or the file MTMP_SWIN_MODEL_REPORT names.

Shapes, from the launchers:
  layernorm_rows(_bwd): a group of G = 16 | 32 | 64 lanes owns a row, a lane NCH chunks of 8 channels: C 8 (one live lane) and 96 ->
      (16, 1), 192 -> (32, 1), 384 -> (64, 1), 768 -> (64, 2), 1536 -> (64, 3).  A wave holds RPW = 64 / G rows, a workgroup 4 RPW; the
      forward's grid stops at 4096 workgroups (65536 rows at C 96, 16384 at C >= 384), the backward's at 1024 (16384 / 4096), one row
      more starts the second trip.  Merge mode: 4 Cs = 384, 768, 1536; 6 x 10 is not square; 15 merged rows of width 96 end inside a
      wave's four rows, 3 of width 384 inside a workgroup's four.
  gelu: 8 elements per thread, 256 threads, 8192 workgroups at the most: n = 8, 2048 + 8 (a second workgroup), 8192 * 2048 + 8.
  window attention: one wave per (image, window, head), 4 per workgroup: (1, 7, 7, 3) leaves a dead wave.  The window type is 0 at
      shift 0, else 2 (last window row) + (last window column): 14 x 14 has one window of each, 14 x 21 / 21 x 14 tell rows from columns.
      Padded maps: 5 x 5 one window; 8 x 8 six pad rows / columns, 13 x 13 one; 9 x 16 / 16 x 9; 15 x 15 where the shift wraps pad tokens
      into the interior of the last windows.
  swin_mlp: 128 rows per workgroup, 32 per wave; C 96: 6 panels of 64 hidden units, C 192: 24 of 32.  swin_ln_linear: the same rows,
      N / 32 groups of output features.  swin_attn_block: one workgroup per window, one wave per head; C 96: two lanes per token and
      the projection's weights prefetched, C 192: four lanes per token, the projection streamed.
  stem: one patch per lane pair's column: 32 per wave, 128 per workgroup.
"""
import contextlib
import json
import math
import os
import time

import pytest
import torch

from tests import swin_model as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
REPORT = {}
SENTINEL = 768.0                       # (exact in bf16) what the wrappers' float buffers hold before a launch
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
    path = os.environ.get("MTMP_SWIN_MODEL_REPORT") or os.path.join(ROOT, "build", "swin_model_report.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    REPORT["_wall_seconds"] = time.time() - T0
    with open(path, "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


class Checks:
    """collects the checks of one test: every figure is printed and recorded before the test asserts"""

    def __init__(self, tag):
        self.tag, self.failed = tag, []

    def close(self, name, got, ref, e_chain, bf16_out=False):
        key = f"{self.tag}.{name}"
        assert key not in REPORT, key
        finite = bool(torch.isfinite(got).all())
        e, b = (S.err(got, ref) if finite else math.inf), S.bound(e_chain, bf16_out)
        REPORT[key] = {"err": e, "e_chain": e_chain, "bound": b, "ratio": e / b}
        print(f"{key}: err {e:.3e} e_chain {e_chain:.3e} bound {b:.3e} ratio {e / b:.3f}")
        if not (math.isfinite(e) and e <= b):
            self.failed.append(f"{key}: err {e:.3e} > bound {b:.3e} (e_chain {e_chain:.3e})")

    def all(self, prefix, got, ref, e, bf16_names=()):
        for name in got:
            self.close(prefix + name, got[name], ref[name], e[name], name in bf16_names)

    def exact(self, name, ok):
        if not ok:
            self.failed.append(f"{self.tag}.{name}")

    def done(self):
        assert not self.failed, "\n".join(self.failed)


def dn(dt):
    return S.dt_name(dt)


@contextlib.contextmanager
def sentinel_outputs():
    """the buffers that the wrappers allocate for a launch start out as SENTINEL, so an element the kernels do not write shows;
    yields the list of those buffers"""
    empty, empty_like = torch.empty, torch.empty_like
    made = []

    def fill(t):
        if t.is_floating_point():
            t.fill_(SENTINEL)
        made.append(t)
        return t

    torch.empty = lambda *a, **k: fill(empty(*a, **k))
    torch.empty_like = lambda *a, **k: fill(empty_like(*a, **k))
    try:
        yield made
    finally:
        torch.empty, torch.empty_like = empty, empty_like


def put(t, dt=F32):
    return None if t is None else t.to(DEV, dt).contiguous()


def word(v):
    return torch.tensor([int(v)], dtype=torch.int32, device=DEV)


def poison(t, live):
    """leading rows / images behind the live ones are NaN: reading one shows in the output"""
    if live < t.shape[0]:
        t[live:] = float("nan")
    return t


def untouched(ck, name, t, live):
    ck.exact(f"{name}: rows at and behind the live count were written", bool((t[live:] == SENTINEL).all()))


def e_of(model, *args, dt, **kw):
    return S.e_chain_of(model, *args, dt=dt, **kw)


def both(model, *args, dt, **kw):
    """(float64 outputs, working-precision outputs, {name: e_chain}): for checks on a part of an output tensor"""
    ref, ch = model(*args, dt=dt, ft=F64, **kw), model(*args, dt=dt, ft=F32, **kw)
    return ref, ch, {k: S.err(ch[k], ref[k]) for k in ref}


# ------------------------------------------------------------------------------------------ 1. layernorm_rows
def run_ln(ops, ck, prefix, rows, C, dt, live=None, device="cpu", seed=0):
    p = S.ln_inputs(rows, C, dt, seed=seed, device=device)
    L = rows if live is None else live
    ref, e = e_of(S.ln_rows_model, p["x"][:L], p["w"], p["b"], dt=dt)
    x = poison(put(p["x"], dt), L)
    with sentinel_outputs(), ops.rows_live(None if live is None else word(live), 0):
        y = ops.layernorm_rows(x, put(p["w"]), put(p["b"]))
    if live is not None:
        untouched(ck, prefix + "y", y, L)
    ck.close(prefix + "y", y[:L], ref["y"], e["y"], dt == BF16)


@pytest.mark.parametrize("dt", S.DTS, ids=dn)
@pytest.mark.parametrize("C", S.LN_WIDTHS)
def test_layernorm_rows_at_every_row_edge(ops, C, dt):
    """rows on both sides of RPW and of a workgroup's 4 RPW; a live word below, at and inside a row group of a two-workgroup buffer"""
    ck = Checks(f"layernorm_rows[C={C},{dn(dt)}]")
    for rows in S.ln_rows_cases(C):
        run_ln(ops, ck, f"rows={rows}.", rows, C, dt)
    rpw = S.ln_rpw(C)
    for live in sorted({1, rpw, rpw + 1, 4 * rpw + 2}):
        run_ln(ops, ck, f"live={live}.", 8 * rpw + 1, C, dt, live=live, seed=1)
    ck.done()


@pytest.mark.parametrize("dt", S.DTS, ids=dn)
@pytest.mark.parametrize("C,rows", S.LN_WRAP)
def test_layernorm_rows_grid_wrap(ops, C, rows, dt):
    """4096 workgroups: the last row is the second trip of workgroup 0"""
    ck = Checks(f"layernorm_rows.wrap[C={C},rows={rows},{dn(dt)}]")
    run_ln(ops, ck, "", rows, C, dt, device=DEV)
    p = S.ln_inputs(rows, C, dt, device=DEV)
    ref, e = e_of(S.ln_rows_model, p["x"][rows - 1:], p["w"], p["b"], dt=dt)
    y = ops.layernorm_rows(p["x"].to(dt), p["w"], p["b"])
    ck.close("y[last row]", y[rows - 1:], ref["y"], e["y"], dt == BF16)
    ck.done()


@pytest.mark.parametrize("dt", S.DTS, ids=dn)
@pytest.mark.parametrize("n,H,W,Cs", S.MERGE_CASES)
def test_layernorm_rows_merge_mode(ops, n, H, W, Cs, dt):
    ck = Checks(f"layernorm_rows.merge[{n}x{H}x{W}x{Cs},{dn(dt)}]")
    p = S.merge_inputs(n, H, W, Cs, dt)
    ref, e = e_of(S.ln_rows_model, p["x"], p["w"], p["b"], merge_hw=(H, W), dt=dt)
    with sentinel_outputs():
        y = ops.layernorm_rows(put(p["x"], dt), put(p["w"]), put(p["b"]), merge_hw=(H, W))
    ck.close("y", y, ref["y"], e["y"], dt == BF16)
    if n > 1:                                                   # one image in use: the merged rows of the others stay
        per = (H // 2) * (W // 2)
        x = poison(put(p["x"], dt), 1)
        with sentinel_outputs(), ops.rows_live(word(per), 0):
            y = ops.layernorm_rows(x, put(p["w"]), put(p["b"]), merge_hw=(H, W))
        untouched(ck, "live.y", y, 1)
        ck.close("live.y", y[:1], ref["y"][:1], S.err(S.ln_rows_model(p["x"][:1], p["w"], p["b"], merge_hw=(H, W), dt=dt, ft=F32)["y"],
                                                      ref["y"][:1]), dt == BF16)
    ck.done()


# ------------------------------------------------------------------------------------------ 2. layernorm_rows_bwd
def run_ln_bwd(ops, lib, ck, prefix, rows, C, dt, device="cpu", p=None):
    p = p or S.ln_inputs(rows, C, dt, device=device)
    ref, e = e_of(S.ln_rows_bwd_model, p["x"], p["w"], p["dy"], dt=dt)
    with sentinel_outputs() as made:
        dx, dw, db = ops.layernorm_rows_bwd(put(p["x"], dt), put(p["w"]), put(p["dy"], dt))
    slabs = [t for t in made if t.dim() == 3 and tuple(t.shape[1:]) == (2, C)]
    want = lib.mtmp_layernorm_rows_bwd_slab_rows(rows, C)
    ck.exact(f"{prefix}slab rows {[t.shape[0] for t in slabs]} != {want}",
             len(slabs) == 1 and slabs[0].shape[0] == want == S.ln_bwd_slab_rows(rows, C))
    ck.all(prefix, dict(dx=dx, dw=dw, db=db), ref, e, bf16_names=("dx",) if dt == BF16 else ())


@pytest.mark.parametrize("dt", S.DTS, ids=dn)
@pytest.mark.parametrize("C", S.LN_WIDTHS)
def test_layernorm_rows_bwd_at_every_row_edge(ops, lib, C, dt):
    ck = Checks(f"layernorm_rows_bwd[C={C},{dn(dt)}]")
    for rows in S.ln_bwd_rows_cases(C):
        run_ln_bwd(ops, lib, ck, f"rows={rows}.", rows, C, dt)
    ck.done()


@pytest.mark.parametrize("dt", S.DTS, ids=dn)
@pytest.mark.parametrize("C,rows", S.LN_BWD_WRAP)
def test_layernorm_rows_bwd_grid_wrap(ops, lib, C, rows, dt):
    ck = Checks(f"layernorm_rows_bwd.wrap[C={C},rows={rows},{dn(dt)}]")
    run_ln_bwd(ops, lib, ck, "", rows, C, dt, device=DEV)
    ck.done()


@pytest.mark.parametrize("dt", S.DTS, ids=dn)
def test_probe_second_trip_of_layernorm_rows_bwd(ops, lib, dt):
    """dy is zero outside the rows of the second trip: dw / db are that trip's term alone (tests/test_swin_model_cpu.py: bound <= 0.25,
    err >= 0.5 without it)"""
    ck = Checks(f"probe.ln_bwd_second_trip[{dn(dt)}]")
    run_ln_bwd(ops, lib, ck, "", S.LN_BWD_PROBE["rows"], S.LN_BWD_PROBE["C"], dt, p=S.ln_bwd_probe_inputs(dt, device=DEV))
    assert REPORT[f"{ck.tag}.dw"]["bound"] <= S.PROBE_BOUND and REPORT[f"{ck.tag}.db"]["bound"] <= S.PROBE_BOUND
    ck.done()


# ------------------------------------------------------------------------------------------ 3. gelu
@pytest.mark.parametrize("dt", S.DTS, ids=dn)
@pytest.mark.parametrize("n", S.GELU_N)
def test_gelu_forward_and_backward(ops, n, dt):
    ck = Checks(f"gelu[n={n},{dn(dt)}]")
    dev = DEV if n > 100000 else "cpu"
    p = S.gelu_inputs(n, dt, device=dev)
    ref, e = e_of(S.gelu_model, p["x"], dt=dt)
    refg, eg = e_of(S.gelu_grad_model, p["x"], p["dy"], dt=dt)
    with sentinel_outputs():
        y = ops.gelu_fwd(put(p["x"], dt))
        dx = ops.gelu_bwd(put(p["x"], dt), put(p["dy"], dt))
    ck.close("y", y, ref["y"], e["y"], dt == BF16)
    ck.close("dx", dx, refg["dx"], eg["dx"], dt == BF16)
    ck.close("y[last 8]", y[-8:], ref["y"][-8:], S.err(S.gelu_model(p["x"][-8:], dt=dt, ft=F32)["y"], ref["y"][-8:]), dt == BF16)
    ck.done()


# ------------------------------------------------------------------------------------------ 4. window attention
def run_wattn(ops, ck, prefix, c, dt, p=None, n_live=None, want_bwd=True):
    """forward and backward of one case through the entry its map selects -> (outputs, reference)"""
    n, H, W, heads, shift = c
    C = heads * S.DH
    padded = H % 7 != 0 or W % 7 != 0
    p = p or S.attn_inputs(n, H, W, heads, dt, pad=padded)
    L = n if n_live is None else n_live
    ref, chain, e = both(S.window_attn_model, p["qkv"][:L], p["rpb"], heads, shift, p["bias"], p["d_out"][:L] if want_bwd else None, dt=dt)
    qkv, tab, bias = poison(put(p["qkv"], dt), L), put(S.table_model(p["rpb"], heads, shift, dt), dt), put(p["bias"])
    with sentinel_outputs(), ops.rows_live(None if n_live is None else word(L * H * W), 0):
        o = ops.swin_window_attn_pad(qkv, bias, tab, heads, shift) if padded else ops.swin_window_attn(qkv, tab, heads, shift)
    if n_live is not None:
        untouched(ck, prefix + "o", o, L)
    ck.close(prefix + "o", o[:L], ref["o"], e["o"], dt == BF16)
    got = dict(o=o)
    if want_bwd:
        d_out = put(p["d_out"], dt)
        with sentinel_outputs():
            if padded:
                dqkv, dtab, dbias = ops.swin_window_attn_pad_bwd(qkv, bias, tab, d_out, heads, shift)
                got["dbias"] = dbias
            else:
                dqkv, dtab = ops.swin_window_attn_bwd(qkv, tab, d_out, heads, shift)
        got.update(dqkv=dqkv, dtab=dtab)
        ck.close(prefix + "dqkv", dqkv, ref["dqkv"], e["dqkv"], dt == BF16)
        ck.close(prefix + "dtab", dtab, ref["dtab"], e["dtab"])
        if shift == 0:
            ck.exact(prefix + "dtab: a plane of another window type is not zero at shift 0", not bool(dtab[1:].any()))
        ck.exact(prefix + "dtab: pad-slot rows / columns are not zero", not bool(dtab[:, :, 49:].any()) and not bool(dtab[..., 49:].any()))
        if padded:
            ck.close(prefix + "dbias[C:]", dbias[C:], ref["dbias"][C:], S.err(chain["dbias"][C:], ref["dbias"][C:]))
            ck.exact(prefix + "dbias[0..C) is not zero", not bool(dbias[:C].any()))
    return got, ref, chain


@pytest.mark.parametrize("dt", S.DTS, ids=dn)
@pytest.mark.parametrize("c", S.WATTN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_window_attention_whole_windows(ops, c, dt):
    ck = Checks(f"swin_window_attn[{'x'.join(map(str, c))},{dn(dt)}]")
    run_wattn(ops, ck, "", c, dt)
    ck.done()


@pytest.mark.parametrize("dt", S.DTS, ids=dn)
def test_window_attention_live_word(ops, dt):
    """1 of 3 images in use: the others are NaN on the way in and keep the sentinel"""
    ck = Checks(f"swin_window_attn.live[3x14x14x3x3,{dn(dt)}]")
    run_wattn(ops, ck, "", (3, 14, 14, 3, 3), dt, n_live=1, want_bwd=False)
    ck.done()


@pytest.mark.parametrize("dt", S.DTS, ids=dn)
@pytest.mark.parametrize("c", S.WATTN_PAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_window_attention_padded_maps(ops, c, dt):
    """o, dqkv, dtab (the pad keys' columns included; a pad query's row exactly zero), dbias[C..3C) and an untouched dbias[0..C)"""
    n, H, W, heads, shift = c
    ck = Checks(f"swin_window_attn_pad[{'x'.join(map(str, c))},{dn(dt)}]")
    got, ref, _ = run_wattn(ops, ck, "", c, dt)
    # rows of pad queries: where EVERY window of a type has a pad token at slot q, row q of that plane is exactly zero
    pix, types = S.window_geometry(H, W, shift)[0], S.window_types(H, W, shift)
    for t in range(4):
        sel = types == t
        if bool(sel.any()):
            rows = (pix[sel] < 0).all(0)
            ck.exact(f"dtab[{t}]: a pad query's row is not zero", not bool(got["dtab"][t][:, :49][:, rows.to(DEV)].any()))
            ck.exact(f"model dtab[{t}]: a pad query's row is not zero", not bool(ref["dtab"][t][:, :49][:, rows].any()))
    ck.done()


@pytest.mark.parametrize("dt", S.DTS, ids=dn)
def test_padded_backward_entry_leaves_dbias_alone_on_whole_windows(ops, dt):
    """mtmp_swin_window_attn_pad_bwd on a 14 x 14 map runs the whole-window kernel: dbias comes back as it went in"""
    from medical_tri_modal_pilot_amd import _lib
    n, H, W, heads, shift = 1, 14, 14, 3, 3
    C = heads * S.DH
    p = S.attn_inputs(n, H, W, heads, dt, pad=True)
    qkv, d_out, bias = put(p["qkv"], dt), put(p["d_out"], dt), put(p["bias"])
    tab = put(S.table_model(p["rpb"], heads, shift, dt), dt)
    dqkv, dtab = torch.empty_like(qkv), torch.zeros(4, heads, 64, 64, device=DEV)
    dbias = torch.full((3 * C,), SENTINEL, device=DEV)
    _lib.call("mtmp_swin_window_attn_pad_bwd", ops._dt(qkv), ops._p(qkv), ops._p(bias), ops._p(tab), ops._p(d_out), ops._p(dqkv),
              ops._p(dtab), ops._p(dbias), n, H, W, C, heads, shift, float(S.DH ** -0.5), ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(dbias, torch.full_like(dbias, SENTINEL))
    dq0, dt0 = ops.swin_window_attn_bwd(qkv, tab, d_out, heads, shift)
    assert torch.equal(dqkv, dq0) and torch.equal(dtab, dt0)                   # (one window per plane: the atomics have no order)


@pytest.mark.parametrize("dt", S.DTS, ids=dn)
def test_probe_last_window_row_and_column(ops, dt):
    """14 x 21 at shift 3: v and d_out are zero outside the corner window and its two neighbours, so o, dqkv and dtab are those
    windows' alone; each window's tokens also as a tensor of their own"""
    c = S.CORNER_PROBE
    case = (c["n"], c["H"], c["W"], c["heads"], c["shift"])
    ck = Checks(f"probe.wattn_corner[{dn(dt)}]")
    p = S.corner_probe_inputs(dt)
    got, ref, chain = run_wattn(ops, ck, "", case, dt, p=p)
    for w, name in S.corner_probe_windows():
        tok = S.window_tokens(c["H"], c["W"], c["shift"], w)
        for k in ("o", "dqkv"):
            ck.close(f"{k}[{name}]", got[k][:, tok.to(DEV)], ref[k][:, tok], S.err(chain[k][:, tok], ref[k][:, tok]), dt == BF16)
    for t in (1, 2, 3):
        ck.close(f"dtab[{t}]", got["dtab"][t], ref["dtab"][t], S.err(chain["dtab"][t], ref["dtab"][t]))
    assert all(REPORT[f"{ck.tag}.{k}"]["bound"] <= S.PROBE_BOUND for k in ("o", "dqkv", "dtab"))
    ck.done()


@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("dt", S.DTS, ids=dn)
def test_probe_pad_keys(ops, dt, shift):
    """8 x 8: v is zero on every real token, so o is what the pad tokens add as keys; dbias is the pad tokens' gradient alone"""
    c = S.PAD_PROBE
    ck = Checks(f"probe.wattn_pad_keys[shift={shift},{dn(dt)}]")
    run_wattn(ops, ck, "", (c["n"], c["H"], c["W"], c["heads"], shift), dt, p=S.pad_probe_inputs(dt, shift))
    assert REPORT[f"{ck.tag}.o"]["bound"] <= S.PROBE_BOUND and REPORT[f"{ck.tag}.dbias[C:]"]["bound"] <= S.PROBE_BOUND
    ck.done()


# ------------------------------------------------------------------------------------------ 5. swin_mlp, swin_ln_linear
def mlp_args(p, dev=False):
    f = (lambda t, dt=F32: put(t, dt)) if dev else (lambda t, dt=F32: t)
    return [f(p["x"], BF16), f(p["ln_w"]), f(p["ln_b"]), 1e-5, f(p["w1"], BF16), f(p["b1"]), f(p["w2"], BF16), f(p["b2"])]


def run_mlp(ops, ck, prefix, M, C, scaled, live=None, p=None):
    p = p or S.mlp_inputs(M, C)
    L = M if live is None else live
    rs = S.row_scales(M, 49) if scaled else None
    q = dict(p, x=p["x"][:L])
    ref, e = e_of(S.swin_mlp_model, *mlp_args(q), rs, 49, dt=BF16)
    a = mlp_args(p, dev=True)
    poison(a[0], L)
    with sentinel_outputs(), ops.rows_live(None if live is None else word(live), 0):
        y = ops.swin_mlp(*a, put(rs), 49)
    if live is not None:
        untouched(ck, prefix + "y", y, L)
    ck.close(prefix + "y", y[:L], ref["y"], e["y"], True)
    if scaled and L > 49:                                       # rows 49 .. 97 carry the factor 0: y = x there, bit for bit
        ck.exact(prefix + "y != x under a factor 0", torch.equal(y[49:min(L, 98)], a[0][49:min(L, 98)]))
    return y, ref, e


@pytest.mark.parametrize("scaled", [False, True], ids=["noscale", "scale49"])
@pytest.mark.parametrize("C", [96, 192])
def test_swin_mlp_at_every_row_edge(ops, C, scaled):
    ck = Checks(f"swin_mlp[C={C},{'scale49' if scaled else 'noscale'}]")
    for M in S.M_EDGES:
        run_mlp(ops, ck, f"M={M}.", M, C, scaled)
    ck.done()


@pytest.mark.parametrize("C", [96, 192])
def test_swin_mlp_live_word(ops, C):
    """inside a wave (40), at a wave edge (64), at a workgroup edge (128)"""
    ck = Checks(f"swin_mlp.live[C={C}]")
    for live in (40, 64, 128):
        run_mlp(ops, ck, f"live={live}.", 257, C, True, live=live)
    ck.done()


@pytest.mark.parametrize("C", [96, 192])
def test_probe_last_hidden_panel_of_swin_mlp(ops, C):
    """w2 is zero outside the last panel's columns: the branch is that panel's term"""
    ck = Checks(f"probe.mlp_last_panel[C={C}]")
    run_mlp(ops, ck, "", S.MLP_PROBE_M, C, False, p=S.mlp_probe_inputs(C))
    assert REPORT[f"{ck.tag}.y"]["bound"] <= S.PROBE_BOUND
    ck.done()


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("N", [32, 288, 576])
@pytest.mark.parametrize("C", [96, 192])
def test_swin_ln_linear_at_every_row_edge(ops, C, N, bias):
    ck = Checks(f"swin_ln_linear[C={C},N={N},{'bias' if bias else 'nobias'}]")
    for M in S.M_EDGES:
        p = S.ln_linear_inputs(M, C, N, bias=bias)
        ref, e = e_of(S.ln_linear_model, p["x"], p["ln_w"], p["ln_b"], 1e-5, p["w"], p["bias"], dt=BF16)
        with sentinel_outputs():
            y = ops.swin_ln_linear(put(p["x"], BF16), put(p["ln_w"]), put(p["ln_b"]), 1e-5, put(p["w"], BF16), put(p["bias"]))
        ck.close(f"M={M}.y", y, ref["y"], e["y"], True)
    if bias:                                                    # a live word that retires the workgroup's last two waves and a workgroup
        M, live = 257, 64
        p = S.ln_linear_inputs(M, C, N)
        ref, e = e_of(S.ln_linear_model, p["x"][:live], p["ln_w"], p["ln_b"], 1e-5, p["w"], p["bias"], dt=BF16)
        x = poison(put(p["x"], BF16), live)
        with sentinel_outputs(), ops.rows_live(word(live), 0):
            y = ops.swin_ln_linear(x, put(p["ln_w"]), put(p["ln_b"]), 1e-5, put(p["w"], BF16), put(p["bias"]))
        untouched(ck, "live.y", y, live)
        ck.close("live=64.y", y[:live], ref["y"], e["y"], True)
    ck.done()


# ------------------------------------------------------------------------------------------ 6. swin_attn_block(_pad)
def run_block(ops, ck, prefix, C, case, scaled, n_live=None):
    n, H, W, shift = case
    heads = C // S.DH
    padded = H % 7 != 0 or W % 7 != 0
    p = S.block_inputs(n, H, W, C)
    rs = S.row_scales(n, 1) if scaled else None
    L = n if n_live is None else n_live
    ref, e = e_of(S.attn_block_model, p["x"][:L], p["ln_w"], p["ln_b"], 1e-5, p["wqkv"], p["bqkv"], p["rpb"], heads, shift,
                  p["wproj"], p["bproj"], None if rs is None else rs[:L], dt=BF16)
    x = poison(put(p["x"], BF16), L)
    tab = put(S.table_model(p["rpb"], heads, shift, BF16, acc_order=True), BF16)
    entry = ops.swin_attn_block_pad if padded else ops.swin_attn_block
    with sentinel_outputs(), ops.rows_live(None if n_live is None else word(L * H * W), 0):
        y = entry(x, put(p["ln_w"]), put(p["ln_b"]), 1e-5, put(p["wqkv"], BF16), put(p["bqkv"]), tab, heads, shift,
                  put(p["wproj"], BF16), put(p["bproj"]), put(rs))
    if n_live is not None:
        untouched(ck, prefix + "y", y, L)
    ck.close(prefix + "y", y[:L], ref["y"], e["y"], True)
    if scaled and L > 1:
        ck.exact(prefix + "the image with factor 0 is not x", torch.equal(y[1], x[1]))


@pytest.mark.parametrize("scaled", [False, True], ids=["noscale", "scaled"])
@pytest.mark.parametrize("case", S.BLOCK_CASES + S.BLOCK_PAD_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("C", [96, 192])
def test_swin_attn_block(ops, C, case, scaled):
    ck = Checks(f"swin_attn_block[C={C},{'x'.join(map(str, case))},{'scaled' if scaled else 'noscale'}]")
    run_block(ops, ck, "", C, case, scaled)
    ck.done()


@pytest.mark.parametrize("case", [(3, 14, 14, 3), (3, 8, 8, 3)], ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("C", [96, 192])
def test_swin_attn_block_live_word(ops, C, case):
    ck = Checks(f"swin_attn_block.live[C={C},{'x'.join(map(str, case))}]")
    run_block(ops, ck, "", C, case, True, n_live=2)
    ck.done()


# ------------------------------------------------------------------------------------------ 7. stem
@pytest.mark.parametrize("dt", S.DTS, ids=dn)
@pytest.mark.parametrize("n,H,W", S.STEM_CASES)
def test_swin_stem(ops, n, H, W, dt):
    """patch counts on both sides of a wave's 32 and a workgroup's 128; `order` as a permutation; a live word inside an image's
    patches and at an image edge"""
    ck = Checks(f"swin_stem[{n}x{H}x{W},{dn(dt)}]")
    p = S.stem_inputs(n, H, W)
    names = ("img", "w", "bias", "ln_w", "ln_b")
    dev = [put(p[k]) for k in names]
    ref, e = e_of(S.stem_model, *[p[k] for k in names], dt=dt)
    with sentinel_outputs():
        y = ops.swin_stem(*dev, dt)
    ck.close("y", y, ref["y"], e["y"], dt == BF16)
    if n > 1:
        order = torch.tensor([(i + 1) % n for i in range(n)], dtype=torch.int32)
        ref, e = e_of(S.stem_model, *[p[k] for k in names], order, dt=dt)
        per = (H // 4) * (W // 4)
        for live in (n * per, per + per // 4, per):
            with sentinel_outputs(), ops.rows_live(None if live == n * per else word(live), 0):
                y = ops.swin_stem(*dev, dt, order=order.to(DEV))
            yf, rf = y.view(n * per, 96), ref["y"].view(n * per, 96)
            untouched(ck, f"order.live={live}.y", yf, live)
            chain = S.stem_model(*[p[k] for k in names], order, dt=dt, ft=F32)["y"].view(n * per, 96)
            ck.close(f"order.live={live}.y", yf[:live], rf[:live], S.err(chain[:live], rf[:live]), dt == BF16)
    ck.done()
