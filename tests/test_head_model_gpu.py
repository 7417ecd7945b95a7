"""-m gpu: the BatchNorm classification head (csrc/head.hip: ops.HeadFn, mtmp_head_fwd / mtmp_head_bwd, the FlatParams sink of
mtmp_head_bwd_scatter) and the mean-reduced BCE (mtmp_bce_logits_mean) against the float64 model of tests/head_model.py, element by
element, at every batch size where the one-, two- and four-rows-per-lane kernels change form or have a ragged last lane group.
Metric and bound: head_model.py -- every bound here is max(8 e_torch, 16 * 2^-24) (+ 2^-8 for a bf16 output) with e_torch the error
of the same chain in fp32 on the CPU, bit equality, or exact zero; the three gradients that cancel in training mode (db1, dln_b,
ddemo_be) are held to the absolute sum of their summands.  Every case asserts its ReLU gate margin from the float64 reference
before it compares, and no element is left out.  BatchNorm eps 1e-3, momentum 0.25, LayerNorm eps 1e-5: no two constants equal.
Every check appends {err, e_torch, bound} to a report: build/head_report.json, or the file MTMP_HEAD_REPORT names (and, next to it
as .txt, the worst err / bound per tensor, mode and CLS type: the text of profiles/head_parity.txt).
Every launch is at most 256 rows: a case takes milliseconds.  The first case of the file also loads the library and starts HIP.
"""
import json
import math
import os
import re

import pytest
import torch
import torch.nn as nn

from tests import head_model as H
from tests import row_kernels_model as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32, F64, BF16 = H.F32, H.F64, H.BF16
DT = [F32, BF16]
MODES = [True, False]
REPORT = {}
mode_name = lambda tr: "train" if tr else "eval"


@pytest.fixture(scope="module")
def ops():
    from medical_tri_modal_pilot_amd import ops as _ops
    return _ops


def summary(report):
    """worst err / bound per (check family, mode, CLS type, tensor), and the case it comes from"""
    worst = {}
    for key, v in report.items():
        m = re.fullmatch(r"(\w+)\[(.*?)\]\.(\w+)", key)
        fam, args, name = m.group(1), m.group(2).split(","), m.group(3)
        g = (fam, ",".join(args[1:]), name)
        ratio = v["err"] / v["bound"]
        if g not in worst or ratio > worst[g][0]:
            worst[g] = (ratio, args[0], v)
    lines = ["family            mode,type    tensor      worst err/bound  at      err        e_torch    bound"]
    for (fam, rest, name), (ratio, at, v) in sorted(worst.items()):
        lines.append(f"{fam:17s} {rest:12s} {name:11s} {ratio:15.3f}  {at:7s} {v['err']:.3e}  {v['e_torch']:.3e}  {v['bound']:.3e}")
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module", autouse=True)
def _dump_report():
    yield
    path = os.environ.get("MTMP_HEAD_REPORT") or os.path.join(ROOT, "build", "head_report.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)
    with open(os.path.splitext(path)[0] + ".txt", "w") as f:
        f.write(summary(REPORT))


class Checks:
    """collects the checks of one test: every figure is printed and recorded before the test asserts"""

    def __init__(self, tag):
        self.tag, self.failed = tag, []

    def head(self, name, got, c, training, bf16_out=False):
        self.record(name, H.err_of(name, got, c["ref"], training), c["e_torch"][name], R.bound(c["e_torch"][name], bf16_out))

    def close(self, name, got, ref, e_torch):
        self.record(name, R.err(got, ref), e_torch, R.bound(e_torch))

    def record(self, name, e, e_torch, b):
        key = f"{self.tag}.{name}"
        assert key not in REPORT, key
        REPORT[key] = {"err": e, "e_torch": e_torch, "bound": b}
        print(f"{key}: err {e:.3e} e_torch {e_torch:.3e} bound {b:.3e} ratio {e / b:.3f}")
        if not (math.isfinite(e) and e <= b):
            self.failed.append(f"{key}: err {e:.3e} > bound {b:.3e} (e_torch {e_torch:.3e})")

    def done(self):
        assert not self.failed, "\n".join(self.failed)


def _margin(c):
    m = c["ref"]["margin"]
    assert m > H.GATE_MARGIN, f"a ReLU pre-activation lies {m:.2e} from zero: pick another seed (head_model.find_seeds)"


class Dev:
    """one case on the device: CLS rows in their type (a leaf), parameters as fp32 leaves, the running statistics and the counter"""

    def __init__(self, c, dt, param=False):
        inp = c["inp"]
        self.cls = inp["cls"].to(DEV, dt).requires_grad_()
        self.age, self.gender, self.w = inp["age"].to(DEV), inp["gender"].to(DEV), inp["w"].to(DEV)
        self.prm = [nn.Parameter(p.to(DEV)) if param else p.to(DEV).requires_grad_() for p in inp["params"]]
        self.rm, self.rv = inp["run_mean"].to(DEV), inp["run_var"].to(DEV)
        self.nbt = torch.tensor(41, dtype=torch.int64, device=DEV)

    def run(self, ops, training, cls_view=None, leaf=None):
        """logits and the gradients of sum(o * w) for [the CLS leaf] + the twelve parameters"""
        o = ops.HeadFn.apply(self.cls if cls_view is None else cls_view, self.age, self.gender, training, H.MOMENTUM, H.BN_EPS,
                             self.rm, self.rv, self.nbt if training else None, *self.prm)
        g = torch.autograd.grad((o * self.w).sum(), [self.cls if leaf is None else leaf] + self.prm, allow_unused=True)
        return o.detach(), g[0], list(g[1:])


# ------------------------------------------------------------------------------------------ a. HeadFn against the model
@pytest.mark.parametrize("dt", DT, ids=R.dt_name)
@pytest.mark.parametrize("B,training", [(B, tr) for B in H.BATCHES for tr in H.modes(B)],
                         ids=lambda v: mode_name(v) if isinstance(v, bool) else str(v))
def test_head_against_model(ops, B, training, dt):
    """logits, d cls (in the CLS type), the twelve parameter gradients and the running statistics of one call; B = 1 in eval mode only"""
    c = H.case(B, dt, training)
    _margin(c)
    d = Dev(c, dt)
    o, dcls, grads = d.run(ops, training)
    ck = Checks(f"head[B={B},{mode_name(training)},{R.dt_name(dt)}]")
    assert o.shape == (B, 1) and o.dtype == F32
    ck.head("o", o, c, training)
    assert dcls.dtype == dt and dcls.shape == (B, 256)
    ck.head("dcls", dcls, c, training, dt == BF16)
    for name, g, p in zip(H.GRAD_NAMES, grads, d.prm):
        assert g.shape == p.shape and g.dtype == F32, name
        ck.head(name, g, c, training)
    if training:
        assert int(d.nbt) == 42                                           # BatchNorm1d.num_batches_tracked, counted by the first launch
        ck.head("run_mean", d.rm, c, training)
        ck.head("run_var", d.rv, c, training)
    else:
        assert int(d.nbt) == 41
        assert torch.equal(d.rm.cpu(), c["inp"]["run_mean"]) and torch.equal(d.rv.cpu(), c["inp"]["run_var"])
    ck.done()


# ------------------------------------------------------------------------------------------ b. strided CLS rows
@pytest.mark.parametrize("dt", DT, ids=R.dt_name)
@pytest.mark.parametrize("training", MODES, ids=mode_name)
@pytest.mark.parametrize("B", [5, 129])
def test_strided_cls_rows(ops, B, training, dt):
    """CLS as the view [:, 0, :] of a [B, 7, 256] tensor: the bits of the contiguous call, and exactly 0 for the other six rows"""
    c = H.case(B, dt, training)
    d0, d1 = Dev(c, dt), Dev(c, dt)
    o0, dcls0, g0 = d0.run(ops, training)
    full = torch.randn(B, 7, 256, generator=torch.Generator().manual_seed(5)).to(DEV, dt)
    full[:, 0, :] = d1.cls.detach()
    full.requires_grad_()
    o1, dfull, g1 = d1.run(ops, training, cls_view=full[:, 0, :], leaf=full)
    assert dfull.dtype == dt and dfull.shape == full.shape
    assert torch.equal(o0, o1) and torch.equal(dfull[:, 0, :], dcls0)
    assert float(dfull[:, 1:, :].abs().max()) == 0.0
    assert all(torch.equal(a, b) for a, b in zip(g0, g1))
    assert torch.equal(d0.rm, d1.rm) and torch.equal(d0.rv, d1.rv) and int(d0.nbt) == int(d1.nbt)


# ------------------------------------------------------------------------------------------ c. the FlatParams sink
@pytest.mark.parametrize("dt", DT, ids=R.dt_name)
@pytest.mark.parametrize("training", MODES, ids=mode_name)
@pytest.mark.parametrize("B", [65, 256])
def test_flat_params_sink(ops, B, training, dt):
    """through optim.FlatParams the backward's last launch writes the twelve slices of the flat gradient buffer and autograd sees
    None: the same kernels, another destination, the same bits"""
    from medical_tri_modal_pilot_amd.optim import FlatParams
    c = H.case(B, dt, training)
    d0, d1 = Dev(c, dt), Dev(c, dt, param=True)
    o0, dcls0, g0 = d0.run(ops, training)
    flat = FlatParams(list(zip(H.PARAM_NAMES, d1.prm)))
    flat.zero_grad()
    flat.grad.fill_(float("nan"))                                         # (every element of every slice must be OVERWRITTEN)
    o1, dcls1, g1 = d1.run(ops, training)
    assert all(g is None for g in g1) and flat.written == set(range(12))
    assert torch.equal(o0, o1) and torch.equal(dcls0, dcls1)
    for name, p, g in zip(H.PARAM_NAMES, d1.prm, g0):
        assert p.grad.shape == g.shape and torch.equal(p.grad, g), name
        assert p.grad.data_ptr() == flat.grad.data_ptr() + 4 * flat.offsets[flat.index_of[id(p)]], name


# ------------------------------------------------------------------------------------------ d. the float-only entries
G_ROWS = ["dln_g", "dln_b", "ddemo_g", "ddemo_be", "ddemo_w0", "ddemo_w1", "ddemo_b"]


@pytest.mark.parametrize("training", MODES, ids=mode_name)
@pytest.mark.parametrize("B", [63, 127, 255])
def test_float_entries(ops, B, training):
    """mtmp_head_fwd / mtmp_head_bwd on the fp32 case: HeadFn's kernels, so HeadFn's bits, but for g_rows[7][256], whose slab is
    reduced in another fixed order -- that one is held to the model at the bound."""
    from medical_tri_modal_pilot_amd import _lib
    c = H.case(B, F32, training)
    _margin(c)
    d = Dev(c, F32)
    o, dcls, grads = d.run(ops, training)
    g = dict(zip(H.GRAD_NAMES, grads))
    f32 = dict(dtype=F32, device=DEV)
    inp = c["inp"]
    P = [p.to(DEV) for p in inp["params"]]
    rm, rv = inp["run_mean"].to(DEV), inp["run_var"].to(DEV)
    table = ops._ptrs(P[:10] + [rm, rv] + P[10:])
    cls, do = inp["cls"].to(DEV), inp["w"].to(DEV).view(-1).contiguous()
    out, ws = torch.empty(B, **f32), torch.empty(_lib.lib().mtmp_head_ws_floats(B), **f32)
    _lib.call("mtmp_head_fwd", cls.data_ptr(), d.age.data_ptr(), d.gender.data_ptr(), table, out.data_ptr(), ws.data_ptr(), B,
              H.LN_EPS, H.BN_EPS, H.MOMENTUM, int(training), ops._stream())
    nan = lambda *sh: torch.full(sh, float("nan"), **f32)
    dcls1, g_rows, dw1, g_feat, db2 = nan(B, 256), nan(7, 256), nan(256, 512), nan(4, 256), nan(1)
    wsb = torch.empty(B * 256 * 8, **f32)
    _lib.call("mtmp_head_bwd", do.data_ptr(), cls.data_ptr(), d.age.data_ptr(), d.gender.data_ptr(), table, ws.data_ptr(),
              dcls1.data_ptr(), g_rows.data_ptr(), dw1.data_ptr(), g_feat.data_ptr(), db2.data_ptr(), wsb.data_ptr(), B, H.LN_EPS,
              int(training), ops._stream())
    for name, a, b in (("o", out, o.view(-1)), ("dcls", dcls1, dcls), ("dw1", dw1, g["dw1"]), ("db1", g_feat[0], g["db1"]),
                       ("dbn_g", g_feat[1], g["dbn_g"]), ("dbn_b", g_feat[2], g["dbn_b"]), ("dw2", g_feat[3], g["dw2"].view(-1)),
                       ("db2", db2, g["db2"]), ("run_mean", rm, d.rm), ("run_var", rv, d.rv)):
        assert torch.equal(a, b), name
    ck = Checks(f"float_entries[B={B},{mode_name(training)},fp32]")
    rows = dict(zip(G_ROWS, g_rows))
    rows["ddemo_w"] = torch.stack([rows.pop("ddemo_w0"), rows.pop("ddemo_w1")], 1)
    for name, got in rows.items():
        ck.head(name, got, c, training)
    ck.done()


# ------------------------------------------------------------------------------------------ e. determinism, graph replay
def _chain(ops, cls, age, gender, y, prm, rm, rv, nbt):
    """head (training mode) -> BCE -> backward with the unit gradient"""
    o = ops.HeadFn.apply(cls, age, gender, True, H.MOMENTUM, H.BN_EPS, rm, rv, nbt, *prm)
    loss = ops.bce_with_logits(nn.BCEWithLogitsLoss(), o, y)
    assert type(loss.grad_fn).__name__.startswith("BceLogitsMean")
    g = torch.autograd.grad(loss, [cls] + prm, ops.unit_grad(loss))
    return [o.detach(), loss.detach()] + list(g)


def _chain_inputs(c, dt):
    inp = c["inp"]
    return inp["cls"].to(DEV, dt).requires_grad_(), inp["age"].to(DEV), inp["gender"].to(DEV), (inp["w"] > 0).float().to(DEV)


def _state(c):
    return c["inp"]["run_mean"].to(DEV), c["inp"]["run_var"].to(DEV), torch.tensor(41, dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("dt", DT, ids=R.dt_name)
def test_two_runs_are_bit_identical(ops, dt):
    c = H.case(65, dt, True)
    prm = [p.to(DEV).requires_grad_() for p in c["inp"]["params"]]
    runs = []
    for _ in range(2):
        st = _state(c)
        runs.append(_chain(ops, *_chain_inputs(c, dt), prm, *st) + [st[0], st[1]])
    assert all(torch.equal(s, t) for s, t in zip(*runs))


def test_chain_replays_from_a_captured_graph(ops):
    """head -> BCE -> backward recorded with torch.cuda.graph on static buffers (one stream: one chain of launches, nothing forks)
    and replayed three times with other inputs copied in: each replay bit-equal to the eager chain on those inputs, the batch
    counter -- incremented inside the head's first kernel -- advanced by exactly one per replay, and the running statistics those
    of three eager steps."""
    B, dt = 65, BF16
    cases = [H.case(B, dt, True)] + [H.case(B, dt, True, seed=H.SEEDS[B] + 1000 + k) for k in range(3)]
    prm = [p.to(DEV).requires_grad_() for p in cases[0]["inp"]["params"]]
    cls, age, gender, y = _chain_inputs(cases[0], dt)
    rm, rv, nbt = _state(cases[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _chain(ops, cls, age, gender, y, prm, rm, rv, nbt)                 # warm-up: unit_grad and the allocator's pool
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = _chain(ops, cls, age, gender, y, prm, rm, rv, nbt)
    rm0, rv0, nbt0 = _state(cases[0])
    rm.copy_(rm0), rv.copy_(rv0), nbt.copy_(nbt0)                          # (the warm-up stepped them; the capture itself ran nothing)
    rm_e, rv_e, nbt_e = _state(cases[0])
    for k, c in enumerate(cases[1:]):
        c2, a2, g2, y2 = _chain_inputs(c, dt)
        with torch.no_grad():
            cls.copy_(c2), age.copy_(a2), gender.copy_(g2), y.copy_(y2)
        graph.replay()
        eager = _chain(ops, c2, a2, g2, y2, prm, rm_e, rv_e, nbt_e)
        torch.cuda.synchronize()
        assert int(nbt) == 42 + k and int(nbt_e) == 42 + k
        for s, e in zip(static_out, eager):
            assert torch.equal(s, e)
        assert torch.equal(rm, rm_e) and torch.equal(rv, rv_e)
    assert not torch.equal(rm, rm0) and not torch.equal(rv, rv0)


# ------------------------------------------------------------------------------------------ f. BCE with logits, mean-reduced
def _bce(ops, c):
    od, td = c["o"].to(DEV).requires_grad_(), c["t"].to(DEV)
    loss = ops.bce_with_logits(nn.BCEWithLogitsLoss(), od, td)
    assert loss.shape == () and type(loss.grad_fn).__name__.startswith("BceLogitsMean")
    return od, loss


@pytest.mark.parametrize("n", H.BCE_N)
def test_bce_against_model(ops, n):
    """logits 2 randn: the loss and every dlogit at the bound.  An incoming gradient of 3.0 takes the multiplying branch of
    _saved_grad_once, and a second backward over a retained graph gets a copy, not the saved tensor."""
    c = H.bce_case(n)
    od, loss = _bce(ops, c)
    (d1,) = torch.autograd.grad(loss, od, ops.unit_grad(loss), retain_graph=True)
    (d2,) = torch.autograd.grad(loss, od, ops.unit_grad(loss), retain_graph=True)
    (d3,) = torch.autograd.grad(loss * 3.0, od)
    ck = Checks(f"bce[n={n},randn]")
    ck.close("loss", loss.detach().reshape(1), c["ref"]["loss"], c["e_torch"]["loss"])
    ck.close("dlogit", d1, c["ref"]["dlogit"], c["e_torch"]["dlogit"])
    assert d1.shape == od.shape and d1.dtype == F32
    assert torch.equal(d1, d2) and d1.data_ptr() != d2.data_ptr()
    assert torch.equal(d3, d1 * 3.0) and d3.data_ptr() != d1.data_ptr()
    ck.done()


@pytest.mark.parametrize("n", H.BCE_N)
def test_bce_where_exp_overflows_and_sigmoid_saturates(ops, n):
    """logits +-20, +-88, +-89, +-104 and 0, each with target 0 and with target 1, among 2 randn: everything finite, dlogit inside
    [-1/n, 1/n] (the interval's ends as fp32 holds them), and its sign that of sigmoid(o) - t.
    fp32 cannot hold every such difference.  sigmoid(o) - t is a difference of two fp32 numbers: below one ulp of the larger of
    the two (2^-23 max(sigmoid(o), t): o = 20 and up with target 1) it may round to 0, and so may a quotient below the smallest
    normal fp32 number, 2^-126 (o = -88 and down with target 0).  There a zero is accepted as well; the opposite sign never is.
    Everywhere else the sign must be the reference's.  Which elements are which is decided from the float64 reference alone."""
    c = H.bce_case(n, planted=True)
    od, loss = _bce(ops, c)
    (d,) = torch.autograd.grad(loss, od, ops.unit_grad(loss))
    ref = c["ref"]["dlogit"]
    got = d.detach().cpu().double()
    assert math.isfinite(float(loss.detach())) and bool(torch.isfinite(got).all())
    assert float(got.abs().max()) <= float(torch.tensor(1.0 / n, dtype=F32))
    sig, t = torch.sigmoid(c["o"].double()), c["t"].double()
    strict = ((ref * n).abs() >= 2.0 ** -23 * torch.maximum(sig, t)) & (ref.abs() >= 2.0 ** -126)
    assert bool((torch.sign(ref) != 0).all())
    assert bool((torch.sign(got) == torch.sign(ref))[strict].all())
    assert bool((got * torch.sign(ref) >= 0)[~strict].all())
    if n >= 2 * len(H.BCE_PLANTED):                # +-20, +-88 and 0 with the target they do not saturate against, and both kinds there
        assert int(strict[:18].sum()) >= 9 and int((~strict[:18]).sum()) >= 6
    ck = Checks(f"bce[n={n},planted]")
    ck.close("loss", loss.detach().reshape(1), c["ref"]["loss"], c["e_torch"]["loss"])
    ck.done()
