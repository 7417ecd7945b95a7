"""-m gpu: the kernels of ``--vslt-type QIE`` -- ops.QieAddsFn (csrc/qie.hip), ops.QieHeadFn (csrc/head.hip, width 256) and the vital-sign add
of the stream-input node (ops.StreamInputsQieFn) -- against the float64 models of tests/qie_model.py, element by element.
Metric and bound: qie_model.py -- every bound is max(8 e_torch, 16 * 2^-24) (+ 2^-8 for a bf16 output) with e_torch the error of the same
chain in fp32 on the CPU, bit equality, or the absolute-sum rule for the head's two cancelling gradients.  Every case asserts its ReLU
gate margin from the float64 reference before it compares, and no element is left out.

Sizes of the adds.  The backward's grid is B x chunks and a workgroup's work depends on its chunk alone (csrc/qie.hip), so the batch sizes
{1, 2, 63, 64, 65, 256} run at N_v = 9 and the token counts at B = 3; (65, 1000) and (256, 129) cross them once more.  Token counts:
    1, 3, 4    chunk of L <= 4 tokens: waves without a row
    5, 9       the first pair (t, t + 4) / the single row behind a pair
    8, 24      pairs only
    63, 64, 65, 127, 128, 129   the 64-token chunk: ragged last chunk, full last chunk, a chunk of one token -- one and two chunks deep
    1000       15 full chunks and one of 40
and, packed, kv_len in {1, N_v} (and one in between) mixed in one batch: empty chunks beside full ones.  N_i = 49, N_t = 128 throughout.
Every figure is printed before its test asserts and collected in build/qie_report.json (or the file MTMP_QIE_REPORT names), with the
worst err / bound per tensor next to it as .txt: the text of profiles/qie_parity.txt."""
import ctypes
import json
import math
import os

import pytest
import torch
import torch.nn as nn

from tests import head_model as H
from tests import qie_model as Q
from tests import row_kernels_model as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
DT = [F32, BF16]
REPORT = {}
KEPT_ALIVE = []                          # captured graphs and what they point to are never released (graph.py)
NB = 4                                   # bottleneck rows in front of the CLS row: kv_off = NB + 1
mode_name = lambda tr: "train" if tr else "eval"
ADD_SIZES = ([(B, 9) for B in Q.ADD_BATCHES] + [(3, n) for n in (1, 3, 4, 5, 8, 9, 24, 63, 64, 65, 127, 128, 129, 1000)]
             + [(65, 1000), (256, 129)])


@pytest.fixture(scope="module")
def ops():
    from medical_tri_modal_pilot_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module", autouse=True)
def _dump_report():
    yield
    path = os.environ.get("MTMP_QIE_REPORT") or os.path.join(ROOT, "build", "qie_report.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)
    worst = {}
    for key, v in REPORT.items():
        fam, name = key.split("[")[0], key.rsplit(".", 1)[1]
        if (fam, name) not in worst or v["err"] / v["bound"] > worst[(fam, name)][0]:
            worst[(fam, name)] = (v["err"] / v["bound"], key, v)
    with open(os.path.splitext(path)[0] + ".txt", "w") as f:
        f.write("family      tensor     worst err/bound  err        e_torch    bound      at\n")
        for (fam, name), (ratio, key, v) in sorted(worst.items()):
            f.write(f"{fam:11s} {name:10s} {ratio:15.3f}  {v['err']:.3e}  {v['e_torch']:.3e}  {v['bound']:.3e}  {key}\n")


class Checks:
    """collects the checks of one test: every figure is printed and recorded before the test asserts"""

    def __init__(self, tag):
        self.tag, self.failed = tag, []

    def record(self, name, e, e_torch, b):
        key = f"{self.tag}.{name}"
        assert key not in REPORT, key
        REPORT[key] = {"err": e, "e_torch": e_torch, "bound": b}
        print(f"{key}: err {e:.3e} e_torch {e_torch:.3e} bound {b:.3e} ratio {e / b:.3f}")
        if not (math.isfinite(e) and e <= b):
            self.failed.append(f"{key}: err {e:.3e} > bound {b:.3e} (e_torch {e_torch:.3e})")

    def close(self, name, got, c, bf16_out=False):
        ref = c["ref"][name]
        self.record(name, R.err(got.reshape(ref.shape), ref), c["e_torch"][name], R.bound(c["e_torch"][name], bf16_out))

    def head(self, name, got, c, training, bf16_out=False):
        self.record(name, Q.qhead_err(name, got, c["ref"], training), c["e_torch"][name], R.bound(c["e_torch"][name], bf16_out))

    def done(self):
        assert not self.failed, "\n".join(self.failed)


def _margin(c):
    m = c["ref"]["margin"]
    assert m > Q.GATE_MARGIN, f"a ReLU pre-activation lies {m:.2e} from zero: pick another seed (qie_model.find_seeds)"


# ------------------------------------------------------------------------------------------ a. QieAddsFn against the model
def run_adds(ops, c, dt, kv_live=None, param=False):
    """(adds, d_it, d_tt, the four parameters) of one case: the forward, then the backward on the case's three input gradients,
    left in the hand-off dict as ops.StreamInputsQieFn leaves them"""
    inp = c["inp"]
    dev = lambda t: None if t is None else t.to(DEV, dt)
    prm = [nn.Parameter(p.to(DEV)) if param else p.to(DEV).requires_grad_() for p in inp["params"]]
    it, tt = dev(inp["it"]), dev(inp["tt"])
    if it is not None:
        it.requires_grad_(), tt.requires_grad_()
    handoff = {}
    adds = ops.QieAddsFn.apply(inp["age"].to(DEV), inp["gender"].to(DEV), it, tt, dt, handoff, *prm)
    kv = None if kv_live is None else (torch.tensor(kv_live, dtype=torch.int32) + NB + 1).to(DEV)
    handoff.update(dxs=(dev(inp["dx_v"]), dev(inp["dx_i"]), dev(inp["dx_t"])), kv_len=kv, kv_off=NB + 1)
    torch.autograd.backward([adds[0]], [torch.empty_like(adds[0])])
    assert "dxs" not in handoff
    return adds, (None if it is None else it.grad), (None if tt is None else tt.grad), prm


def check_adds(ck, c, dt, adds, d_it, d_tt, prm):
    with_time = c["inp"]["it"] is not None
    for name, t in zip(("add_v", "add_i", "add_t"), adds):
        if name == "add_v" or with_time:
            assert t.dtype == dt and t.shape == c["ref"][name].shape
            ck.close(name, t, c, dt == BF16)
        else:
            assert t is None
    if with_time:
        assert d_it.dtype == dt and d_tt.dtype == dt
        ck.close("d_it", d_it, c, dt == BF16)
        ck.close("d_tt", d_tt, c, dt == BF16)
    for name, p in zip(Q.ADD_GRADS, prm):
        assert p.grad.shape == p.shape and p.grad.dtype == F32, name
        ck.close(name, p.grad, c)


@pytest.mark.parametrize("with_time", [True, False], ids=["time", "notime"])
@pytest.mark.parametrize("dt", DT, ids=R.dt_name)
@pytest.mark.parametrize("B,N_v", ADD_SIZES)
def test_adds_against_model(ops, B, N_v, dt, with_time):
    """the three add rows (in the streams' type), d it, d tt (in the streams' type) and the four ie_demo gradients (fp32)"""
    c = Q.adds_case(B, N_v, dt, with_time)
    _margin(c)
    ck = Checks(f"adds[B={B},N_v={N_v},{R.dt_name(dt)},{'time' if with_time else 'notime'}]")
    check_adds(ck, c, dt, *run_adds(ops, c, dt))
    ck.done()


@pytest.mark.parametrize("dt", DT, ids=R.dt_name)
@pytest.mark.parametrize("N_v", [9, 129])
def test_adds_with_a_packed_vital_sign_stream(ops, N_v, dt):
    """kv_len (bottleneck and CLS rows included) with 1, N_v and something between live tokens in one batch; dx_v's pad rows are zeros,
    as the stream-input backward writes them, so skipping them and reading them must agree: against the model, and bit for bit against
    the same call without kv_len"""
    live = (N_v, 1, max(N_v // 2, 1), 1, N_v)
    c = Q.adds_case(5, N_v, dt, True, live)
    _margin(c)
    ck = Checks(f"adds_packed[B=5,N_v={N_v},{R.dt_name(dt)}]")
    got = run_adds(ops, c, dt, kv_live=live)
    check_adds(ck, c, dt, *got)
    ck.done()
    plain = run_adds(ops, c, dt)
    assert torch.equal(got[1], plain[1]) and torch.equal(got[2], plain[2])
    assert all(torch.equal(a.grad, b.grad) for a, b in zip(got[3], plain[3]))


@pytest.mark.parametrize("dt", DT, ids=R.dt_name)
def test_adds_backward_twice_is_bit_identical_and_d_it_has_token_sums_bits(ops, dt):
    """no float atomics, fixed orders: two launches of the backward return the same bits, whichever workgroup finished last; d it / d tt
    are mtmp_token_sums' own values"""
    c = Q.adds_case(65, 1000, dt)
    runs = [run_adds(ops, c, dt) for _ in range(2)]
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
    assert all(torch.equal(a.grad, b.grad) for a, b in zip(runs[0][3], runs[1][3]))
    dxs = [c["inp"][k].to(DEV, dt) for k in ("dx_i", "dx_t")]
    outs = [torch.empty(65, 256, dtype=dt, device=DEV) for _ in dxs]
    ops.call("mtmp_token_sums", ops._dt(dxs[0]), 2, (ctypes.c_void_p * 2)(*[d.data_ptr() for d in dxs]),
             (ctypes.c_void_p * 2)(*[o.data_ptr() for o in outs]), (ctypes.c_int * 2)(65, 65), (ctypes.c_int * 2)(Q.N_I, Q.N_T), ops._stream())
    assert torch.equal(outs[0], runs[0][1]) and torch.equal(outs[1], runs[0][2])


def test_adds_flat_params_sink(ops):
    """through optim.FlatParams the backward's last launch overwrites the four slices of the flat gradient and autograd sees None"""
    from medical_tri_modal_pilot_amd.optim import FlatParams
    c = Q.adds_case(64, 9, BF16)
    ref = run_adds(ops, c, BF16)
    inp = c["inp"]
    prm = [nn.Parameter(p.to(DEV)) for p in inp["params"]]
    flat = FlatParams(list(zip(["w", "b", "g", "be"], prm)))
    flat.zero_grad()
    flat.grad.fill_(float("nan"))
    handoff = {}
    it, tt = inp["it"].to(DEV, BF16).requires_grad_(), inp["tt"].to(DEV, BF16).requires_grad_()
    adds = ops.QieAddsFn.apply(inp["age"].to(DEV), inp["gender"].to(DEV), it, tt, BF16, handoff, *prm)
    handoff.update(dxs=tuple(inp[k].to(DEV, BF16) for k in ("dx_v", "dx_i", "dx_t")), kv_len=None, kv_off=NB + 1)
    torch.autograd.backward([adds[0]], [torch.empty_like(adds[0])])
    assert flat.written == set(range(4))
    for p, q in zip(prm, ref[3]):
        assert torch.equal(p.grad, q.grad)
    assert torch.equal(it.grad, ref[1]) and torch.equal(tt.grad, ref[2])


# ------------------------------------------------------------------------------------------ b. QieHeadFn against the model
class Dev:
    def __init__(self, c, dt, param=False):
        inp = c["inp"]
        self.cls = inp["cls"].to(DEV, dt).requires_grad_()
        self.w = inp["w"].to(DEV)
        self.prm = [nn.Parameter(p.to(DEV)) if param else p.to(DEV).requires_grad_() for p in inp["params"]]
        self.rm, self.rv = inp["run_mean"].to(DEV), inp["run_var"].to(DEV)
        self.nbt = torch.tensor(41, dtype=torch.int64, device=DEV)

    def run(self, ops, training):
        o = ops.QieHeadFn.apply(self.cls, training, Q.MOMENTUM, Q.BN_EPS, self.rm, self.rv, self.nbt if training else None, *self.prm)
        g = torch.autograd.grad((o * self.w).sum(), [self.cls] + self.prm, allow_unused=True)
        return o.detach(), g[0], list(g[1:])


@pytest.mark.parametrize("dt", DT, ids=R.dt_name)
@pytest.mark.parametrize("B,training", [(B, tr) for B in H.BATCHES for tr in H.modes(B)],
                         ids=lambda v: mode_name(v) if isinstance(v, bool) else str(v))
def test_head_against_model(ops, B, training, dt):
    """logits, d cls (in the CLS type), the eight parameter gradients and the running statistics of one call; B = 1 in eval mode only"""
    c = Q.qhead_case(B, dt, training)
    _margin(c)
    d = Dev(c, dt)
    o, dcls, grads = d.run(ops, training)
    ck = Checks(f"qhead[B={B},{mode_name(training)},{R.dt_name(dt)}]")
    assert o.shape == (B, 1) and o.dtype == F32
    ck.head("o", o, c, training)
    assert dcls.dtype == dt and dcls.shape == (B, 256)
    ck.head("dcls", dcls, c, training, dt == BF16)
    for name, g, p in zip(Q.HEAD_GRADS, grads, d.prm):
        assert g.shape == p.shape and g.dtype == F32, name
        ck.head(name, g, c, training)
    if training:
        assert int(d.nbt) == 42
        ck.head("run_mean", d.rm, c, training)
        ck.head("run_var", d.rv, c, training)
    else:
        assert int(d.nbt) == 41
        assert torch.equal(d.rm.cpu(), c["inp"]["run_mean"]) and torch.equal(d.rv.cpu(), c["inp"]["run_var"])
    ck.done()


@pytest.mark.parametrize("dt", DT, ids=R.dt_name)
@pytest.mark.parametrize("training", [True, False], ids=mode_name)
@pytest.mark.parametrize("B", [65, 256])
def test_head_flat_params_sink(ops, B, training, dt):
    """the eight slices of the flat gradient buffer, every element overwritten: the same kernels, another destination, the same bits"""
    from medical_tri_modal_pilot_amd.optim import FlatParams
    c = Q.qhead_case(B, dt, training)
    d0, d1 = Dev(c, dt), Dev(c, dt, param=True)
    o0, dcls0, g0 = d0.run(ops, training)
    flat = FlatParams(list(zip(Q.HEAD_PARAMS, d1.prm)))
    flat.zero_grad()
    flat.grad.fill_(float("nan"))
    o1, dcls1, g1 = d1.run(ops, training)
    assert all(g is None for g in g1) and flat.written == set(range(8))
    assert torch.equal(o0, o1) and torch.equal(dcls0, dcls1)
    for name, p, g in zip(Q.HEAD_PARAMS, d1.prm, g0):
        assert p.grad.shape == g.shape and torch.equal(p.grad, g), name


def _chain(ops, cls, y, prm, rm, rv, nbt):
    o = ops.QieHeadFn.apply(cls, True, Q.MOMENTUM, Q.BN_EPS, rm, rv, nbt, *prm)
    loss = ops.bce_with_logits(nn.BCEWithLogitsLoss(), o, y)
    g = torch.autograd.grad(loss, [cls] + prm, ops.unit_grad(loss))
    return [o.detach(), loss.detach()] + list(g)


def _state(c):
    return c["inp"]["run_mean"].to(DEV), c["inp"]["run_var"].to(DEV), torch.tensor(41, dtype=torch.int64, device=DEV)


def test_head_chain_replays_from_a_captured_graph(ops):
    """head -> BCE -> backward captured on static buffers and replayed three times with other inputs copied in: each replay bit-equal
    to the eager chain, the batch counter advanced by one per replay"""
    B, dt = 65, BF16
    cases = [Q.qhead_case(B, dt, True)] + [Q.qhead_case(B, dt, True, seed=1000 + k) for k in range(3)]
    prm = [p.to(DEV).requires_grad_() for p in cases[0]["inp"]["params"]]
    inputs = lambda c: (c["inp"]["cls"].to(DEV, dt).requires_grad_(), (c["inp"]["w"] > 0).float().to(DEV))
    cls, y = inputs(cases[0])
    rm, rv, nbt = _state(cases[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _chain(ops, cls, y, prm, rm, rv, nbt)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = _chain(ops, cls, y, prm, rm, rv, nbt)
    KEPT_ALIVE.append((graph, static_out, cls, y, prm, rm, rv, nbt))
    rm0, rv0, nbt0 = _state(cases[0])
    rm.copy_(rm0), rv.copy_(rv0), nbt.copy_(nbt0)
    rm_e, rv_e, nbt_e = _state(cases[0])
    for k, c in enumerate(cases[1:]):
        c2, y2 = inputs(c)
        with torch.no_grad():
            cls.copy_(c2), y.copy_(y2)
        graph.replay()
        eager = _chain(ops, c2, y2, prm, rm_e, rv_e, nbt_e)
        torch.cuda.synchronize()
        assert int(nbt) == 42 + k and int(nbt_e) == 42 + k
        assert all(torch.equal(s, e) for s, e in zip(static_out, eager))
        assert torch.equal(rm, rm_e) and torch.equal(rv, rv_e)


# ------------------------------------------------------------------------------------------ c. the stream-input node with three adds
@pytest.mark.parametrize("p_drop", [0.0, 0.2], ids=["nodrop", "drop"])
@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
@pytest.mark.parametrize("dt", DT, ids=R.dt_name)
def test_stream_node_with_the_vital_sign_add(ops, dt, packed, p_drop, monkeypatch):
    """ops.StreamInputsQieFn (one add row per sample for EACH stream, the vital-sign stream's too) against x + add formed in torch and
    three ops.StreamInputFn nodes (same seeds, so the masks agree): outputs bit for bit (the same forward kernel on the same rounded
    rows); no mtmp_token_sums launch, the three input gradients left in the hand-off dict; every gradient to rounding, with the
    tolerances of test_stream_inputs_node_vs_three_stream_input_nodes (2e-5 fp32: the same fp32 summands over ~300 rows in another
    order, 300 * 2^-24 = 1.8e-5 of the largest; 2e-2 where a bf16 tensor is compared) -- the adds' gradients as the token sums of
    the handed-over tensors against what autograd's broadcast add returns."""
    from tests.test_gpu_parity import check
    g = torch.Generator().manual_seed(23)
    B, Ns = 3, [37, 14, 9]
    rn = lambda *sh: torch.randn(*sh, generator=g)
    xs = [rn(B, n, 256).to(dt) for n in Ns]
    adds = [rn(B, 256).to(dt) for _ in Ns]
    cls, gam, bet = [rn(1, 1, 256) for _ in Ns], [1 + 0.1 * rn(256) for _ in Ns], [0.1 * rn(256) for _ in Ns]
    bott = rn(1, NB, 256)
    ws = [rn(B, NB + 1 + n, 256) for n in Ns]
    kv = torch.tensor([NB + 1 + 37, NB + 1 + 1, NB + 1 + 20], dtype=torch.int32, device=DEV) if packed else None
    pack = ops.row_starts(kv, NB + 1 + Ns[0]) if packed else None
    seeds = [17, 18, 19]

    def leaves(adds_grad):
        L = dict(x=[t.clone().to(DEV).requires_grad_() for t in xs], add=[t.clone().to(DEV).requires_grad_(adds_grad) for t in adds])
        L["prm"] = [t.clone().to(DEV).requires_grad_() for m in range(3) for t in (cls[m], gam[m], bet[m])]
        L["bott"] = bott.clone().to(DEV).requires_grad_()
        return L

    def loss_of(zs):
        tot = 0.0
        for m, z in enumerate(zs):
            w = ws[m].to(DEV)
            if m == 0 and packed:
                rows = torch.cat([int(pack[b]) + torch.arange(int(kv[b]), device=DEV) for b in range(B)])
                tot = tot + (z.reshape(-1, 256)[rows].float() * w.reshape(-1, 256)[:rows.numel()]).sum()
            else:
                tot = tot + (z.float() * w).sum()
        return tot
    # (a) x + add through torch, three nodes
    A = leaves(True)
    za = []
    for m in range(3):
        pk = (pack, kv) if (m == 0 and packed) else (None, None)
        za.append(ops.StreamInputFn.apply(A["x"][m] + A["add"][m].unsqueeze(1), A["prm"][3 * m], A["prm"][3 * m + 1], A["prm"][3 * m + 2],
                                          None, A["bott"], 1e-5, p_drop, seeds[m], *pk))
    loss_of(za).backward()
    # (b) one node, the adds inside the kernels
    Bv = leaves(False)
    called = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (called.append(name), real(name, *a))[1])
    handoff = {}
    meta = dict(pe=[None, None, None], seeds=seeds, pack=(pack, kv) if packed else None, streams=None, qie=handoff)
    zb = ops.StreamInputsQieFn.apply(Bv["x"][0], Bv["x"][1], Bv["x"][2], Bv["bott"], *Bv["add"], 1e-5, 1e-5, 1e-5, p_drop, meta, *Bv["prm"])
    if packed:
        rows0 = torch.cat([int(pack[b]) + torch.arange(int(kv[b]), device=DEV) for b in range(B)])
        assert torch.equal(za[0].reshape(-1, 256)[rows0], zb[0].reshape(-1, 256)[rows0])
    else:
        assert torch.equal(za[0], zb[0])
    assert torch.equal(za[1], zb[1]) and torch.equal(za[2], zb[2])
    loss_of(zb).backward()
    assert "mtmp_token_sums" not in called and called.count("mtmp_stream_input_bwd_grouped") == 1
    assert handoff["kv_off"] == NB + 1 and (handoff["kv_len"] is kv if packed else handoff["kv_len"] is None)
    t = f"qie_stream_node[{R.dt_name(dt)},{'packed' if packed else 'padded'},p={p_drop}]"
    tol = 2e-5 if dt == F32 else 2e-2
    for m in range(3):
        assert torch.equal(handoff["dxs"][m], Bv["x"][m].grad)
        check(f"{t}.dx{m}", Bv["x"][m].grad.float(), A["x"][m].grad.float(), tol)
        check(f"{t}.d_add{m}", handoff["dxs"][m].float().sum(1), A["add"][m].grad.float(), tol)
    if packed:                                        # the pad rows of the packed stream's input gradient are written, as zeros
        live = torch.arange(Ns[0], device=DEV).view(1, -1) < (kv.view(-1, 1) - NB - 1)
        assert float(handoff["dxs"][0][~live].abs().max()) == 0.0
    for k in range(9):
        check(f"{t}.d_prm{k}", Bv["prm"][k].grad, A["prm"][k].grad, 2e-5)
    check(t + ".d_bott", Bv["bott"].grad, A["bott"].grad, 2e-5)
