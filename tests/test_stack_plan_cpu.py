"""CPU-only, no library: what the fusion stack nodes run, as stack_plan.StackPlan decides it -- the per-layer schedule against
tables written out by hand here, the combinations the plan refuses, and the host pieces the encoders share (block collector, key
lengths, gradient placement).  The bottleneck prefix is 4 rows."""
import ast
import os

import pytest
import torch

from medical_tri_modal_pilot_amd import stack_plan, tuning
from medical_tri_modal_pilot_amd.stack_plan import LayerStep, StackPlan

ALL, V = (0, 1, 2), (0,)


def plan(**kw):
    base = dict(n_layers=3, kv=[torch.zeros(1, dtype=torch.int32)] * 3, missing=None, drop_p=0.0, seeds=[], fused=[], dtype=torch.bfloat16)
    return StackPlan(**{**base, **kw})


def S(streams, exchange, cls_tok=None, ffn_rows=None, solo=False):
    return LayerStep(streams=streams, cls_tok=cls_tok, ffn_rows=ffn_rows, solo=solo, exchange=exchange)


A = [S(ALL, True), S(ALL, True), S(ALL, True)]
C_KW = dict(vsltonly=1, cls_only=True, exchange_only_layer=1)
SCHEDULES = {
    "A": (dict(), A),
    "B": (dict(vsltonly=1), [S(ALL, True), S(ALL, True), S(V, False)]),
    "C": (C_KW, [S(ALL, True), S(ALL, True, ffn_rows=4), S(V, False, cls_tok=4)]),
    "C-fp32": (dict(C_KW, dtype=torch.float32), [S(ALL, True), S(ALL, True), S(V, False, cls_tok=4)]),
    "D": (dict(n_layers=2, vsltonly=1, final=False, prebuilt=True), [S(ALL, True), S(ALL, True)]),
    "E": (dict(n_layers=2, n_streams=2), [S((0, 1), True), S((0, 1), True)]),
    "F": (dict(inputs_on_side=True), [S(ALL, True, solo=True), S(ALL, True), S(ALL, True)]),
    "G-forward": (dict(bott_rows_unused=True), A),
    "H": (dict(n_layers=1, vsltonly=1), [S(V, False)]),
    "first_only": (dict(first_only=True), [S(ALL, True), S(ALL, True), S(V, False)]),
    "Multi": (dict(first_only=True, exchange_last=False, masks=[None] * 3), [S(ALL, True), S(ALL, True), S(V, False)]),
    "Multi-all": (dict(exchange_last=False, masks=[None] * 3), [S(ALL, True), S(ALL, True), S(ALL, False)]),
}


@pytest.mark.parametrize("case", sorted(SCHEDULES))
def test_schedule_table(case):
    kw, want = SCHEDULES[case]
    p = plan(**kw)
    assert p.schedule() == want
    if not kw.get("bott_rows_unused"):          # without it the backward walks the forward's schedule, whatever gradients arrived
        assert p.backward_schedule(True) == want and p.backward_schedule(False) == want


def test_backward_schedule_prunes_the_last_layer_only_without_gradient_and_resbottle():
    g = plan(bott_rows_unused=True)
    assert g.backward_schedule(True) == [S(ALL, True), S(ALL, True), S(V, False)]           # G
    assert g.backward_schedule(False) == A                                                   # G-grad
    assert plan(bott_rows_unused=True, resbottle=True).backward_schedule(True) == A          # G-res
    assert g.schedule() == A                                                                 # (the forward's is left alone)
    b = plan(bott_rows_unused=True, vsltonly=1)                                              # nothing to prune: B either way
    assert b.backward_schedule(True) == b.schedule() == SCHEDULES["B"][1]
    d = plan(n_layers=2, final=False, prebuilt=True, bott_rows_unused=True)                  # a non-final segment is never pruned
    assert d.backward_schedule(True) == [S(ALL, True), S(ALL, True)]
    e = plan(n_layers=2, n_streams=2, bott_rows_unused=True)
    assert e.backward_schedule(True) == [S((0, 1), True), S(V, False)]


def test_ffn_rows_switch_is_read_when_the_schedule_is_made(monkeypatch):
    p = plan(**C_KW)
    assert p.schedule()[1].ffn_rows == 4
    monkeypatch.setattr(tuning, "FFN_ROWS_BEFORE_LAST", False)
    assert [s.ffn_rows for s in p.schedule()] == [None, None, None]


def test_blocks_of_the_flat_parameter_list():
    assert plan().block(0, 0) == slice(0, 14) and plan().block(2, 1) == slice(98, 112)
    assert plan(n_streams=2).block(2, 1) == slice(70, 84)
    assert plan().sink(1, 2) is None and plan(sinks=[["a", "b", "c"], ["d", "e", "f"]]).sink(1, 2) == "f"


@pytest.mark.parametrize("kw", [dict(final=False), dict(final=False, prebuilt=True, resbottle=True),
                                dict(pack_v=object()), dict(pack_v=object(), prebuilt=True, dtype=torch.float32),
                                dict(pack_v=object(), prebuilt=True, kv=[None] * 3),
                                dict(final=False, prebuilt=True, cls_only=True), dict(final=False, prebuilt=True, first_only=True)])
def test_refused_combinations(kw):
    with pytest.raises(ValueError):
        plan(**kw)


def test_accepted_neighbours_and_unknown_field():
    plan(final=False, prebuilt=True)
    plan(pack_v=object(), prebuilt=True)
    plan(cls_only=True, first_only=True)
    with pytest.raises(TypeError):
        plan(n_stream=2)
    with pytest.raises(TypeError):
        StackPlan(n_layers=1)


def test_module_needs_no_library():
    src = os.path.join(os.path.dirname(stack_plan.__file__), "stack_plan.py")
    names = set()
    for node in ast.walk(ast.parse(open(src).read())):
        if isinstance(node, ast.ImportFrom):
            names |= {node.module} | {a.name for a in node.names}
        elif isinstance(node, ast.Import):
            names |= {a.name for a in node.names}
    assert not names & {"ops", "_lib", "medical_tri_modal_pilot_amd.ops", "medical_tri_modal_pilot_amd._lib"}


# ---- the collector
class StubLayer:
    log = []

    def __init__(self, name):
        self.name = name

    @staticmethod
    def fused_weights_of(blocks, dtype):
        StubLayer.log.append(("fused", [b.name for b in blocks], dtype))
        return ["F" + b.name for b in blocks]

    def param_list(self):
        return [f"{self.name}.p{k}" for k in range(14)]

    def dropout_args(self):
        StubLayer.log.append(("seeds", self.name))
        n = sum(1 for e in StubLayer.log if e[0] == "seeds")
        return 0.25, (2 * n, 2 * n + 1)

    def grad_sink(self):
        return "S" + self.name


def test_collector_keeps_a_dead_block_in_line():
    StubLayer.log = []
    layers = [[StubLayer(f"{li}{m}") for m in range(3)] for li in range(2)]
    dead = lambda li, m: li == 1 and m > 0
    params, fused, seeds, p, sinks = stack_plan.collect_blocks(layers, dead, torch.bfloat16)
    names = ["00", "01", "02", "10", "11", "12"]
    assert params == [f"{n}.p{k}" for n in names for k in range(14)]                    # the dead blocks' parameters included
    assert StubLayer.log[0] == ("fused", ["00", "01", "02", "10"], torch.bfloat16)      # ONE call, before any seed, live blocks only
    assert StubLayer.log[1:] == [("seeds", n) for n in names]                           # layer-major, stream-minor, dead ones too
    assert fused == [["F00", "F01", "F02"], ["F10", None, None]]
    assert seeds == [[(2, 3), (4, 5), (6, 7)], [(8, 9), (10, 11), (12, 13)]] and p == 0.25
    assert sinks == [["S00", "S01", "S02"], ["S10", "S11", "S12"]]
    with torch.no_grad():
        assert stack_plan.collect_blocks(layers, dead, torch.bfloat16)[4] is None
    assert stack_plan.collect_blocks(layers, dead, torch.bfloat16, want_sinks=False)[4] is None


# ---- key lengths and gradient placement
def test_key_lengths():
    lens = [torch.tensor([5, 2, 0]), torch.tensor([9, 9, 9]), torch.tensor([2, 7, 3], dtype=torch.int32)]
    kept = [v.clone() for v in lens]
    got = stack_plan.key_lengths(lens, [True, False, True], 2, "cpu", [1, 1, 1])
    assert got[1] is None and all(v.dtype == torch.int64 for v in (got[0], got[2]))
    assert got[0].tolist() == [6, 3, 1] and got[2].tolist() == [0, 8, 4]               # text: 2 + 1 == 3 -> 0
    assert all(torch.equal(a, b) for a, b in zip(lens, kept))
    assert [v.tolist() for v in stack_plan.key_lengths(lens[:2], [True, True], 1, "cpu", [1, 1])] == [[6, 3, 1], [10, 10, 10]]
    multi = stack_plan.key_lengths([torch.tensor(5), torch.tensor([1, 2, 3]), torch.tensor(3)], [True] * 3, 2, "cpu", [4, 0, 0], batch=3)
    assert [v.tolist() for v in multi] == [[9, 9, 9], [1, 2, 3], [0, 0, 0]]


def test_keep_grads_and_zero_streams():
    pshapes = [(2, 3)] * 28
    pgrads = [None] * 28
    g = [torch.full((6,), float(k)) for k in range(14)]
    stack_plan.keep_grads(pgrads, pshapes, slice(14, 28), None)
    assert pgrads == [None] * 28
    stack_plan.keep_grads(pgrads, pshapes, slice(14, 28), g)
    assert pgrads[:14] == [None] * 14 and all(pgrads[14 + k].shape == (2, 3) and float(pgrads[14 + k][0, 0]) == k for k in range(14))
    a, b = stack_plan.zero_streams([(2, 3, 4), (2, 5, 4)], torch.float32, "cpu")
    assert a.shape == (2, 3, 4) and b.shape == (2, 5, 4) and not a.any() and not b.any() and a.is_contiguous() and b.is_contiguous()
    assert a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()             # one fill for both
