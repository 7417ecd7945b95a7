"""CPU-only checks of the host side: C-ABI surface, state_dict / flag parity with the
reference, trainer integer logic, scheduler, flat parameter storage, and the 2-rank
gradient reducer over gloo.  No HIP kernel is launched here (there is no GPU)."""
import ctypes
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "medical_tri_modal_pilot_amd", "libmtmp_hip.so")


def _args(*extra):
    from medical_tri_modal_pilot_amd.control.config import parse_args
    a = parse_args(["--input-types", "vslt_img_txt", "--model", "tri_mbt_vsltcls", "--modality-inclusion",
                    "train-missing_test-missing", "--batch-size", "4", "--transformer-num-layers", "2",
                    "--imgtxt-time", "1", "--mbt-only-vslt", "1", *extra])
    a.device = torch.device("cpu")
    return a


def test_c_abi_exports_every_declared_symbol():
    if not os.path.exists(LIB):
        import __graft_entry__ as ge
        ge.build()
    hdr = open(os.path.join(ROOT, "include", "mtmp.h")).read()
    declared = set(re.findall(r"\b(mtmp_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 14
    lib = ctypes.CDLL(LIB)                       # loads without a GPU: HIP initialises lazily
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/mtmp.h but not exported"
    from medical_tri_modal_pilot_amd import _lib
    assert set(_lib.SIGNATURES) == declared
    lib.mtmp_abi_version.restype = ctypes.c_int
    assert lib.mtmp_abi_version() == 6


def test_ops_fail_loudly_without_gpu():
    from medical_tri_modal_pilot_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.attn_fwd(torch.zeros(1, 8, 768), None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gemm_nt(torch.zeros(8, 64), torch.zeros(32, 64))


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "medical_tri_modal_pilot_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(d, f)).read()
                assert "oracle" not in src.replace("# oracle", ""), f"{f} mentions the oracle"


def test_state_dict_and_flag_surface_match_reference():
    from medical_tri_modal_pilot_amd.builder.models import get_model
    a = _args()
    model = get_model(a)(a)
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "state_shapes_L2.json")))
    sd = model.state_dict()
    assert set(sd) == set(ref)
    for k, (shape, dtype) in ref.items():
        assert tuple(sd[k].shape) == tuple(shape), k
        assert str(sd[k].dtype).replace("torch.", "") == dtype, k
    # parameters that receive gradients = the golden's grad set (static unused set excluded)
    G = np.load(os.path.join(ROOT, "tests", "golden", "model_step.npz"))
    assert sorted(n for n, _ in model.hot_parameters()) == sorted(str(s) for s in G["grad_names"])
    # README.md:44 command line parses unchanged
    from medical_tri_modal_pilot_amd.control.config import parse_args
    r = parse_args("--input-types vslt_img_txt --model tri_mbt_vsltcls --modality-inclusion train-missing_test-missing "
                   "--lr-init 1e-5 --output-type intubation --batch-size 64 --epochs 50 --transformer-num-layers 6 "
                   "--vslt-type TIE --model-types detection --imgtxt-time 1 --mbt-only-vslt 1 --num-workers 16 "
                   "--multiimages 1".split())
    assert r.batch_size == 64 and r.transformer_num_layers == 6 and r.weight_decay == 1e-6 and r.dropout == 0.1
    with pytest.raises(ValueError):
        get_model(_args("--input-types", "vslt"))(_args("--input-types", "vslt"))      # reference: IndexError


def test_missing_num_bit_exact():
    from medical_tri_modal_pilot_amd.builder.trainer import missing_to_num
    from oracle import tri_mbt_oracle as O
    import filler
    G = np.load(os.path.join(ROOT, "tests", "golden", "model_step.npz"))
    bt = filler.make_batch(int(G["seed"]), int(G["B"]), int(G["T"]))
    mn, _ = missing_to_num(bt["missing"])
    assert torch.equal(mn, torch.from_numpy(G["missing_num"]))
    # template rows only (the product's closed-form fast path) and rows outside the template (vital signs missing,
    # values other than 0/1: they become new unique rows and shift the indices, as in the reference) -- all against
    # the oracle's unique-based restatement of trainer.py:53-77
    for rows in ([[0, 1, 1], [0, 0, 0]], [[0, 0, 1]] * 5, [[0, 1, 0], [0, 1, 1], [0, 0, 1], [0, 0, 0]],
                 [[1, 0, 0], [0, 1, 1]], [[0, 2, 0], [0, 0, 1], [0, 1, 0]], [[0, 0.5, 1], [0, 1, 1]], [[1, 1, 1]] * 3):
        m = torch.tensor(rows, dtype=torch.float32)
        assert torch.equal(missing_to_num(m)[0], O.missing_to_num(m)), rows
    g = torch.Generator().manual_seed(3)
    for _ in range(20):
        m = torch.randint(0, 2, (17, 3), generator=g).float()
        m[:, 0] = 0
        assert torch.equal(missing_to_num(m)[0], O.missing_to_num(m))
        for fd in ("txt1", "img1"):
            got = missing_to_num(m, fd)[0]
            sub = torch.stack([m[:, 0], m[:, 2]]).permute(1, 0) if fd == "txt1" else m[:, :2]
            tmpl = torch.tensor([[0., 0.], [0., 1.]])                              # trainer.py:57-66
            want = torch.unique(torch.cat([tmpl, sub], 0), dim=0, sorted=True, return_inverse=True)[1][2:]
            assert torch.equal(got, want)


def test_missing_memo_answers_only_for_the_same_tensor_object_and_version():
    """the memo of a device-resident `missing` must not match another tensor that merely reuses the address."""
    from medical_tri_modal_pilot_amd.builder.trainer import trainer as T
    memo = T._MissingMemo()
    a = torch.tensor([[0., 1., 1.], [0., 0., 0.]])
    ctx = ("cpu", "txt1_img1", "vslt_img_txt")
    assert memo.lookup(a, ctx) is None
    memo.store(a, ctx, "ids-a")
    assert memo.lookup(a, ctx) == "ids-a"
    assert memo.tensor is a                                 # holds the tensor: its storage cannot be recycled
    assert memo.lookup(a, ("cpu", "txt1", "vslt_img_txt")) is None
    b = a.clone()                                           # equal content, other object: no hit
    assert memo.lookup(b, ctx) is None
    a[0, 1] = 0.                                            # in-place write bumps the version counter
    assert memo.lookup(a, ctx) is None
    memo.store(a, ctx, "ids-a2")
    view = a[:]                                             # a view is another object
    assert memo.lookup(view, ctx) is None
    memo.clear()
    assert memo.lookup(a, ctx) is None
    # host tensors never go through the memo: two different batches in a row
    args = _args()
    T._MISSING_MEMO.clear()
    m1 = torch.tensor([[0., 1., 1.], [0., 0., 0.], [0., 0., 1.], [0., 1., 0.]])
    m2 = torch.tensor([[0., 0., 0.], [0., 1., 1.], [0., 1., 0.], [0., 0., 1.]])
    assert T._missing_ids(args, m1, "cpu").tolist() == [3, 0, 1, 2]
    assert T._missing_ids(args, m2, "cpu").tolist() == [0, 3, 2, 1]
    assert T._MISSING_MEMO.tensor is None


def test_key_lengths_bit_exact():
    from medical_tri_modal_pilot_amd.builder.models.src.transformer.mbt_encoder import TrimodalTransformerEncoder_MBT
    from oracle import tri_mbt_oracle as O
    for multi in (0, 1):
        enc = TrimodalTransformerEncoder_MBT(4, 3, 4, 0, 256, 1, 4, 256, 1024, mask=[True, bool(multi), True])
        in_len, txt_len = torch.tensor([20, 3, 1000, 7]), torch.tensor([20, 0, 126, 1])
        img_time = torch.tensor([[1., 10, 10], [10, 10, 10], [-1, -2, -3], [0.5, 10, 2]])
        img_len = torch.count_nonzero(img_time - 10, dim=1) * 49 if multi else 49
        lens = enc.key_lengths([in_len, img_len, txt_len + 2], "cpu")
        ref = O.fusion_kv_lengths(in_len, txt_len, img_time, multi, 49)
        for got, want in zip(lens, ref):
            if want is None:
                assert got is None
            else:
                assert torch.equal(got + 4, want)
        assert torch.equal(in_len, torch.tensor([20, 3, 1000, 7]))        # caller's tensor is not mutated


def test_scheduler_matches_reference_sequence():
    from medical_tri_modal_pilot_amd.builder.utils.cosine_annealing_with_warmup_v2 import CosineAnnealingWarmupRestarts
    G = np.load(os.path.join(ROOT, "tests", "golden", "sched.npz"))
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.AdamW([p], lr=1e-5)
    s = CosineAnnealingWarmupRestarts(opt, first_cycle_steps=500, cycle_mult=2, max_lr=1e-5 * math.sqrt(64),
                                      min_lr=1e-6, warmup_steps=50, gamma=0.5)
    assert opt.param_groups[0]["lr"] == 1e-6
    for it, lr in zip(G["its"], G["lrs"]):
        s.step(int(it))
        assert opt.param_groups[0]["lr"] == pytest.approx(float(lr), rel=1e-12, abs=0)


def test_flat_params_views_and_grads():
    from medical_tri_modal_pilot_amd.optim import FlatParams
    lin = torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.Linear(3, 2))
    before = {n: p.detach().clone() for n, p in lin.named_parameters()}
    flat = FlatParams(lin.named_parameters())
    for n, p in lin.named_parameters():
        assert torch.equal(p, before[n]) and p.data_ptr() >= flat.data.data_ptr()
    assert all(o % 4 == 0 for o in flat.offsets)
    lin(torch.randn(7, 5)).sum().backward()
    for i, p in enumerate(flat.params):
        lo, hi = flat.slice_of(i)
        assert torch.equal(flat.grad[lo:hi].view_as(p), p.grad) and p.grad.abs().sum() > 0
    flat.zero_grad()
    assert float(flat.grad.abs().sum()) == 0 and all(p.grad.data_ptr() >= flat.grad.data_ptr() for p in flat.params)
    sd = lin.state_dict()
    lin.load_state_dict({k: v + 1 for k, v in sd.items()})                # in-place: views survive
    assert float(flat.data[: 15].sum()) == pytest.approx(float(before["0.weight"].sum()) + 15, rel=1e-5)


def test_sink_param_grads_writes_single_use_gradients_into_the_flat_buffer():
    """ops.sink_param_grads: gradients of single-use parameters go straight into their FlatParams slices (and the
    DDP ready callback fires); a slice that was already written this step, or a parameter outside the flat buffer,
    falls back to returning the gradient to autograd."""
    from medical_tri_modal_pilot_amd import ops
    from medical_tri_modal_pilot_amd.optim import FlatParams
    lin = torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.Linear(3, 2))
    flat = FlatParams(lin.named_parameters())
    flat.zero_grad()
    ready = []
    flat.ready_cb = ready.append
    w, b = lin[0].weight, lin[0].bias
    gw, gb = torch.randn(3, 5), torch.randn(3)
    out = ops.sink_param_grads([w, b], [gw, gb])
    assert out == [None, None]
    assert torch.equal(w.grad, gw) and torch.equal(b.grad, gb)
    assert sorted(ready) == sorted(flat.index_of[id(q)] for q in (w, b))
    again = ops.sink_param_grads([w, b], [gw, gb])            # second writer in the same step: autograd must accumulate
    assert again[0] is gw and again[1] is gb
    flat.zero_grad()
    assert ops.sink_param_grads([w, b], [gw, gb]) == [None, None]          # claim released by zero_grad
    stray = torch.nn.Parameter(torch.zeros(4))
    g = torch.ones(4)
    assert ops.sink_param_grads([stray], [g])[0] is g
    assert ops.sink_param_grads([w, stray], [gw, g])[1] is g


DDP_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.environ["MTMP_ROOT"])
from medical_tri_modal_pilot_amd.optim import FlatParams
from medical_tri_modal_pilot_amd.ddp import GradReducer, broadcast_module_state
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
torch.manual_seed(100 + rank)                      # replicas start different ...
net = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.ReLU(), torch.nn.Linear(32, 8), torch.nn.Linear(8, 1))
unused = torch.nn.Linear(4, 4)                      # a parameter that never gets a gradient (static unused set)
broadcast_module_state(net, 0)                      # ... and are made identical
flat = FlatParams(list(net.named_parameters()) + [("unused." + n, p) for n, p in unused.named_parameters()])
red = GradReducer(flat, bucket_bytes=1024, overlap=True)
assert len(red.buckets) >= 2
ref = [p.detach().clone() for p in net.parameters()]
g = torch.Generator().manual_seed(7)
xs = [torch.randn(6, 16, generator=g) for _ in range(world)]     # every rank can rebuild every shard
for step in range(2):
    flat.zero_grad()
    net(xs[rank]).pow(2).mean().backward()
    red.wait()
    # expected: sum over ranks of single-rank gradients on identical replicas
    exp = [torch.zeros_like(p) for p in ref]
    for r in range(world):
        m = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.ReLU(), torch.nn.Linear(32, 8), torch.nn.Linear(8, 1))
        with torch.no_grad():
            for q, s in zip(m.parameters(), ref):
                q.copy_(s)
        m(xs[r]).pow(2).mean().backward()
        for e, q in zip(exp, m.parameters()):
            e += q.grad
    for p, e in zip(net.parameters(), exp):
        assert torch.allclose(p.grad, e, rtol=1e-5, atol=1e-6), (rank, step)
    assert float(sum(p.grad.abs().sum() for p in unused.parameters())) == 0.0
gathered = [torch.zeros_like(flat.grad) for _ in range(world)]
dist.all_gather(gathered, flat.grad)
assert all(torch.equal(gathered[0], t) for t in gathered)       # every rank holds the same reduced buffer

# ---- staged mode (what hipGraph replays use): hooks only LOG, launch() is called between the stages of a step that
# is cut at an activation (here: after the first Linear), and the result equals the hook-mode result
def expected():
    exp = [torch.zeros_like(p) for p in ref]
    for r in range(world):
        m = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.ReLU(), torch.nn.Linear(32, 8), torch.nn.Linear(8, 1))
        with torch.no_grad():
            for q, s in zip(m.parameters(), ref):
                q.copy_(s)
        m(xs[r]).pow(2).mean().backward()
        for e, q in zip(exp, m.parameters()):
            e += q.grad
    return exp
with torch.no_grad():
    for q, s in zip(net.parameters(), ref):
        q.copy_(s)
red.remove()
flat = FlatParams(net.named_parameters())            # only parameters that do get gradients (the product's hot set)
red = GradReducer(flat, bucket_bytes=1024)
red.staged = True
flat.zero_grad()
h = net[1](net[0](xs[rank]))
loss = net[3](net[2](h)).pow(2).mean()
later = [p for n, p in net.named_parameters() if n.startswith(("2.", "3."))]
torch.autograd.backward(loss, inputs=[h] + later, retain_graph=True)          # stage 0: down to h
assert not red.works                                                            # nothing went out by itself
first = red.take_ready()
assert first and all(red.buckets[b][0] >= flat.offsets[flat.index_of[id(net[2].weight)]] for b in first)
red.launch(first)
torch.autograd.backward([h], [h.grad])                                          # stage 1: the rest
red.launch(red.take_ready())
red.wait()
for p, e in zip(net.parameters(), expected()):
    assert torch.allclose(p.grad, e, rtol=1e-5, atol=1e-6), rank
red.staged = False

# ---- gradient accumulation: no_sync() for every backward but the last; a late gradient raises
flat.zero_grad()
with red.no_sync():
    net(xs[rank]).pow(2).mean().backward()
net(xs[rank]).pow(2).mean().backward()
red.wait()
for p, e in zip(net.parameters(), expected()):
    assert torch.allclose(p.grad, 2 * e, rtol=1e-5, atol=1e-6), rank
flat.zero_grad()
net(xs[rank]).pow(2).mean().backward()
try:
    net(xs[rank]).pow(2).mean().backward()          # second backward without no_sync: its buckets are already in flight
    raise SystemExit("late gradient was accepted")
except RuntimeError as e:
    assert "no_sync" in str(e), e
red.wait()
dist.destroy_process_group()
print("OK", rank)
"""


STAGED_WORKER = r"""
# Two gloo ranks drive the PRODUCT's staged step (builder/trainer/trainer.py _stage_bounds + _staged_step, the stage
# callables GraphedTrainStep captures one hipGraph each from) on a CPU stand-in of the model surface those use:
# fusion_transformer.{n_layers, fusion_idx, graph_segments, segment_boundaries}, backward_stage_params().  The runner
# below is GraphedTrainStep._eager_on_side_stream without the streams: stage, take_ready(), launch().
import os, sys, types, torch, torch.distributed as dist
sys.path.insert(0, os.environ["MTMP_ROOT"])
from medical_tri_modal_pilot_amd.optim import FlatParams
from medical_tri_modal_pilot_amd import ddp as T_ddp
from medical_tri_modal_pilot_amd.ddp import GradReducer, broadcast_module_state
from medical_tri_modal_pilot_amd.builder.trainer import trainer as T
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
D, L = 8, 6


class Enc(torch.nn.Module):
    supports_segments, resbottle = True, False

    def __init__(self):
        super().__init__()
        self.n_layers, self.fusion_idx, self.graph_segments, self.segment_boundaries = L, 0, None, []
        self.layer_stacks = torch.nn.ModuleList(torch.nn.ModuleList(torch.nn.Linear(D, D) for _ in range(3)) for _ in range(L))

    def forward(self, zs):
        self.segment_boundaries = []
        cuts = set(self.graph_segments or ())
        for l, layer in enumerate(self.layer_stacks):
            if l in cuts:
                self.segment_boundaries.append(tuple(zs))
            mix = sum(z.mean(1, keepdim=True) for z in zs) / 3          # the streams meet in every layer, as through the bottleneck
            zs = [torch.tanh(f(z)) + mix for f, z in zip(layer, zs)]
        return zs


class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.inp = torch.nn.ModuleList(torch.nn.Linear(5, D) for _ in range(3))
        self.bn = torch.nn.BatchNorm1d(D)                              # buffers: running stats + num_batches_tracked
        self.fusion_transformer = Enc()
        self.fc_list = torch.nn.Linear(3 * D, 1)

    def forward(self, x):
        zs = [f(x) for f in self.inp]
        zs[1] = self.bn(zs[1].transpose(1, 2)).transpose(1, 2)
        zs = self.fusion_transformer(zs)
        return self.fc_list(torch.cat([z[:, 0] for z in zs], -1))

    def backward_stage_params(self, lo, hi, head):
        pre = tuple(f"fusion_transformer.layer_stacks.{l}." for l in range(lo, hi)) + (("fc_list.",) if head else ())
        return [p for n, p in self.named_parameters() if n.startswith(pre)]


torch.manual_seed(100 + rank)
net = Net()
with torch.no_grad():
    net.bn.running_mean.fill_(float(rank + 1))
    net.bn.num_batches_tracked.fill_(7 * (rank + 1))
broadcast_module_state(net, 0)
assert float(net.bn.running_mean[0]) == 1.0 and int(net.bn.num_batches_tracked) == 7      # rank 0's buffers everywhere
state = [torch.zeros_like(t) for t in list(net.parameters()) + list(net.buffers())]
for s, t in zip(state, list(net.parameters()) + list(net.buffers())):
    s.copy_(t)
    both = [torch.zeros_like(t) for _ in range(world)]
    dist.all_gather(both, t.data)
    assert all(torch.equal(both[0], b) for b in both)

flat = FlatParams(net.named_parameters())
red = GradReducer(flat, bucket_bytes=1024)
red.staged = True
opt = types.SimpleNamespace(flat=flat, zero_grad=flat.zero_grad)
crit = torch.nn.BCEWithLogitsLoss()
args = types.SimpleNamespace(graph_stages=3, vslt_type="TIE")
enc = net.fusion_transformer
assert T._stage_bounds(types.SimpleNamespace(graph_stages=0, vslt_type="TIE"), enc, True) == [0, 1, L]   # DDP default: one cut behind layer 0
bounds = T._stage_bounds(args, enc, True)
assert bounds == [0, 2, 4, 6], bounds
assert len(T._stage_bounds(types.SimpleNamespace(graph_stages=0, vslt_type="TIE"), enc, False)) == 2   # single rank: one graph
enc.graph_segments = bounds[1:-1]
g = torch.Generator().manual_seed(3)
xs = [torch.randn(4, 7, 5, generator=g) for _ in range(world)]
ys = [(torch.rand(4, generator=g) > 0.5).float() for _ in range(world)]
run_model = lambda t: net(t["data"]).squeeze()
stages = T._staged_step(net, enc, opt, crit, run_model, bounds)
assert len(stages) == 3


def reference():
    exp, losses = None, []
    for r in range(world):
        m = Net()
        with torch.no_grad():
            for q, s in zip(list(m.parameters()) + list(m.buffers()), state):
                q.copy_(s)
        loss = crit(m(xs[r]).squeeze(), ys[r])
        loss.backward()
        gs = [q.grad.clone() for q in m.parameters()]
        exp = gs if exp is None else [a + b for a, b in zip(exp, gs)]
        losses.append(float(loss))
    return exp, losses


exp, losses = reference()
for step in range(2):                                                # the second step re-arms hooks, buckets and the log
    with torch.no_grad():
        for q, s in zip(list(net.parameters()) + list(net.buffers()), state):
            q.copy_(s)
    carry, per_stage = {}, []
    inputs = dict(data=xs[rank], final_target=ys[rank])
    for st in stages:
        st(inputs, carry)
        assert not red.works or per_stage                              # nothing goes out before the first launch()
        ids = red.take_ready()
        per_stage.append(list(ids))
        red.launch(ids)
    red.wait()
    assert abs(float(carry["loss"]) - losses[rank]) < 1e-6
    assert len(carry["bnds"]) == 2
    sent = [b for ids in per_stage for b in ids]
    assert sorted(sent) == list(range(len(red.buckets))), (per_stage, len(red.buckets))    # every bucket once
    assert all(per_stage), per_stage                                   # every stage completed buckets of its own
    # stage 0 only sent buckets that lie entirely in [first parameter of layer 4, end): layers 4, 5 and the head
    lo4 = flat.offsets[flat.index_of[id(enc.layer_stacks[4][0].weight)]]
    assert all(red.buckets[b][0] >= lo4 for b in per_stage[0]), per_stage
    lo2 = flat.offsets[flat.index_of[id(enc.layer_stacks[2][0].weight)]]
    assert all(red.buckets[b][0] >= lo2 for b in per_stage[1]), per_stage
    for (n, p), e in zip(net.named_parameters(), exp):
        assert torch.allclose(p.grad, e, rtol=1e-5, atol=1e-6), (rank, step, n)
    # the collectives went out in the order of the plan: per stage the merged ranges of its buckets
    plan = red.plan(per_stage)
    assert red.last_issued == [tuple(r) for st in plan for r in st], (red.last_issued, plan)
# The plan was agreed on by all ranks in the first staged step's wait() (ONE collective, at a point every rank reaches together) ...
assert red.verified_plan == red.plan(per_stage), (red.verified_plan, per_stage)
assert sum(len(st) for st in red.verified_plan) >= 3, red.verified_plan
# ... so a capture is compared with it LOCALLY: ranks whose ragged batches give them different shape signatures capture on
# different steps (ADVICE r4), and a collective tied to the capture would pair with the peers' gradient all-reduces.  Here the
# ranks "capture" one after the other, with a barrier in between: a collective inside assert_same_plan would deadlock.
for turn in range(world):
    if rank == turn:
        assert red.assert_same_plan(per_stage) == red.verified_plan
    dist.barrier()
# a capture that completed other bucket sets is refused on the spot, on the rank it happened on
bad = [list(ids) for ids in per_stage]
bad[0], bad[1] = bad[1], bad[0]
try:
    red.assert_same_plan(bad)
    raise SystemExit("a differing captured plan was accepted")
except T_ddp.PlanMismatch as e:
    assert "differ from the plan the ranks agreed on" in str(e), e
# ... and the agreement itself catches a rank that differs -- on EVERY rank, in front of the step's last all-reduce.  (Only the
# LOG of rank 1 is tampered with: the collectives actually issued still pair up, so nothing hangs while the check is tested.)
red.verified_plan = None
with torch.no_grad():
    for q, s in zip(list(net.parameters()) + list(net.buffers()), state):
        q.copy_(s)
carry = {}
for st in stages:
    st(dict(data=xs[rank], final_target=ys[rank]), carry)
    red.launch(red.take_ready())
if rank == 1:
    red.launch_log[0], red.launch_log[1] = red.launch_log[1], red.launch_log[0]
try:
    red.wait()
    raise SystemExit("differing plans were accepted")
except T_ddp.PlanMismatch as e:
    assert "plans other collectives" in str(e), e
for w in red.works:
    w.wait()
red.works = []
red._reset()
# parameter equality after an update from the reduced gradients (what the optimizer does with 1 / world folded in)
red.verified_plan = None
with torch.no_grad():
    for q, s in zip(list(net.parameters()) + list(net.buffers()), state):
        q.copy_(s)
carry = {}
for st in stages:
    st(dict(data=xs[rank], final_target=ys[rank]), carry)
    red.launch(red.take_ready())
red.wait()
with torch.no_grad():
    for q in net.parameters():
        q -= 0.1 * q.grad / world
    chk = torch.stack([q.double().sum() for q in net.parameters()] + [q.double().abs().sum() for q in net.parameters()])
both = [torch.zeros_like(chk) for _ in range(world)]
dist.all_gather(both, chk)
assert all(torch.equal(both[0], b) for b in both), "replicas diverged"
dist.destroy_process_group()
print("OK", rank)
"""


def test_bi_vslttxt_model_surface_matches_reference():
    """get_model(--model bi_vslttxt_mbt_v1) -> the reference's state_dict keys / shapes and gradient set."""
    from medical_tri_modal_pilot_amd.builder.models import get_model
    a = _args()
    a.input_types, a.model = "vslt_txt", "bi_vslttxt_mbt_v1"
    model = get_model(a)(a)
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "state_shapes_bi_vslttxt_L2.json")))
    sd = model.state_dict()
    assert set(sd) == set(ref)
    for k, (shape, dtype) in ref.items():
        assert tuple(sd[k].shape) == tuple(shape) and str(sd[k].dtype).replace("torch.", "") == dtype, k
    G = np.load(os.path.join(ROOT, "tests", "golden", "bimodel_step.npz"))
    assert sorted(n for n, _ in model.hot_parameters()) == sorted(str(s) for s in G["grad_names"])
    with pytest.raises(NotImplementedError):
        a.model = "tri_mbt_vmulti"        # (a sibling that is not built: DESIGN.md section 8)
        get_model(a)


@pytest.mark.parametrize("name,input_types,tag", [("tri_mbt_vsltcls_noshareumse", "vslt_img_txt", "noshareumse"), ("tri_mbt_v1", "vslt_img_txt", "tri_v1"),
                                                  ("tri_mbt_vflexible", "vslt_img_txt", "tri_vflex"), ("tri_mbt_vflexible2", "vslt_img_txt", "tri_vflex2"),
                                                  ("tri_mbt_vflexible3", "vslt_img_txt", "tri_vflex3"),
                                                  ("bi_vsltimg_mbt_v1", "vslt_img", "bi_vsltimg"), ("bitxt_mbt_vflexible1", "vslt_txt", "bitxt_vflex1"),
                                                  ("biimg_mbt_vflexible1", "vslt_img", "biimg_vflex1"), ("tri_mbt_v2", "vslt_img_txt", "tri_v2"),
                                                  ("tri_mbt_vnoshavgtr", "vslt_img_txt", "tri_vnoshavgtr")])
def test_more_sibling_model_surfaces_match_reference(name, input_types, tag):
    """SURVEY 8 f-4 / VERDICT r2 missing #3: the other two siblings whose forward returns -- state_dict keys / shapes of the
    real classes, parameter ORDER (what torch.optim.AdamW(model.parameters()) state is indexed by), gradient set."""
    from medical_tri_modal_pilot_amd.builder.models import get_model
    a = _args()
    a.input_types, a.model, a.output_dim = input_types, name, 1
    if name == "tri_mbt_v2":
        a.berttype = "bert"                 # token-id reports (tri_mbt_v2.py:205)
    model = get_model(a)(a)
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", f"state_shapes_{tag}_L2.json")))
    sd = model.state_dict()
    assert set(sd) == set(ref), set(sd) ^ set(ref)
    for k, (shape, dtype) in ref.items():
        assert tuple(sd[k].shape) == tuple(shape) and str(sd[k].dtype).replace("torch.", "") == dtype, k
    pnames = [n for n, _ in model.named_parameters()]
    assert pnames == [k for k in ref if k in set(pnames)]               # registration order = the reference's
    G = np.load(os.path.join(ROOT, "tests", "golden", f"{tag}_step.npz"))
    want = sorted(str(s) for s in G["grad_names"])      # (the image encoder included where the reference trains it: bi_vsltimg_mbt_v1)
    assert sorted(n for n, _ in model.hot_parameters()) == want


def test_bench_launches_its_own_ranks(tmp_path):
    """`python bench.py --gpus 2` with no launcher environment starts two ranks as children of a GPU-free parent
    (torch.distributed.run on 127.0.0.1) and relays rank 0's JSON line; --dry-run stops before the first GPU call."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    line = [l for l in r.stdout.decode().splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d == {"dry_run": True, "n_gpus": 2, "rccl_ranks": 2, "max_rank": 1}


def test_bench_dump_outputs_float_files_and_fixed_sample(tmp_path, monkeypatch):
    """bench.py --dump-outputs: the loss as float64, the flat parameter / gradient buffers as float32, a buffer larger than
    DUMP_MAX_ELEMS as the same seeded sample of positions in every run."""
    import types
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    flat = types.SimpleNamespace(data=torch.arange(5000, dtype=torch.float32), grad=-torch.arange(5000, dtype=torch.float32))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), 0.25, flat)
    for d in ("a", "b"):
        assert sorted(os.listdir(tmp_path / d)) == ["grads.npy", "loss.npy", "params.npy"]
        loss = np.load(tmp_path / d / "loss.npy")
        assert loss.dtype == np.float64 and loss.tolist() == [0.25]
    p, g = np.load(tmp_path / "a" / "params.npy"), np.load(tmp_path / "a" / "grads.npy")
    assert p.dtype == g.dtype == np.float32 and p.shape == g.shape == (1000,)
    assert np.array_equal(p, -g) and len(np.unique(p)) == 1000 and np.all(np.diff(p) > 0)
    assert np.array_equal(p, np.load(tmp_path / "b" / "params.npy"))


def test_flat_params_claim_refuses_slices_autograd_accumulated_into():
    """A backward kernel may overwrite a gradient slice only if nothing was accumulated into it since zero_grad()."""
    from medical_tri_modal_pilot_amd.optim import FlatParams
    lin = torch.nn.Linear(5, 3)
    flat = FlatParams(lin.named_parameters())
    flat.zero_grad()
    idx = [flat.index_of[id(lin.weight)]]
    lin(torch.randn(2, 5)).sum().backward()          # autograd accumulates into the flat views
    assert flat.accumulated and not flat.claim(idx)
    flat.zero_grad()
    assert flat.claim(idx) and not flat.claim(idx)   # free after zero_grad, once


def test_fused_adamw_state_dict_speaks_the_reference_layout():
    """optimizer.state_dict() / load_state_dict() as the reference's Logger.save / resume code calls them
    (logger.py:167, 2_train.py:98): moments indexed like torch.optim.AdamW(model.parameters())."""
    from medical_tri_modal_pilot_amd.optim import FusedAdamW
    net = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.Linear(3, 2), torch.nn.Linear(2, 1))
    hot = [(n, p) for n, p in net.named_parameters() if not n.startswith("1.")]      # a subset, in another order
    hot = hot[2:] + hot[:2]
    opt = FusedAdamW(hot, lr=1e-3, reference_params=list(net.parameters()))
    assert opt.state_dict()["state"] == {}                    # nothing stepped yet
    opt.exp_avg.copy_(torch.arange(opt.exp_avg.numel()).float())
    opt.exp_avg_sq.copy_(torch.arange(opt.exp_avg_sq.numel()).float() * 2)
    opt.step_count = 7
    sd = opt.state_dict()
    ref = torch.optim.AdamW(net.parameters(), lr=1e-3)
    assert len(sd["param_groups"][0]["params"]) == len(list(net.parameters()))
    assert sorted(sd["state"]) == [0, 1, 4, 5]                # positions in model.parameters(); Linear 1 is not trained
    ref.load_state_dict({"state": sd["state"], "param_groups": sd["param_groups"]})           # torch accepts it as is
    assert float(ref.state[net[2].weight]["step"]) == 7
    j = opt.flat.index_of[id(net[2].weight)]
    lo, hi = opt.flat.slice_of(j)
    assert torch.equal(ref.state[net[2].weight]["exp_avg"].reshape(-1), opt.exp_avg[lo:hi])
    opt2 = FusedAdamW(hot, lr=1e-3, reference_params=list(net.parameters()))
    opt2.load_state_dict(ref.state_dict())                   # a checkpoint written by the reference's own AdamW
    assert opt2.step_count == 7
    for j in range(len(opt.flat.params)):                    # (alignment padding between slices belongs to nobody)
        lo, hi = opt.flat.slice_of(j)
        assert torch.equal(opt2.exp_avg[lo:hi], opt.exp_avg[lo:hi]) and torch.equal(opt2.exp_avg_sq[lo:hi], opt.exp_avg_sq[lo:hi])
    # a stepped checkpoint WITHOUT the entry of a trained parameter (torch creates state at the first gradient): that parameter
    # would resume at step 0 in the reference, here at the global step -- refused
    partial = ref.state_dict()
    del partial["state"][4]
    with pytest.raises(ValueError, match="no entry for 1 trained parameter"):
        FusedAdamW(hot, lr=1e-3, reference_params=list(net.parameters())).load_state_dict(partial)


def test_grad_reducer_two_ranks_gloo(tmp_path):
    script = tmp_path / "ddp_worker.py"
    script.write_text(DDP_WORKER)
    env = dict(os.environ, MTMP_ROOT=ROOT, MASTER_ADDR="127.0.0.1", MASTER_PORT="29613", WORLD_SIZE="2",
               OMP_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(2)]
    outs = [p.communicate(timeout=240)[0].decode() for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"OK {r}" in o, o


@pytest.mark.parametrize("world", [2, 8])
def test_product_staged_step_two_ranks_gloo(tmp_path, world):
    """E3: trainer._stage_bounds / _staged_step (the stage callables of the hipGraph step under DDP) with ddp.GradReducer in
    staged mode on gloo ranks (2, and the 8 of one MI355X node): three stages, every bucket launched once behind the stage that
    completed it, gradients = the sum of the single-rank gradients; broadcast_module_state carries the BatchNorm buffers; the
    plan agreement (one collective in the first staged step, local comparisons at every capture: ranks capture on different
    steps), a differing plan caught on every rank; replicas equal after an update."""
    script = tmp_path / "staged_worker.py"
    script.write_text(STAGED_WORKER)
    env = dict(os.environ, MTMP_ROOT=ROOT, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29617 + world), WORLD_SIZE=str(world),
               OMP_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(world)]
    outs = [p.communicate(timeout=400)[0].decode() for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"OK {r}" in o, o
