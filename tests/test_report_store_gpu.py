"""The report gather on the GPU (csrc/report_store.hip through ops.report_tokens): the reference's text branch reproduced from a
device-resident store in all four type pairs -- digests of the reference's own ``__getitem__`` output for float32, torch's
conversion of it for the others --, the edge shapes, the bfloat16 rounding, and trainer steps fed the plan against steps fed
the host-built float32 tensor.  Every comparison is exact: the gather copies or converts, it does no other arithmetic."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import filler
from medical_tri_modal_pilot_amd.builder.data import ReportStore
from tests import report_store_model as M
from tests.test_gpu_parity import DEV, ROOT, _Logger, _product_model

pytestmark = pytest.mark.gpu
IN_CHILD = os.environ.get("MTMP_TEST_CHILD") == "1"
F32, BF16 = torch.float32, torch.bfloat16
PAIRS = [(F32, F32), (BF16, BF16), (F32, BF16), (BF16, F32)]


@pytest.fixture(scope="module")
def ops():
    from medical_tri_modal_pilot_amd import ops as _ops
    return _ops


def _stores(mapping, **kw):
    """the same reports three times: on the host (float32, for the model) and on the device in both types"""
    return {"host": ReportStore.from_mapping(mapping, **kw), F32: ReportStore.from_mapping(mapping, **kw).to(DEV, F32),
            BF16: ReportStore.from_mapping(mapping, **kw).to(DEV, BF16)}


@pytest.fixture(scope="module")
def gstores():
    return _stores(M.golden_mapping())


@pytest.fixture(scope="module")
def sstores():
    return _stores(M.synthetic_mapping())


def _want(ref32, src, dst):
    """torch's conversion of the reference's float32 batch along the pair's path"""
    x = ref32 if src == F32 else ref32.to(BF16)
    return x.to(dst)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.cpu().contiguous().view(torch.uint8).flatten().equal(
        b.cpu().contiguous().view(torch.uint8).flatten())


def _check_pairs(ops, stores, idx, comb=None, tag=""):
    ref = None
    for src, dst in PAIRS:
        batch = stores[src].plan(np.asarray(idx, np.int64), comb)
        if ref is None:
            ref = M.plan_tokens(batch, stores["host"].emb)
        got = ops.report_tokens(batch, DEV, dst)
        assert got.dtype == dst and tuple(got.shape) == (len(idx), batch.max_tokens, batch.width) and got.is_contiguous()
        ne = int((got.cpu().float() != _want(ref, src, dst).float()).sum())
        print(f"report_tokens[{tag} {src} -> {dst}]: B {len(idx)}, lengths {batch.txt_lengths.tolist()[:12]}: {ne} values differ")
        assert _same_bits(got, _want(ref, src, dst))
    return ref


def test_golden_cases(ops, gstores):
    """the 40 cases of the reference's __getitem__ as one batch and as four batches of ten"""
    g = M.golden()
    idx = M.golden_report_idx(gstores["host"])
    for lo, hi in [(0, 40), (0, 10), (10, 20), (20, 30), (30, 40)]:
        batch = gstores[F32].plan(idx[lo:hi], g["case_comb"][lo:hi])
        assert batch.txt_lengths.tolist() == g["text_length"][lo:hi].tolist()
        got = ops.report_tokens(batch, DEV, F32)
        assert [M.digest(t) for t in got] == g["sha256"][lo:hi].tolist()
        ref = _check_pairs(ops, gstores, idx[lo:hi], g["case_comb"][lo:hi], f"golden {lo}:{hi}")
        assert _same_bits(got, ref)


def test_edge_shapes(ops, sstores):
    # synthetic reports by index: 0 tokens, 1, 37, 128 (= L), 127 (= L - 1), 5
    for i in (0, 1, 4, 3):
        _check_pairs(ops, sstores, [i], tag=f"B 1 report {i}")
    _check_pairs(ops, sstores, [2, 2, 5, 2], tag="one report three times")
    _check_pairs(ops, sstores, [0, -1, 3, 1], [0, 0, 1, 3], tag="all missing")
    # rows that are no multiple of a wave's 1 KiB: L 3 x W 40 (120 elements a sample) and W 8
    small = {f"s{k}": {"embedding": M.golden_embedding(200 + k, n, 40)} for k, n in enumerate((3, 0, 1, 2))}
    _check_pairs(ops, _stores(small, width=40, max_tokens=3), [0, 1, 2, 3, 0, -1, 3], tag="L 3 W 40")
    tiny = {f"t{k}": {"embedding": M.golden_embedding(300 + k, n, 8)} for k, n in enumerate((5, 1, 4))}
    _check_pairs(ops, _stores(tiny, width=8, max_tokens=5), [2, 0, 1], tag="L 5 W 8")


def test_zeros_come_from_the_kernel_and_nothing_else_is_written(ops, sstores):
    idx = np.asarray([1, 0, 3, 5, 4], np.int64)
    for src, dst in PAIRS:
        batch = sstores[src].plan(idx)
        ref = _want(M.plan_tokens(batch, sstores["host"].emb), src, dst)
        big = torch.full((len(idx) + 2, 128, 768), float("nan"), dtype=dst, device=DEV)
        out = ops.report_tokens(batch, DEV, dst, out=big[1:-1])
        assert out.data_ptr() == big[1].data_ptr() and _same_bits(out, ref) and not torch.isnan(out).any()
        assert torch.isnan(big[0]).all() and torch.isnan(big[-1]).all()
    with pytest.raises(ValueError, match="out must be a contiguous"):
        ops.report_tokens(batch, DEV, F32, out=torch.empty(5, 128, 768, dtype=BF16, device=DEV))
    with pytest.raises(ValueError, match="out must be a contiguous"):
        ops.report_tokens(batch, DEV, F32, out=torch.empty(4, 128, 768, device=DEV))
    with pytest.raises(RuntimeError, match="store.to"):
        ops.report_tokens(sstores["host"].plan(idx), DEV, F32)


def test_descriptor_rows_outside_the_store_give_zeros(ops, sstores):
    """through ``tables``: rows the plan would never make -- behind the store's tokens, more tokens than L, negative -- zero
    their own sample and leave the neighbours exact"""
    idx = np.asarray([3, 2, 4, 5, 2, 1], np.int64)
    for src, dst in PAIRS:
        st = sstores[src]
        batch = st.plan(idx)
        desc = batch.descriptor()
        desc[1] = torch.tensor([st.n_tokens - 2, 5])          # its last three rows lie behind the store
        desc[3] = torch.tensor([0, 129])                      # n > L
        desc[4] = torch.tensor([-1, 4])
        want = _want(M.plan_tokens(batch, sstores["host"].emb), src, dst)
        want[[1, 3, 4]] = 0
        out = torch.full((6, 128, 768), float("nan"), dtype=dst, device=DEV)
        ops.report_tokens(batch, DEV, dst, out=out, tables=desc.to(DEV))
        assert _same_bits(out, want)
    desc[4] = torch.tensor([st.n_tokens, 0])                  # an empty run at the very end is in bounds
    ops.report_tokens(batch, DEV, dst, out=out, tables=desc.to(DEV))
    assert not out[4].any()


def test_bfloat16_rounding(ops):
    """ties to even both ways, the overflow to inf, denormals, +-0: float32 store -> bfloat16 out has the bits of torch's
    .to(torch.bfloat16); bfloat16 store -> float32 out widens exactly; NaN, through the raw entry only, stays NaN"""
    r = M.rounding_values()
    st = ReportStore.from_mapping({"r": {"embedding": r[np.isfinite(r)].reshape(-1, 8)}}, width=8, max_tokens=r.size // 8).to(DEV, F32)
    batch = st.plan(np.asarray([0, 0]))
    got = ops.report_tokens(batch, DEV, BF16)
    want = torch.tensor(r).to(BF16).reshape(1, -1, 8).expand(2, -1, -1)
    assert torch.isinf(want.float()).sum() == 8 and (want.float() == 0).sum() >= 8
    assert _same_bits(got, want.contiguous())
    assert np.array_equal(got[0].cpu().view(torch.int16).numpy().view(np.uint16).reshape(-1), M.bf16_bits_rne(r))
    stb = ReportStore.from_mapping({"r": {"embedding": r.reshape(-1, 8)[:4]}}, width=8, max_tokens=4).to(DEV, BF16)
    wide = ops.report_tokens(stb.plan(np.asarray([0])), DEV, F32)
    assert _same_bits(wide, torch.tensor(r.reshape(-1, 8)[:4]).to(BF16).float().reshape(1, 4, 8))
    # NaN cannot enter a store (from_mapping refuses it): quiet, signalling and negative ones through the entry itself
    nan_bits = np.asarray([0x7FC00000, 0x7F800001, 0xFFC00000, 0xFF800001, 0x7FFFFFFF, 0x7F80FFFF, 0x7FBFFFFF, 0xFFFFFFFF], np.uint32)
    emb = torch.from_numpy(nan_bits.view(np.float32).copy()).reshape(1, 8).to(DEV)
    desc = torch.tensor([[0, 1]], dtype=torch.int64, device=DEV)
    for dst in (BF16, F32):
        out = torch.zeros(1, 2, 8, dtype=dst, device=DEV)
        ops.call("mtmp_report_gather", ops._p(emb), 0, 1, ops._p(desc), ops._p(out), ops._dt(out), 1, 2, 8, ops._stream())
        assert torch.isnan(out[0, 0]).all() and not out[0, 1].any()
    assert _same_bits(out[0, 0], emb[0])                      # the float32 copy keeps every bit


# ---------------------------------------------------------------------------------------------------------- the trainer
def _steps(bt, x_txt, txt_lengths, hip_graph, dtype):
    """two training steps and one evaluation call of TRI_MBT_VSLTCLS (2 layers, TIE-len 64); txt_lengths: one per call"""
    from medical_tri_modal_pilot_amd.builder.trainer import get_trainer
    from medical_tri_modal_pilot_amd.builder.utils.cosine_annealing_with_warmup_v2 import CosineAnnealingWarmupRestarts
    from medical_tri_modal_pilot_amd.optim import FusedAdamW
    args, model = _product_model(2, 0, dtype, hip_graph=hip_graph, TIE_len=64)
    model.train()
    model.img_encoder.eval()
    opt = FusedAdamW(model.hot_parameters(), lr=args.lr_init, weight_decay=args.weight_decay)
    sched = CosineAnnealingWarmupRestarts(opt, first_cycle_steps=args.t_0 * 10, cycle_mult=args.t_mult,
                                          max_lr=args.lr_init * math.sqrt(args.batch_size), min_lr=1e-6,
                                          warmup_steps=args.t_up * 10, gamma=args.gamma)
    lg = _Logger()
    kw = dict(args=args, x=bt["x"], static=torch.stack([bt["gen"], bt["age"]], 1), y=bt["y"], output_lengths=None, model=model,
              logger=lg, device=torch.device(DEV), scheduler=sched, optimizer=opt, criterion=torch.nn.BCEWithLogitsLoss(),
              x_txt=x_txt, x_img=bt["img"], imgtxt_time=(bt["img_time"], bt["txt_time"]), scaler=None, missing=bt["missing"],
              reports_tokens=None, reports_lengths=None, criterion_aux=(None, None))
    tl = lambda k: None if txt_lengths[k] is None else txt_lengths[k].clone()
    losses = [get_trainer(iteration=it, input_lengths=bt["input_lengths"].clone(), txt_lengths=tl(it - 1), flow_type="train",
                          **kw)[1] for it in (1, 2)]
    torch.cuda.synchronize()
    params = opt.flat.data.detach().clone()
    model.eval()
    losses.append(get_trainer(iteration=3, input_lengths=bt["input_lengths"].clone(), txt_lengths=tl(2), flow_type="test", **kw)[1])
    target, output = lg.evaluator.calls[-1]
    return losses, params, target.detach().clone(), output.detach().clone(), args, model, kw


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("graph", [0, 1])
def test_trainer_step_on_report_batch_equals_step_on_host_tensor(sstores, graph, dtype):
    """TRI_MBT_VSLTCLS, B 4, 2 layers, TIE-len 64, two steps and one evaluation call: the ReportBatch through the trainer's
    ops.report_tokens against the float32 [4, 128, 768] host tensor the reference's loader builds for the same reports (lengths
    0, 1, 37, 128) -- losses, every parameter and the evaluator's inputs, bit for bit.  The bf16 build rests on
    test_bfloat16_rounding: if this fails while that passes, the difference is in the plumbing, not the kernel.  The store is
    float32 for the eager steps and of the build's own type for the replayed ones.  The replayed cases run in a process of their
    own (below)."""
    if graph == 1 and not IN_CHILD:
        # Captured graphs are never released and a process may hold 64 of them (graph.MAX_ALIVE_GRAPHS): by this point of the
        # whole suite the budget is spent and the steps would run eagerly -- the graph 0 case once more.  The replayed case
        # therefore runs where the cache starts empty, in a pytest process of its own, which asserts the replays below.
        r = subprocess.run([sys.executable, "-m", "pytest", f"{os.path.abspath(__file__)}::"
                            f"test_trainer_step_on_report_batch_equals_step_on_host_tensor[{graph}-{dtype}]", "-x", "-q", "-s", "-m",
                            "gpu", "-p", "no:cacheprovider"], env=dict(os.environ, MTMP_TEST_CHILD="1"), cwd=ROOT,
                           capture_output=True, text=True, timeout=300)
        print(r.stdout[-3000:], r.stderr[-2000:])
        assert r.returncode == 0 and "1 passed" in r.stdout
        return
    store = sstores[F32 if graph == 0 or dtype == "fp32" else BF16]
    plan = store.plan(np.asarray([0, 1, 2, 3]))
    assert plan.txt_lengths.tolist() == [0, 1, 37, 128]
    host = M.plan_tokens(plan, sstores["host"].emb)
    bt = filler.make_batch(4321, 4, 64, missing_mode="none")
    bt["missing"] = torch.stack([bt["missing"][:, 0], bt["missing"][:, 1], plan.missing], 1)
    l_rep, p_rep, t_rep, o_rep, args, model, kw = _steps(bt, plan, [None, plan.txt_lengths, None], graph, dtype)
    l_host, p_host, t_host, o_host, _, model_host, _ = _steps(bt, host, [plan.txt_lengths] * 3, graph, dtype)
    print(f"report-store trainer[graph {graph}, {dtype}, store {store.dtype}]: losses plan {l_rep} host tensor {l_host}")
    assert all(math.isfinite(v) for v in l_rep)
    assert [np.float32(v).tobytes() for v in l_rep] == [np.float32(v).tobytes() for v in l_host]
    assert torch.equal(p_rep, p_host) and torch.equal(t_rep, t_host) and torch.equal(o_rep, o_host)
    if graph == 1:            # both runs replayed their second step from a captured graph; none fell back to eager launches
        for m in (model, model_host):
            gs = m._mtmp_graph_step
            print("graph cache:", gs.stats())
            assert not gs.disabled and gs.captures == 1 and gs.replays >= 1 and gs.eager_over_budget == 0
        want = BF16 if dtype == "bf16" else F32              # the static text input of the plan's graph is in the compute type
        sig = dict((k, dt) for k, _, dt in model._mtmp_graph_step.capture_log[-1]["signature"][:-1])
        assert sig["x_txt"] == want and dict((k, dt) for k, _, dt in model_host._mtmp_graph_step.capture_log[-1]["signature"][:-1])["x_txt"] == F32
    if graph == 0 and dtype == "bf16":
        from medical_tri_modal_pilot_amd.builder.trainer import get_trainer
        with pytest.raises(ValueError, match="txt_lengths differs"):
            get_trainer(iteration=4, input_lengths=bt["input_lengths"].clone(), txt_lengths=torch.tensor([0, 1, 37, 127]),
                        flow_type="test", **kw)
        with pytest.raises(ValueError, match="None or a host tensor"):
            get_trainer(iteration=4, input_lengths=bt["input_lengths"].clone(), txt_lengths=plan.txt_lengths.to(DEV),
                        flow_type="test", **kw)
        args.berttype = "bert"
        with pytest.raises(ValueError, match="--berttype bert reads token ids"):
            get_trainer(iteration=4, input_lengths=bt["input_lengths"].clone(), txt_lengths=None, flow_type="test", **kw)


def test_training_loop_with_both_stores_under_hip_graph():
    """train.py --report-store 1 --tie-store 1 --hip-graph 1 for a handful of iterations at a small size, as the command-line
    tool it is: a process of its own, whose graph cache starts empty (captured graphs are never released, and the budget of a
    process that has run the rest of the suite is spent)"""
    import re
    r = subprocess.run([sys.executable, "-m", "medical_tri_modal_pilot_amd.train", "--input-types", "vslt_img_txt", "--model",
                        "tri_mbt_vsltcls", "--modality-inclusion", "train-missing_test-missing", "--lr-init", "1e-5", "--batch-size",
                        "4", "--epochs", "1", "--transformer-num-layers", "2", "--vslt-type", "TIE", "--imgtxt-time", "1",
                        "--mbt-only-vslt", "1", "--TIE-len", "128", "--synthetic", "1", "--iters-per-epoch", "6", "--report-store",
                        "1", "--tie-store", "1", "--hip-graph", "1"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert "report store: 256 reports" in r.stdout and "event store:" in r.stdout
    loss = re.search(r"epoch 1: mean loss ([0-9.eE+-]+|nan|inf)", r.stdout)
    assert loss and math.isfinite(float(loss.group(1)))
    m = re.search(r"hipGraph: (\d+) captures, (\d+) replays, (\d+) eager", r.stdout)
    assert m and int(m.group(1)) >= 1 and int(m.group(2)) >= 1 and int(m.group(3)) == 0
