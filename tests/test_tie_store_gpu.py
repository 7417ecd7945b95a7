"""The event-window gather on the GPU (csrc/tie_store.hip through ops.tie_windows): bit-equal to the host path of the same
windows -- ``tie_window`` / the reference goldens, ``collate_packed`` and ``PackedTieBatch.on_device`` -- in the packed and the
padded form, with and without the fp16 rounding; and a trainer step fed the plan against the step fed the host-built batch.
Every comparison is exact: the gather does no arithmetic whose rounding is free."""
import json
import math
import os

import numpy as np
import pytest
import torch

import filler
from medical_tri_modal_pilot_amd.builder.data import PackedTie, collate_packed
from tests import tie_store_model as M
from tests.test_gpu_parity import DEV, ROOT, O, _Logger, _product_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from medical_tri_modal_pilot_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def gstore():
    return M.new_golden_store().to(DEV)


@pytest.fixture(scope="module")
def sstore():
    return M.new_synthetic_store().to(DEV)


def _host_batch(rows, batch):
    """the parent's host path for the same windows: collate_packed of tie_window's rows"""
    return collate_packed([(r, s, t) for r, s, t in zip(rows, batch.static.numpy(), batch.txt_time.tolist())])


def _check_all_forms(ops, batch, rows, tag):
    """rows: per sample what tie_window returns.  Packed, packed into a 4096 bucket, padded, and without the rounding."""
    pb = _host_batch(rows, batch)
    t_pad = batch.max_len + 3
    want = pb.on_device("cpu", t_pad)
    got = ops.tie_windows(batch, DEV, t_pad)
    assert isinstance(got, PackedTie) and got.t_pad == t_pad and got.events.dtype == torch.float32
    ne = int((got.events.cpu() != want.events).sum())
    print(f"tie_windows[{tag}]: B {batch.batch_size}, {batch.total_rows} rows, longest {batch.max_len}: {ne} values differ")
    assert torch.equal(got.events.cpu(), want.events) and torch.equal(got.cu_seqlens.cpu(), want.cu_seqlens)
    assert got.cu_seqlens.dtype == torch.int32 and torch.equal(batch.input_lengths, pb.input_lengths)
    assert torch.equal(batch.txt_time, pb.txt_time) and torch.equal(batch.static, pb.static)
    bucket = ops.tie_windows(batch, DEV, t_pad, bucket=4096)
    wantb = pb.on_device("cpu", t_pad, bucket=4096)
    assert bucket.events.shape == wantb.events.shape and bucket.events.shape[0] % 4096 == 0
    assert torch.equal(bucket.events.cpu(), wantb.events) and not bucket.events[batch.total_rows:].any()
    padded = ops.tie_windows(batch, DEV, t_pad, padded=True)
    assert padded.shape == (batch.batch_size, t_pad, 3) and torch.equal(padded.cpu(), pb.to_padded(t_pad).half().float())
    raw = ops.tie_windows(batch, DEV, t_pad, round_fp16=False)
    assert raw.events.cpu().numpy().tobytes() == np.concatenate(rows).astype(np.float32).tobytes()


@pytest.mark.parametrize("k", range(len(M.golden_groups())))
def test_golden_cases(ops, gstore, k):
    g, off = M.golden(), M.golden_offsets()
    rt, tl, sel = M.golden_groups()[k]
    batch = gstore.plan(g["case"][sel][:, 2:5], tl, rt)
    rows = [g["seq_cat"][off[c]:off[c] + int(g["len"][c])] for c in sel]          # the reference's own __getitem__ output
    _check_all_forms(ops, batch, rows, f"golden realtime {rt} tie_len {tl}")


@pytest.mark.parametrize("rt,tl", M.SYNTHETIC_CONFIGS)
def test_synthetic_patients(ops, sstore, rt, tl):
    """one batch of every synthetic window (None hours at either end, empty present hours, over 1000 events -- a sample across
    several row chunks --, cuts inside the initial rows and the events, empty and full initial blocks) against tie_window"""
    pats, wins = M.synthetic_patients(), M.synthetic_windows()
    batch = sstore.plan(wins, tl, rt)
    rows = [M.reference_window(pats, M.FMIN, M.FMAX, p, key, L, tl, rt)[0] for p, key, L in wins.tolist()]
    if tl == M.CHUNK_CASE["tie_len"]:
        b = wins.tolist().index(list(M.CHUNK_CASE["window"]))
        assert int(batch.input_lengths[b]) == batch.max_len == 4 * M.CHUNK_ROWS + 6
    _check_all_forms(ops, batch, rows, f"synthetic realtime {rt} tie_len {tl}")


def test_edge_shapes(ops, sstore):
    pats = M.synthetic_patients()
    ref = lambda w, tl, rt: [M.reference_window(pats, M.FMIN, M.FMAX, p, key, L, tl, rt)[0] for p, key, L in w]
    # B = 1
    w = [M.CHUNK_CASE["window"]]
    for rt in (1, 0):
        _check_all_forms(ops, sstore.plan(np.asarray(w), 1200, rt), ref(w, 1200, rt), f"B 1 realtime {rt}")
    # the same patient three times (twice the very same window)
    w = [(0, 8, 7), (0, 8, 7), (0, 11, 3)]
    _check_all_forms(ops, sstore.plan(np.asarray(w), 1000, 0), ref(w, 1000, 0), "one patient three times")
    # buffers pre-filled with NaN: the kernel, not a memset, writes the zeros behind the rows
    batch = sstore.plan(np.asarray(w), 1000, 1)
    pb = _host_batch(ref(w, 1000, 1), batch)
    n = batch.total_rows
    out = torch.full((4096, 3), float("nan"), device=DEV)
    pk = ops.tie_windows(batch, DEV, 64, bucket=4096, out=out)
    assert pk.events.data_ptr() == out.data_ptr() and torch.equal(out.cpu(), pb.on_device("cpu", 64, bucket=4096).events)
    assert not out[n:].any() and not torch.isnan(out).any()
    out = torch.full((3, 70, 3), float("nan"), device=DEV)
    ops.tie_windows(batch, DEV, 70, padded=True, out=out)
    assert torch.equal(out.cpu(), pb.to_padded(70).half().float())
    out = torch.full((n + 5, 3), float("nan"), device=DEV)          # an unbucketed buffer: nothing behind the batch's rows is written
    ops.tie_windows(batch, DEV, 64, out=out[:n])
    assert torch.isnan(out[n:]).all() and torch.equal(out[:n].cpu(), pb.on_device("cpu", 64).events)
    # a descriptor row that points behind the store's events: its rows are zeros in both forms, its neighbours are untouched
    desc, cu = batch.descriptor(), batch.cu_seqlens
    desc[1, 0] = sstore.n_events - 2
    tables = (desc.to(DEV), cu.to(DEV))
    want = pb.on_device("cpu", 64).events.clone()
    want[int(cu[1]):int(cu[2])] = 0
    out = torch.full((n, 3), float("nan"), device=DEV)
    ops.tie_windows(batch, DEV, 64, out=out, tables=tables)
    assert torch.equal(out.cpu(), want)
    out = torch.full((3, 70, 3), float("nan"), device=DEV)
    ops.tie_windows(batch, DEV, 70, padded=True, out=out, tables=tables)
    wantp = pb.to_padded(70).half().float()
    wantp[1] = 0
    assert torch.equal(out.cpu(), wantp)
    with pytest.raises(RuntimeError, match="t_pad 10 is smaller"):
        ops.tie_windows(batch, DEV, 10, padded=True)


# ---------------------------------------------------------------------------------------------------------- the trainer
def _noshareumse_model(hip_graph, T):
    """TRI_MBT_VSLTCLS_NOSHAREUMSE as tests/test_gpu_parity.py builds it (filled from the recorded state shapes)"""
    from medical_tri_modal_pilot_amd.builder.models import get_model
    from medical_tri_modal_pilot_amd.control.config import parse_args
    with open(os.path.join(ROOT, "tests", "golden", "state_shapes_noshareumse_L2.json")) as f:
        shapes = json.load(f)
    sd = {k: filler.fill_tensor(k, torch.zeros(s)) for k, (s, dt_) in shapes.items() if dt_.startswith("float")}
    sd["fusion_transformer.positional_encoding.pe"] = O.sinusoid_table(2500, 256).unsqueeze(0)
    a = parse_args(["--input-types", "vslt_img_txt", "--model", "tri_mbt_vsltcls_noshareumse", "--modality-inclusion",
                    "train-missing_test-missing", "--lr-init", "1e-5", "--batch-size", "4", "--transformer-num-layers", "2",
                    "--imgtxt-time", "1", "--mbt-only-vslt", "1", "--dropout", "0.0", "--compute-dtype", "bf16",
                    "--hip-graph", str(hip_graph), "--TIE-len", str(T)])
    a.device, a.output_dim = torch.device(DEV), 1
    model = get_model(a)(a)
    model.load_state_dict(sd, strict=False)
    return a, model.to(DEV)


def _two_steps(bt, x, hip_graph, T, noshare=False):
    from medical_tri_modal_pilot_amd.builder.trainer import get_trainer
    from medical_tri_modal_pilot_amd.builder.utils.cosine_annealing_with_warmup_v2 import CosineAnnealingWarmupRestarts
    from medical_tri_modal_pilot_amd.optim import FusedAdamW
    args, model = _noshareumse_model(hip_graph, T) if noshare else _product_model(2, 0, "bf16", hip_graph=hip_graph, TIE_len=T)
    model.train()
    model.img_encoder.eval()
    opt = FusedAdamW(model.hot_parameters(), lr=args.lr_init, weight_decay=args.weight_decay)
    sched = CosineAnnealingWarmupRestarts(opt, first_cycle_steps=args.t_0 * 10, cycle_mult=args.t_mult,
                                          max_lr=args.lr_init * math.sqrt(args.batch_size), min_lr=1e-6,
                                          warmup_steps=args.t_up * 10, gamma=args.gamma)
    kw = dict(args=args, x=x, static=bt["static"], y=bt["y"], output_lengths=None, model=model, logger=_Logger(),
              device=torch.device(DEV), scheduler=sched, optimizer=opt, criterion=torch.nn.BCEWithLogitsLoss(),
              x_txt=bt["txt"], x_img=bt["img"], imgtxt_time=(bt["img_time"], bt["txt_time"]), scaler=None,
              missing=bt["missing"], reports_tokens=None, reports_lengths=None, criterion_aux=(None, None))
    losses = [get_trainer(iteration=it, input_lengths=bt["input_lengths"].clone(), txt_lengths=bt["txt_lengths"].clone(),
                          flow_type="train", **kw)[1] for it in (1, 2)]
    torch.cuda.synchronize()
    return losses, opt.flat.data.detach().clone()


def _trainer_batches(sstore, T):
    """four windows of the synthetic patients (a head-trimmed and a tail-trimmed one among them) as the plan and as the host
    path's PackedTieBatch; the other modalities from the synthetic filler"""
    pats = M.synthetic_patients()
    w = [(0, 3, 3), (1, 4, 2), (2, 8, 5), (0, 4, 2)]
    assert {"none_head", "none_tail"} <= set().union(*(M.kinds_of(pats, *x, T) for x in w))
    plan = sstore.plan(np.asarray(w), T, 1)
    pb = _host_batch([M.reference_window(pats, M.FMIN, M.FMAX, p, key, L, T, 1)[0] for p, key, L in w], plan)
    bt = filler.make_batch(4321, 4, T, missing_mode="none")
    bt.update(static=plan.static, input_lengths=plan.input_lengths, txt_time=plan.txt_time)
    return plan, pb, bt


@pytest.mark.parametrize("graph", [0, 1])
def test_trainer_step_on_window_batch_equals_step_on_packed_batch(sstore, graph):
    """TRI_MBT_VSLTCLS, B 4, 2 layers, TIE-len 64, bf16, two steps: the TieWindowBatch through the trainer's ops.tie_windows
    against the PackedTieBatch the host path builds for the same windows -- loss and every parameter, bit for bit."""
    plan, pb, bt = _trainer_batches(sstore, 64)
    l_win, p_win = _two_steps(bt, plan, graph, 64)
    l_pkd, p_pkd = _two_steps(bt, pb, graph, 64)
    print(f"tie-store trainer[graph {graph}]: losses windows {l_win} packed {l_pkd}")
    assert all(math.isfinite(v) for v in l_win)
    assert [np.float32(v).tobytes() for v in l_win] == [np.float32(v).tobytes() for v in l_pkd]
    assert torch.equal(p_win, p_pkd)


def test_trainer_step_of_a_model_without_packed_batches_gets_the_padded_form(sstore):
    """TRI_MBT_VSLTCLS_NOSHAREUMSE refuses packed batches: the trainer hands it the padded tensor of the same launch; against
    the step fed the reference's zero-padded [B, TIE-len, 3] batch"""
    plan, pb, bt = _trainer_batches(sstore, 64)
    l_win, p_win = _two_steps(bt, plan, 0, 64, noshare=True)
    l_pad, p_pad = _two_steps(bt, pb.to_padded(64), 0, 64, noshare=True)
    print(f"tie-store trainer[noshareumse]: losses windows {l_win} padded {l_pad}")
    assert all(math.isfinite(v) for v in l_win)
    assert [np.float32(v).tobytes() for v in l_win] == [np.float32(v).tobytes() for v in l_pad]
    assert torch.equal(p_win, p_pad)
