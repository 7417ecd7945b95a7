"""builder/trainer/validate.py end to end on TRI_MBT_VSLTCLS (2 layers, batch 8, TIE-len 48, bf16): five synthetic batches, the
last of 5 samples, through ``validate()`` with eager launches and replayed from a hipGraph, against the existing
``get_trainer(flow_type="test")`` loop with ``Evaluator`` on the same batches -- logits, mean loss and the reference's metric
list --, the training step that follows a validation pass against the one that follows none, and a pass fed the device-resident
stores' plans against a pass fed the padded tensors of the same samples.  Replayed cases run in a pytest process of their own:
captured graphs are never released (graph.MAX_ALIVE_GRAPHS), and by this point of the suite the process's budget is spent."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import filler
from tests.test_gpu_parity import DEV, ROOT, _Logger, _product_model

pytestmark = pytest.mark.gpu
IN_CHILD = os.environ.get("MTMP_TEST_CHILD") == "1"
T_LEN, SEED = 48, 9100
SIZES = (8, 8, 8, 8, 5)


def _in_child(test_id):
    r = subprocess.run([sys.executable, "-m", "pytest", f"{os.path.abspath(__file__)}::{test_id}", "-x", "-q", "-s", "-m", "gpu",
                        "-p", "no:cacheprovider"], env=dict(os.environ, MTMP_TEST_CHILD="1"), cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0 and "1 passed" in r.stdout


def _model(hip_graph, **over):
    args, model = _product_model(2, 0, "bf16", hip_graph=hip_graph, batch_size=8, TIE_len=T_LEN, **over)
    model.train()
    model.img_encoder.eval()
    return args, model


def _batches():
    """the loader's 12-tuples (2_train.py:223), CPU tensors"""
    out = []
    for k, B in enumerate(SIZES):
        bt = filler.make_batch(SEED + k, B, T_LEN)
        out.append((bt["x"], torch.stack([bt["gen"], bt["age"]], 1), bt["y"], bt["input_lengths"], bt["img"], bt["img_time"],
                    bt["txt"], bt["txt_lengths"], bt["txt_time"], bt["missing"], None, None))
    return out


class _Recording(torch.nn.Module):
    """not a plain BCEWithLogitsLoss instance: the trainer calls it as criterion(output, target)"""

    def __init__(self):
        super().__init__()
        self.logits = []

    def forward(self, output, target):
        self.logits.append(output.detach().reshape(-1).clone())
        return torch.nn.functional.binary_cross_entropy_with_logits(output, target)


def _test_flow(args, model, batches, criterion):
    """the existing path: get_trainer(flow_type='test') per batch, Evaluator, loss.item() per batch"""
    from medical_tri_modal_pilot_amd.builder.trainer import get_trainer
    from medical_tri_modal_pilot_amd.builder.utils.metrics import Evaluator
    lg = _Logger()
    lg.evaluator = Evaluator(args)
    was = [(m, m.training) for m in model.modules()]
    model.eval()
    losses = []
    for x, static, y, in_len, img, img_time, txt, txt_len, txt_time, missing, _f, _y2 in batches:
        _, loss = get_trainer(args=args, iteration=1, x=x, static=static, input_lengths=in_len.clone(), y=y, output_lengths=None,
                              model=model, logger=lg, device=torch.device(DEV), scheduler=None, optimizer=None,
                              criterion=criterion, x_txt=txt, x_img=img, txt_lengths=None if txt_len is None else txt_len.clone(),
                              imgtxt_time=(img_time, txt_time), scaler=None, missing=missing, flow_type="test",
                              reports_tokens=None, reports_lengths=None, criterion_aux=(None, None))
        losses.append(loss)
    for m, t in was:
        m.training = t
    return losses, lg.evaluator


def _validate(args, model, batches, capacity=64):
    from medical_tri_modal_pilot_amd.builder.trainer import validate
    from medical_tri_modal_pilot_amd.builder.utils.device_evaluator import DeviceEvaluator
    ev = DeviceEvaluator(args, DEV, capacity, keep_logits=True)
    res = validate(args, model, batches, torch.device(DEV), torch.nn.BCEWithLogitsLoss(), ev)
    pred, tgt, logit = ev.predictions()
    return res, ev, pred, tgt, logit


def _reference(batches):
    """the existing path on a model of its own: logits (recording criterion), losses and Evaluator (ordinary criterion)"""
    args, model = _model(0)
    rec = _Recording()
    _test_flow(args, model, batches, rec)
    losses, evaluator = _test_flow(args, model, batches, torch.nn.BCEWithLogitsLoss())
    return torch.cat(rec.logits), losses, evaluator


def _check_against_the_test_flow(res, pred, tgt, logit, batches):
    ref_logits, ref_losses, ref_ev = _reference(batches)
    n = sum(SIZES)
    assert res["n"] == n == logit.numel() == ref_logits.numel() and res["batches"] == len(SIZES) and res["status"] == 0
    # (a) the stored logits are those of the existing path, bit for bit
    assert torch.equal(logit.view(torch.int32), ref_logits.float().view(torch.int32))
    assert torch.equal(tgt.cpu(), torch.cat([b[2] for b in batches]).to(torch.uint8))
    # (b) the mean loss: the same float32 losses, summed in float64 in the same order, one division
    assert all(math.isfinite(v) for v in ref_losses)
    assert res["loss"] == sum(ref_losses) / len(ref_losses), (res["loss"], ref_losses)
    # (c) the reference's list.  Preconditions, on the reference side: pairwise distinct probabilities on both sides (two monotone
    #     sigmoids then give the same order) and no unrounded reference metric within 1e-6 of a 4-decimal rounding boundary
    from medical_tri_modal_pilot_amd.builder.utils import metrics as R
    old_p = torch.nan_to_num(torch.cat([p.reshape(-1).float() for p in ref_ev.y_pred_multi]))
    old_t = torch.cat([t.reshape(-1) for t in ref_ev.y_true_multi]).to(torch.uint8)
    assert old_p.unique().numel() == n and pred.unique().numel() == n
    for v in (R.binary_auroc(old_p, old_t), R.binary_average_precision(old_p, old_t), R.binary_f1(old_p, old_t, 0.01)):
        frac = (float(v.double()) * 1e4) % 1.0
        assert abs(frac - 0.5) > 1e-2, f"reference metric {float(v)} sits on a rounding boundary: choose another seed"
    want = ref_ev.performance_metric()
    print("validate:", res, "| Evaluator:", want, "| losses", ref_losses)
    assert [float(v) for v in res["performance_metric"]] == [float(v) for v in want]
    assert 0 < res["n_pos"] < n
    return ref_logits


def test_validate_eager_equals_the_test_flow():
    batches = _batches()
    args, model = _model(0)
    flags = [m.training for m in model.modules()]
    res, ev, pred, tgt, logit = _validate(args, model, batches)
    assert [m.training for m in model.modules()] == flags and model.training and not model.img_encoder.training
    assert not hasattr(model, "_mtmp_graph_eval")
    _check_against_the_test_flow(res, pred, tgt, logit, batches)
    # a second pass over the same batches: reset() inside, the same eight values
    again = _validate(args, model, batches)[0]
    assert {k: (v if v == v else None) for k, v in again.items() if k != "performance_metric"} == \
        {k: (v if v == v else None) for k, v in res.items() if k != "performance_metric"}


def test_validate_replayed_from_a_graph():
    if not IN_CHILD:
        return _in_child("test_validate_replayed_from_a_graph")
    batches = _batches()
    args0, model0 = _model(0)
    logit0 = _validate(args0, model0, batches)[4]
    args, model = _model(1)
    res, ev, pred, tgt, logit = _validate(args, model, batches)
    assert torch.equal(logit.view(torch.int32), logit0.view(torch.int32))          # (a) eager == replayed
    _check_against_the_test_flow(res, pred, tgt, logit, batches)
    # (d) full batches: one warm-up step, one capture, then replays (the capture's own step is a replay); the short batch is eager
    st = model._mtmp_graph_eval.stats()
    print("eval graph:", st)
    assert not model._mtmp_graph_eval.disabled and st["captures"] == 1 and st["replays"] == 3 and st["eager_over_budget"] == 0
    assert not hasattr(model, "_mtmp_graph_step")                                   # the training graph step is untouched
    # a second pass replays every full batch and computes the same values
    res2 = _validate(args, model, batches)
    st2 = model._mtmp_graph_eval.stats()
    assert torch.equal(res2[4].view(torch.int32), logit0.view(torch.int32)) and res2[0]["loss"] == res["loss"]
    assert st2["captures"] == 2 and st2["replays"] == 6             # another evaluator: its buffers are captured afresh


def _train_steps(hip_graph, validate_between):
    """two training steps (three under --hip-graph 1: warm-up, capture, replay), optionally with a validation pass in front of the last"""
    from medical_tri_modal_pilot_amd.builder.trainer import get_trainer
    from medical_tri_modal_pilot_amd.builder.utils.cosine_annealing_with_warmup_v2 import CosineAnnealingWarmupRestarts
    from medical_tri_modal_pilot_amd.builder.models.src.transformer import encoder
    from medical_tri_modal_pilot_amd.optim import FusedAdamW
    torch.manual_seed(0)
    encoder._seed_counter[0] = 0           # the dropout seeds are (torch.initial_seed(), call counter): both runs start alike
    args, model = _model(hip_graph, dropout=0.1)
    opt = FusedAdamW(model.hot_parameters(), lr=args.lr_init, weight_decay=args.weight_decay)
    sched = CosineAnnealingWarmupRestarts(opt, first_cycle_steps=args.t_0 * 10, cycle_mult=args.t_mult,
                                          max_lr=args.lr_init * math.sqrt(args.batch_size), min_lr=1e-6,
                                          warmup_steps=args.t_up * 10, gamma=args.gamma)
    batches = _batches()
    x, static, y, in_len, img, img_time, txt, txt_len, txt_time, missing, _f, _y2 = batches[0]
    kw = dict(args=args, x=x, static=static, y=y, output_lengths=None, model=model, logger=_Logger(), device=torch.device(DEV),
              scheduler=sched, optimizer=opt, criterion=torch.nn.BCEWithLogitsLoss(), x_txt=txt, x_img=img,
              imgtxt_time=(img_time, txt_time), scaler=None, missing=missing, reports_tokens=None, reports_lengths=None,
              criterion_aux=(None, None))
    steps = 3 if hip_graph else 2
    losses = []
    for it in range(1, steps + 1):
        if it == steps and validate_between:
            _validate(args, model, batches)
        losses.append(get_trainer(iteration=it, input_lengths=in_len.clone(), txt_lengths=txt_len.clone(), flow_type="train", **kw)[1])
    torch.cuda.synchronize()
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return losses, opt.flat.data.detach().clone(), state, model


def _check_training_is_untouched(hip_graph):
    l_val, p_val, s_val, model = _train_steps(hip_graph, True)
    l_ref, p_ref, s_ref, _ = _train_steps(hip_graph, False)
    print(f"training around a validation pass[graph {hip_graph}]: losses {l_val} without {l_ref}")
    assert all(math.isfinite(v) for v in l_val)
    assert [np.float32(v).tobytes() for v in l_val] == [np.float32(v).tobytes() for v in l_ref]
    assert torch.equal(p_val, p_ref)
    assert s_val.keys() == s_ref.keys() and all(torch.equal(s_val[k], s_ref[k]) for k in s_val)      # BatchNorm running statistics too
    return model


def test_training_step_after_a_validation_pass_eager():
    _check_training_is_untouched(0)


def test_training_step_after_a_validation_pass_replayed():
    if not IN_CHILD:
        return _in_child("test_training_step_after_a_validation_pass_replayed")
    model = _check_training_is_untouched(1)
    tr, ev = model._mtmp_graph_step.stats(), model._mtmp_graph_eval.stats()
    print("train graph:", tr, "eval graph:", ev)
    assert tr["captures"] == 1 and tr["replays"] == 2 and ev["captures"] == 1 and ev["replays"] == 3


def _store_batches():
    """two batches of four samples as plans of the device-resident stores, and as the padded tensors of the same samples"""
    from medical_tri_modal_pilot_amd.builder.data import ReportStore, collate_packed
    from tests import report_store_model as RM
    from tests import tie_store_model as TM
    tie = TM.new_synthetic_store().to(DEV)
    rep_host = ReportStore.from_mapping(RM.synthetic_mapping())
    rep_dev = ReportStore.from_mapping(RM.synthetic_mapping()).to(DEV, torch.float32)
    pats = TM.synthetic_patients()
    W = [(0, 3, 3), (1, 4, 2), (2, 8, 5), (0, 4, 2)]
    plans, padded = [], []
    for k, (w, ridx) in enumerate(((W, [0, 1, 2, 3]), (W[::-1], [3, 2, 1, 0]))):
        plan = tie.plan(np.asarray(w), 64, 1)
        rows = [TM.reference_window(pats, TM.FMIN, TM.FMAX, p, key, L, 64, 1)[0] for p, key, L in w]
        pb = collate_packed([(r, s, t) for r, s, t in zip(rows, plan.static.numpy(), plan.txt_time.tolist())])
        rplan = rep_dev.plan(np.asarray(ridx))
        bt = filler.make_batch(4321 + k, 4, 64, missing_mode="none")
        missing = torch.stack([bt["missing"][:, 0], bt["missing"][:, 1], rplan.missing], 1)
        plans.append((plan, plan.static, bt["y"], plan.input_lengths, bt["img"], bt["img_time"], rplan, None, plan.txt_time,
                      missing, None, None))
        padded.append((pb.to_padded(64), plan.static.clone(), bt["y"], plan.input_lengths.clone(), bt["img"], bt["img_time"],
                       RM.plan_tokens(rplan, rep_host.emb), rplan.txt_lengths.clone(), plan.txt_time.clone(), missing, None, None))
    return plans, padded


@pytest.mark.parametrize("graph", [0, 1])
def test_validate_on_store_plans_equals_validate_on_padded_tensors(graph):
    if graph == 1 and not IN_CHILD:
        return _in_child(f"test_validate_on_store_plans_equals_validate_on_padded_tensors[{graph}]")
    from medical_tri_modal_pilot_amd.builder.trainer import validate
    from medical_tri_modal_pilot_amd.builder.utils.device_evaluator import DeviceEvaluator
    plans, padded = _store_batches()
    got = []
    for batches in (plans, padded):
        args, model = _product_model(2, 0, "bf16", hip_graph=graph, TIE_len=64)
        model.train()
        model.img_encoder.eval()
        ev, crit = DeviceEvaluator(args, DEV, 16, keep_logits=True), torch.nn.BCEWithLogitsLoss()
        # twice: under --hip-graph 1 the second pass replays both batches
        validate(args, model, batches, torch.device(DEV), crit, ev)
        res = validate(args, model, batches, torch.device(DEV), crit, ev)
        got.append((res, ev.predictions()[2]))
        if graph == 1:
            st = model._mtmp_graph_eval.stats()
            assert st["captures"] >= 1 and st["replays"] >= 2 and st["eager_over_budget"] == 0
    (res_a, logit_a), (res_b, logit_b) = got
    print(f"validate[stores, graph {graph}]: logits plans {logit_a.tolist()} padded {logit_b.tolist()}")
    assert logit_a.numel() == 8 and torch.isfinite(logit_a).all()
    assert torch.equal(logit_a.view(torch.int32), logit_b.view(torch.int32)) and res_a["loss"] == res_b["loss"]


def test_training_loop_with_a_validation_pass():
    """train.py --val-iters 3 with both stores under --hip-graph 1, two epochs at a small size, as the command-line tool it is (a
    process of its own: its graph caches start empty): the validation line of every epoch, the same validation set both times,
    the windows of StoreWindowSweep, the validation graph replayed"""
    import re
    r = subprocess.run([sys.executable, "-m", "medical_tri_modal_pilot_amd.train", "--input-types", "vslt_img_txt", "--model",
                        "tri_mbt_vsltcls", "--modality-inclusion", "train-missing_test-missing", "--lr-init", "1e-5", "--batch-size",
                        "4", "--epochs", "2", "--transformer-num-layers", "2", "--vslt-type", "TIE", "--imgtxt-time", "1",
                        "--mbt-only-vslt", "1", "--TIE-len", "128", "--synthetic", "1", "--iters-per-epoch", "4", "--report-store",
                        "1", "--tie-store", "1", "--hip-graph", "1", "--val-iters", "3", "--val-batch-size", "5"], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0
    val = re.findall(r"epoch (\d): val loss ([0-9.]+) auroc ([0-9.]+) ap ([0-9.]+|nan) f1 ([0-9.]+) \((\d+) predictions, (\d+) positive",
                     r.stdout)
    assert [v[0] for v in val] == ["1", "2"] and all(v[5] == "15" for v in val) and val[0][6] == val[1][6]
    assert all(math.isfinite(float(v[1])) and 0.0 <= float(v[2]) <= 1.0 for v in val)
    assert re.search(r"best auc, apr, f1 \[[0-9., ]+\] at iteration (4|8)\)", r.stdout)
    m = re.search(r"hipGraph \(validation\): (\d+) captures, (\d+) replays, (\d+) eager", r.stdout)
    assert m and int(m.group(1)) == 1 and int(m.group(2)) == 5 and int(m.group(3)) == 0
    t = re.search(r"hipGraph: (\d+) captures, (\d+) replays, (\d+) eager", r.stdout)
    assert t and int(t.group(1)) >= 1 and int(t.group(2)) >= 1 and int(t.group(3)) == 0
