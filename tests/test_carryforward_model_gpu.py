"""``--vslt-type carryforward`` end to end on the GPU: one train-mode step of TRI_MBT_VSLTCLS against the REAL class
(tests/golden/carryforward_step.npz) with the HIP embedding and with the torch chain; trainer steps fed a HourlyWindowBatch against
steps fed the host tensor of the same windows, eager and replayed from a hipGraph (bit for bit: the gather is exact); a validation
pass over StoreWindowSweep; the trainer's refusals.  The replayed case runs in a pytest process of its own: captured graphs are
never released (graph.MAX_ALIVE_GRAPHS), and by this point of the suite the process's budget may be spent."""
import json
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import filler
from tests import hourly_store_model as H
from tests import tie_store_model as M
from tests.test_gpu_parity import DEV, ROOT, TOL, G, O, _digest, _Logger, _rel, check

pytestmark = pytest.mark.gpu
IN_CHILD = os.environ.get("MTMP_TEST_CHILD") == "1"


def _model(dtype, hip_graph=0):
    from medical_tri_modal_pilot_amd.builder.models import get_model
    from medical_tri_modal_pilot_amd.control.config import parse_args
    with open(os.path.join(ROOT, "tests", "golden", "state_shapes_carryforward_L2.json")) as f:
        shapes = json.load(f)
    sd = {k: filler.fill_tensor(k, torch.zeros(s)) for k, (s, dt_) in shapes.items() if dt_.startswith("float")}
    sd["fusion_transformer.positional_encoding.pe"] = O.sinusoid_table(2500, 256).unsqueeze(0)
    a = parse_args(["--input-types", "vslt_img_txt", "--model", "tri_mbt_vsltcls", "--modality-inclusion", "train-missing_test-missing",
                    "--lr-init", "1e-5", "--batch-size", "4", "--transformer-num-layers", "2", "--imgtxt-time", "1",
                    "--mbt-only-vslt", "1", "--dropout", "0.0", "--compute-dtype", dtype, "--hip-graph", str(hip_graph),
                    "--vslt-type", "carryforward"])
    a.device, a.output_dim = torch.device(DEV), 1
    model = get_model(a)(a)
    missing = model.load_state_dict(sd, strict=False)
    assert not [k for k in missing.missing_keys if "relative_position_index" not in k and "idx" not in k], missing
    model = model.to(DEV).train()
    model.img_encoder.eval()
    return a, model, shapes


@pytest.mark.parametrize("hip_embed", [True, False])
def test_train_step_vs_golden(hip_embed, monkeypatch):
    """fp32 build against the real TRI_MBT_VSLTCLS with vslt_type carryforward: logits, loss, every gradient digest, the
    no-gradient set and the state_dict; with tuning.HIP_HOURLY_EMBED on (ops.HourlyEmbedFn) and off (the torch chain)."""
    from medical_tri_modal_pilot_amd import ops, tuning
    monkeypatch.setattr(tuning, "HIP_HOURLY_EMBED", hip_embed)
    seen = []
    real = ops.HourlyEmbedFn.forward
    monkeypatch.setattr(ops.HourlyEmbedFn, "forward", staticmethod(lambda *a: (seen.append(1), real(*a))[1]))
    Gd = G("carryforward_step")
    a, model, shapes = _model("fp32")
    assert {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in model.state_dict().items()} == shapes
    assert tuple(model.vslt_enc[0].weight.shape) == (256, 16)
    bt = filler.make_batch(int(Gd["seed"]), int(Gd["B"]), int(Gd["T"]))
    dv = lambda t: t.to(DEV)
    x, lens, mnum = torch.from_numpy(Gd["x"]), torch.from_numpy(Gd["input_lengths"]), torch.from_numpy(Gd["missing_num"])
    assert tuple(x.shape) == (4, 24, 16) and lens.tolist() == [24, 1, 7, 13]
    out, o2, o3 = model(dv(x), None, None, None, None, dv(bt["age"]), dv(bt["gen"]), dv(lens.clone()), dv(bt["txt"]),
                        dv(bt["txt_lengths"].clone()), dv(bt["img"]), dv(mnum), None, dv(bt["img_time"].half().float()),
                        dv(bt["txt_time"].half().float()), "train", None, None)
    assert o2 is None and o3 is None and tuple(out.shape) == tuple(Gd["logits"].shape)
    assert bool(seen) == hip_embed
    tag = f"carryforward_step[fp32,hip_embed={int(hip_embed)}]"
    check(tag + ".logits", out, torch.from_numpy(Gd["logits"]), TOL[torch.float32])
    loss = torch.nn.BCEWithLogitsLoss()(out.squeeze(-1), dv(bt["y"].float()))
    print(tag, "loss", float(loss.detach()), "golden", float(Gd["loss"]))
    assert abs(float(loss.detach()) - float(Gd["loss"])) < 1e-5
    loss.backward()
    names = [str(s) for s in Gd["grad_names"]]
    med = float(np.median(Gd["grad_digest"][:, 0]))
    prm = dict(model.named_parameters())
    worst, n_checked = 0.0, 0
    for n_, gd in zip(names, Gd["grad_digest"]):
        assert prm[n_].grad is not None, n_
        if gd[0] < 1e-4 * med:
            assert float(_digest(prm[n_].grad)[0]) < 1e-3 * med, n_
            continue
        e = _rel(_digest(prm[n_].grad), torch.from_numpy(gd))
        if n_.startswith("vslt_enc."):
            print(tag, n_, e)
        worst, n_checked = max(worst, e), n_checked + 1
    for n_ in (str(s) for s in Gd["nograd_names"]):
        assert prm[n_].grad is None, n_
    print(tag, "worst gradient digest", worst, "of", n_checked)
    assert all(n_ in names for n_ in ("vslt_enc.0.weight", "vslt_enc.0.bias", "vslt_enc.1.weight", "vslt_enc.1.bias"))
    assert worst < TOL[torch.float32] and n_checked >= 80, (worst, n_checked)


# ---------------------------------------------------------------------------------------------------------- the trainer
def _golden_windows():
    """four golden windows (L = 24, L = 1 and a patient that is not the first among them), their plan on an uploaded store, and
    the host tensor [B, 3, 24, 16] the reference's loader hands over for them (planes 1 and 2 are read by no model here)"""
    g = H.golden()
    case = g["case"]
    rt1 = np.flatnonzero(case[:, 0] == 1)
    pick = [int(rt1[case[rt1, 3] == 24][0]), int(rt1[case[rt1, 3] == 1][-1]), int(rt1[(case[rt1, 3] > 1) & (case[rt1, 3] < 24)][3]),
            int(rt1[(case[rt1, 1] > 2) & (case[rt1, 3] > 4)][0])]
    store = M.new_golden_store().to(DEV)
    plan = store.plan_hourly(case[pick][:, 1:4], 24, g["keep"], 1)
    host = torch.zeros(4, 3, 24, 16)
    host[:, 0] = torch.from_numpy(g["plane0"][pick])
    bt = filler.make_batch(4321, 4, 24, missing_mode="none")
    bt.update(static=plan.static, input_lengths=plan.input_lengths, txt_time=plan.txt_time)
    assert plan.input_lengths.tolist() == g["len"][pick].tolist() and {1, 24} <= set(plan.input_lengths.tolist())
    return plan, host, bt


def _two_steps(bt, x, hip_graph, dtype="bf16", slices=None):
    from medical_tri_modal_pilot_amd.builder.trainer import get_trainer
    from medical_tri_modal_pilot_amd.builder.utils.cosine_annealing_with_warmup_v2 import CosineAnnealingWarmupRestarts
    from medical_tri_modal_pilot_amd.optim import FusedAdamW
    args, model, _ = _model(dtype, hip_graph)
    opt = FusedAdamW(model.hot_parameters(), lr=args.lr_init, weight_decay=args.weight_decay)
    sched = CosineAnnealingWarmupRestarts(opt, first_cycle_steps=args.t_0 * 10, cycle_mult=args.t_mult,
                                          max_lr=args.lr_init * math.sqrt(args.batch_size), min_lr=1e-6,
                                          warmup_steps=args.t_up * 10, gamma=args.gamma)
    kw = dict(args=args, x=x, static=bt["static"], y=bt["y"], output_lengths=None, model=model, logger=_Logger(),
              device=torch.device(DEV), scheduler=sched, optimizer=opt, criterion=torch.nn.BCEWithLogitsLoss(),
              x_txt=bt["txt"], x_img=bt["img"], imgtxt_time=(bt["img_time"], bt["txt_time"]), scaler=None,
              missing=bt["missing"], reports_tokens=None, reports_lengths=None, criterion_aux=(None, None))
    losses, grads = [], []
    for it in (1, 2):
        losses.append(get_trainer(iteration=it, input_lengths=bt["input_lengths"].clone(), txt_lengths=bt["txt_lengths"].clone(),
                                  flow_type="train", **kw)[1])
        grads.append(opt.flat.grad.detach().clone())
    torch.cuda.synchronize()
    gs = getattr(model, "_mtmp_graph_step", None)
    if slices is not None:          # where the embedding's four parameters lie in the flat buffers
        flat = opt.flat
        for n_, q in model.named_parameters():
            if n_.startswith("vslt_enc."):
                i = flat.index_of[id(q)]
                slices[n_] = (int(flat.offsets[i]), int(flat.offsets[i]) + q.numel())
    return losses, grads, opt.flat.data.detach().clone(), (gs.stats() if gs is not None else None)


def _step_on_plan_equals_step_on_host_tensor(graph):
    plan, host, bt = _golden_windows()
    l_win, g_win, p_win, st_win = _two_steps(bt, plan, graph)
    l_host, g_host, p_host, _ = _two_steps(bt, host, graph)
    print(f"carryforward trainer[graph {graph}]: losses windows {l_win} host {l_host}, graph {st_win}")
    assert all(math.isfinite(v) for v in l_win) and all(float(g.abs().sum()) > 0 for g in g_win)
    assert [np.float32(v).tobytes() for v in l_win] == [np.float32(v).tobytes() for v in l_host]
    assert all(torch.equal(a, b) for a, b in zip(g_win, g_host)) and torch.equal(p_win, p_host)
    if graph:
        assert st_win is not None and st_win["captures"] >= 1 and st_win["replays"] >= 1 and st_win["eager_over_budget"] == 0, st_win


def test_trainer_step_on_hourly_batch_equals_step_on_host_tensor_eager():
    """TRI_MBT_VSLTCLS carryforward, B 4, 2 layers, bf16, two steps with --hip-graph 0: loss, flat gradient and parameters"""
    _step_on_plan_equals_step_on_host_tensor(0)


def test_trainer_step_on_hourly_batch_equals_step_on_host_tensor_graphed():
    """the same with --hip-graph 1, in a process of its own (module docstring); the steps must have been replayed"""
    if not IN_CHILD:
        r = subprocess.run([sys.executable, "-m", "pytest", f"{os.path.abspath(__file__)}::"
                            "test_trainer_step_on_hourly_batch_equals_step_on_host_tensor_graphed", "-x", "-q", "-s", "-m", "gpu",
                            "-p", "no:cacheprovider"], env=dict(os.environ, MTMP_TEST_CHILD="1"), cwd=ROOT, capture_output=True,
                           text=True, timeout=300)
        print(r.stdout[-4000:], r.stderr[-2000:])
        assert r.returncode == 0 and "1 passed" in r.stdout
        return
    _step_on_plan_equals_step_on_host_tensor(1)


def test_flat_gradient_of_the_hip_embedding_equals_the_torch_chains(monkeypatch):
    """the trainer's flat gradient buffer (ops.sink_param_grads writes the embedding's four gradients there, dW through a
    transposing copy) with the HIP embedding against the torch chain, whose gradients autograd hands over: fp32 build, one step"""
    from medical_tri_modal_pilot_amd import tuning
    _, host, bt = _golden_windows()
    got = {}
    for on in (True, False):
        monkeypatch.setattr(tuning, "HIP_HOURLY_EMBED", on)
        sl = {}
        losses, grads, _, _ = _two_steps(bt, host, 0, "fp32", sl)
        got[on] = (losses[0], grads[0], sl)
    assert sorted(got[True][2]) == ["vslt_enc.0.bias", "vslt_enc.0.weight", "vslt_enc.1.bias", "vslt_enc.1.weight"]
    assert abs(got[True][0] - got[False][0]) < 1e-5
    for n_, (lo, hi) in got[True][2].items():
        assert got[False][2][n_] == (lo, hi) and float(got[True][1][lo:hi].abs().sum()) > 0
        check(f"carryforward_flat_grad[fp32].{n_}", got[True][1][lo:hi], got[False][1][lo:hi], TOL[torch.float32])
    check("carryforward_flat_grad[fp32].all", got[True][1], got[False][1], TOL[torch.float32])


def test_validate_pass_over_the_store_sweep():
    """two batches of StoreWindowSweep through validate(): as HourlyWindowBatch plans and as the host tensors of the same windows"""
    from medical_tri_modal_pilot_amd.builder.data import StoreWindowSweep
    from medical_tri_modal_pilot_amd.builder.trainer import validate
    from medical_tri_modal_pilot_amd.builder.utils.device_evaluator import DeviceEvaluator
    store = M.new_synthetic_store().to(DEV)
    sweep = StoreWindowSweep(store, 24)
    args, model, _ = _model("bf16", 0)

    def batches(as_plan):
        out = []
        for k in range(2):
            plan = store.plan_hourly(np.stack([sweep[(4 * k + j) * 3 % len(sweep)] for j in range(4)]), 24, None, 1)
            bt = filler.make_batch(777 + k, 4, 24)
            x = plan
            if not as_plan:
                x = torch.zeros(4, 3, 24, 16)
                x[:, 0] = torch.from_numpy(H.model_of(plan))
            out.append((x, plan.static, bt["y"], plan.input_lengths, bt["img"], bt["img_time"], bt["txt"], bt["txt_lengths"],
                        plan.txt_time, bt["missing"], None, None))
        return out
    res = []
    for as_plan in (True, False):
        ev = DeviceEvaluator(args, DEV, 16, keep_logits=True)
        r = validate(args, model, batches(as_plan), torch.device(DEV), torch.nn.BCEWithLogitsLoss(), ev)
        res.append((r, ev.predictions()[2].cpu()))
    print("carryforward validate:", res[0][0])
    assert res[0][0]["n"] == 8 and math.isfinite(res[0][0]["loss"]) and model.training
    assert torch.equal(res[0][1], res[1][1]) and res[0][0]["loss"] == res[1][0]["loss"]


def test_trainer_refusals():
    from medical_tri_modal_pilot_amd.builder.trainer.trainer import prepare_step_inputs
    store = M.new_synthetic_store().to(DEV)
    w = np.asarray([(1, 5, 3), (0, 8, 2)])
    t = torch.zeros(2)
    names = [str(i) for i in range(16)]

    def prep(x, **over):
        a = types.SimpleNamespace(vslt_type="carryforward", vitalsign_labtest=names, window_size=24, TIE_len=1000,
                                  auxiliary_loss_type="None", fullmodal_definition="txt1_img1", input_types="vslt_img_txt")
        for k, v in over.items():
            setattr(a, k, v)
        model = types.SimpleNamespace(takes_packed_tie=True, compute_dtype=torch.float32)
        return prepare_step_inputs(a, x, torch.zeros(2, 2), torch.tensor([3, 2]), t, model, torch.device(DEV), False, False,
                                   x_img=torch.zeros(2, 1, 8, 8), x_txt=torch.zeros(2, 4, 768), txt_lengths=torch.tensor([1, 1]),
                                   imgtxt_time=(t, t), missing=torch.zeros(2, 3))
    hb = store.plan_hourly(w)
    inp = prep(hb)
    assert tuple(inp.data.shape) == (2, 24, 16) and inp.data.is_cuda and inp.input_lengths.tolist() == [3, 2]
    with pytest.raises(ValueError, match="--vslt-type TIE"):
        prep(hb, vslt_type="TIE")
    with pytest.raises(ValueError, match="keeps 16 columns.*names 15"):
        prep(hb, vitalsign_labtest=names[:15])
    with pytest.raises(ValueError, match="window_size 24.*--window-size is 12"):
        prep(hb, window_size=12)
    with pytest.raises(ValueError, match="TieWindowBatch holds TIE events"):
        prep(store.plan(w, 1000, 1))
    from medical_tri_modal_pilot_amd.builder.data import collate_packed
    pats = M.synthetic_patients()
    plan = store.plan(w, 1000, 1)
    pb = collate_packed([(M.reference_window(pats, M.FMIN, M.FMAX, p, k, L, 1000, 1)[0], s, tt)
                         for (p, k, L), s, tt in zip(w.tolist(), plan.static.numpy(), plan.txt_time.tolist())])
    with pytest.raises(ValueError, match="PackedTieBatch holds TIE events"):
        prep(pb)
