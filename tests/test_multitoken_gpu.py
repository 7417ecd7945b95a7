"""-m gpu: the building blocks of the multi-token bottleneck encoder (reference mbt_encoder.py:9-193) on the GPU -- the multi-set
bottleneck exchange against a float64 model of :183-191, the masked BCE over four logit rows against the reference's boolean-index
form, and one encoder layer with a prefix mask through ops.EncoderLayerFn against autograd over the torch chain of the oracle."""
import math

import pytest
import torch

import filler
from oracle import tri_mbt_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

BOTTLENECKS_MAP = [[0, 1, 2], [0, 1, 3], [0, 2, 3]]                     # mbt_encoder.py:63
B_OUT_MEAN_MAP = {0: [[0, 1, 2], [0, 1], [0, 2], [0]], 1: [[0, 1], [0, 1], [0], [0]],      # mbt_encoder.py:98-101
                  2: [[0, 1], [0], [0, 1], [0]], 3: [[0, 1], [0], [1], [0]]}


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


@pytest.fixture(scope="module")
def ops():
    from medical_tri_modal_pilot_amd import ops as _ops
    return _ops


def exchange_model(zs, missing):
    """mbt_encoder.py:178-191 on the three stream buffers [B, n_m, 256] (float64): the new prefixes, written back per holder"""
    B = zs[0].shape[0]
    outs = [[], [], [], []]
    for m in range(3):
        for i in range(3):
            outs[BOTTLENECKS_MAP[m][i]].append(zs[m][:, 4 * i:4 * i + 4])
    new = []
    for b_idx, b_out in enumerate(outs):
        st = torch.stack(b_out)
        means = torch.stack([torch.mean(st[torch.tensor(i)], dim=0) for i in B_OUT_MEAN_MAP[b_idx]])
        new.append(means[missing, torch.arange(B)])
    res = []
    for m in range(3):
        res.append(torch.cat([new[s] for s in BOTTLENECKS_MAP[m]] + [zs[m][:, 12:]], dim=1))
    return res


@pytest.mark.parametrize("dt,tol", [(torch.float32, 1e-6), (torch.bfloat16, 1e-2)])
def test_exchange_multi_fwd_bwd(ops, dt, tol):
    g = torch.Generator().manual_seed(17)
    B, ns = 5, [12 + 9, 12, 12 + 30]
    missing = torch.tensor([0, 1, 2, 3, 1])
    zs = [torch.randn(B, n, 256, generator=g).to(dt).float() for n in ns]
    ws = [torch.randn(B, n, 256, generator=g).to(dt).float() for n in ns]
    zr = [z.double().requires_grad_() for z in zs]
    ref = exchange_model(zr, missing)
    sum((r * w.double()).sum() for r, w in zip(ref, ws)).backward()
    zd = [z.to(DEV, dt).requires_grad_() for z in zs]
    out = ops.BottleneckExchangeMultiFn.apply(*zd, missing.to(DEV))
    sum((o.float() * w.to(DEV)).sum() for o, w in zip(out, ws)).backward()
    for m in range(3):
        e, eg = _rel(out[m].float(), ref[m]), _rel(zd[m].grad.float(), zr[m].grad)
        print(f"exchange_multi[{str(dt)[6:]}] stream {m}: fwd {e:.2e} bwd {eg:.2e}")
        assert e <= tol and eg <= tol, (m, e, eg)
        assert torch.equal(out[m][:, 12:], zd[m][:, 12:])              # the token rows are not touched


def test_bce_rows_masked_mean(ops):
    crit = torch.nn.BCEWithLogitsLoss()
    table = torch.tensor([[0., 0., 0., 0.], [1., 0., 1., 0.], [1., 1., 0., 0.], [1., 1., 1., 0.]])      # trainer.py:79-83
    g = torch.Generator().manual_seed(2)
    cases = [(1, [2]), (4, [0, 1, 2, 3]), (64, None), (6, [3, 3, 2, 3, 2, 2])]      # the last: rows 0 and 1 have no selected sample
    for B, ids in cases:
        mnum = torch.randint(0, 4, (B,), generator=g) if ids is None else torch.tensor(ids)
        o = (torch.randn(4, B, generator=g) * 3).requires_grad_()
        y = (torch.rand(B, generator=g) > 0.5).float()
        miss = table[mnum].permute(1, 0).reshape(-1)
        ref = crit(o.reshape(-1)[miss == 0], y.unsqueeze(0).repeat(4, 1).reshape(-1)[miss == 0])
        (gref,) = torch.autograd.grad(ref * 1.7, o)
        od = o.detach().to(DEV).requires_grad_()
        loss = ops.bce_rows_masked_mean(crit, od, y.to(DEV), mnum.to(DEV))
        (gd,) = torch.autograd.grad(loss * 1.7, od)
        assert abs(float(loss) - float(ref)) <= 1e-6 * max(1.0, abs(float(ref))), (B, float(loss), float(ref))
        assert float((gd.cpu() - gref).abs().max()) <= 1e-6 * float(gref.abs().max()) + 1e-9, B
        assert torch.equal(gd.cpu() == 0, gref == 0)                  # exactly zero outside the selected pairs
        # the boolean-index form on the same device (any other criterion takes it)
        alt = ops.bce_rows_masked_mean(torch.nn.BCEWithLogitsLoss(reduction="sum"), od, y.to(DEV), mnum.to(DEV))
        n_sel = int((miss == 0).sum())
        assert abs(float(alt) / n_sel - float(ref)) <= 1e-5 * max(1.0, abs(float(ref)))


@pytest.mark.parametrize("dt,tol,gtol,ptol", [(torch.float32, 1e-4, 1e-4, 1e-4), (torch.bfloat16, 3e-2, 4e-2, 0.14)])
def test_encoder_layer_with_prefix_mask(ops, dt, tol, gtol, ptol):
    """ops.EncoderLayerFn with qk_mask against autograd over the oracle's layer (float64) with the full boolean mask (two
    workgroups of queries in the backward: N 150).  Bounds: fp32 1e-4 everywhere (README "Parity"); bf16 the attention test's 3e-2
    / 4e-2 for y / dx, and for the PARAMETER gradients the per-tensor gate the benchmarked model's bf16 step is held to
    (tests/test_gpu_parity.py BF16_STEP_GATES grad_norm / grad_digest = 0.14).  That gate is what the number format asks for here:
    the float64 layer with nothing changed but every tensor the bf16 build keeps in bf16 rounded to bf16 (values forward, gradients
    backward, weights as bf16 copies) is already 5.0e-2 away from the exact one on d gamma of the FFN LayerNorm, 7.1e-2 on d b1 and
    1.2e-1 on d W1 for these inputs (sums over 450 rows of products of rounded factors with mixed signs).
    The gradient of the key projection's BIAS is zero in exact arithmetic (a constant added to every key's score leaves the
    softmax unchanged), so it has no scale of its own: it is held to the query bias gradient's scale."""
    from medical_tri_modal_pilot_amd.builder.models.src.transformer.encoder import TransformerEncoderLayer
    from tests.test_attn_prefix_gpu import MASKS, words
    mask = MASKS["v16"]
    lay = TransformerEncoderLayer(256, 4, 1024, 0.0)
    lay.load_state_dict({k: filler.fill_tensor("mt." + k, v) for k, v in lay.state_dict().items()})
    g = torch.Generator().manual_seed(9)
    B, N = 3, 150
    x = torch.randn(B, N, 256, generator=g).to(dt).float()
    w = torch.randn(B, N, 256, generator=g).to(dt).float()
    kv = torch.tensor([150, 16, 77])
    sd = {"l." + k: v.detach().double().requires_grad_() for k, v in lay.state_dict().items()}
    full = O.key_pad_mask(N, kv).clone()
    full[:, :16, :16] = mask
    xr = x.double().requires_grad_()
    (O.encoder_layer(sd, "l", xr, full, 4) * w.double()).sum().backward()
    y_ref = O.encoder_layer(sd, "l", xr, full, 4).detach()
    lay = lay.to(DEV)
    xd = x.to(DEV, dt).requires_grad_()
    y = ops.EncoderLayerFn.apply(xd, kv.to(DEV, torch.int32), *lay.param_list(), lay._fused_weights(dt), 0.0, (0, 0), words(mask))
    (y.float() * w.to(DEV)).sum().backward()
    errs = {"y": (_rel(y.float(), y_ref), tol), "dx": (_rel(xd.grad.float(), xr.grad), gtol)}
    for name, p in lay.named_parameters():
        if name == "self_attention.key_proj.linear.bias":
            scale = float(sd["l.self_attention.query_proj.linear.bias"].grad.abs().max())
            errs["d" + name] = (float(p.grad.abs().max()) / scale, ptol)
            continue
        errs["d" + name] = (_rel(p.grad, sd["l." + name].grad.reshape(p.shape)), ptol)
    for k, (e, bound) in errs.items():
        print(f"layer+mask[{str(dt)[6:]}] {k}: {e:.2e}")
        assert math.isfinite(e) and e <= bound, (k, e)
    # and the mask is what made the difference: the plain layer on the same inputs is not the same function
    y0 = ops.EncoderLayerFn.apply(xd.detach(), kv.to(DEV, torch.int32), *lay.param_list(), lay._fused_weights(dt), 0.0, (0, 0))
    assert not torch.equal(y0[:, :16], y.detach()[:, :16]) and torch.equal(y0[:, 16:], y.detach()[:, 16:])


# ------------------------------------------------------------------ the two models against the goldens of the real classes
MODELS = [("tri_mbt_vmultivslt", "tri_vmultivslt"), ("tri_mbt_vmulti2", "tri_vmulti2")]
BF16_LOSS, BF16_TEST_LOSS = 3.5e-3, 1.8e-3          # tests/test_gpu_parity.py BF16_STEP_GATES


@pytest.mark.parametrize("name,tag", MODELS)
def test_model_step_vs_golden(name, tag):
    """fp32 build: logits [4, B], the masked training loss and every gradient digest against the reference's class driven by its
    own trainer; the tensors without a gradient there have none here"""
    import numpy as np
    from medical_tri_modal_pilot_amd import ops
    from tests.test_noshnoavgtr_gpu import G, _build, _digest, _forward
    Gd = G(tag + "_step")
    a, model = _build(name, tag)
    bt = filler.make_batch(int(Gd["seed"]), int(Gd["B"]), int(Gd["T"]))
    mnum = torch.from_numpy(Gd["missing_num"])
    out, o2, o3 = _forward(model, bt, mnum)
    assert o2 is None and o3 is None and tuple(out.shape) == tuple(Gd["logits"].shape) == (4, 4)
    e = _rel(out, torch.from_numpy(Gd["logits"]))
    print(name, "logits", e)
    assert e <= 1e-4
    loss = ops.bce_rows_masked_mean(torch.nn.BCEWithLogitsLoss(), out, bt["y"].float().to(DEV), mnum.to(DEV))
    print(name, "loss", abs(float(loss.detach()) - float(Gd["loss"])))
    assert abs(float(loss) - float(Gd["loss"])) <= 1e-5
    torch.autograd.backward([loss], [ops.unit_grad(loss)])
    prm = dict(model.named_parameters())
    med = float(np.median(Gd["grad_digest"][:, 0]))
    worst, n_checked = 0.0, 0
    for n_, gd in zip((str(s) for s in Gd["grad_names"]), Gd["grad_digest"]):
        assert prm[n_].grad is not None, n_
        if gd[0] < 1e-4 * med:
            assert float(_digest(prm[n_].grad)[0]) < 1e-3 * med, n_
            continue
        e = _rel(_digest(prm[n_].grad), torch.from_numpy(gd))
        assert e <= 1e-4, (n_, e)
        worst, n_checked = max(worst, e), n_checked + 1
    print(name, "worst gradient digest", worst, "tensors", n_checked)
    assert n_checked >= 0.8 * len(Gd["grad_names"])
    for n_ in (str(s) for s in Gd["nograd_names"] if str(s)):
        assert prm[n_].grad is None, n_


@pytest.mark.parametrize("name,tag", MODELS)
def test_trainer_flows_and_validate_vs_golden(name, tag):
    """missing_trainer (--hip-graph 0): the test flow's loss and probabilities, validate() on the same batch, the train flow's loss"""
    from medical_tri_modal_pilot_amd.builder.trainer import get_trainer, validate
    from medical_tri_modal_pilot_amd.builder.utils.device_evaluator import DeviceEvaluator
    from tests.test_noshnoavgtr_gpu import G, _Logger, _build, _optimizer, _trainer_kw
    Gd = G(tag + "_step")
    a, model = _build(name, tag)
    bt = filler.make_batch(int(Gd["seed"]), int(Gd["B"]), int(Gd["T"]))
    lg = _Logger()
    model.eval()
    kw = _trainer_kw(a, model, bt, lg)
    _, test_loss = get_trainer(iteration=1, input_lengths=bt["input_lengths"].clone(), txt_lengths=bt["txt_lengths"].clone(),
                               flow_type="test", **kw)
    (tgt, prob), = lg.evaluator.calls
    print(name, "test loss", abs(test_loss - float(Gd["test_loss"])), "prob", _rel(prob, torch.from_numpy(Gd["test_prob"])))
    assert abs(test_loss - float(Gd["test_loss"])) <= 1e-5
    assert tuple(prob.shape) == (4,) and _rel(prob, torch.from_numpy(Gd["test_prob"])) <= 1e-4
    ev = DeviceEvaluator(a, DEV, 16, keep_logits=True)
    batch = (bt["x"], torch.stack([bt["gen"], bt["age"]], 1), bt["y"], bt["input_lengths"], bt["img"], bt["img_time"], bt["txt"],
             bt["txt_lengths"], bt["txt_time"], bt["missing"], None, None)
    res = validate(a, model, [batch], torch.device(DEV), torch.nn.BCEWithLogitsLoss(), ev)
    pred, vt, _ = ev.predictions()
    assert res["n"] == 4 and abs(res["loss"] - test_loss) <= 1e-6
    assert _rel(pred, prob.reshape(-1)) <= 1e-6 and torch.equal(vt.cpu().float(), bt["y"].float())
    model.train()
    model.img_encoder.eval()
    opt, sched = _optimizer(a, model)
    kw = _trainer_kw(a, model, bt, _Logger(), opt, sched)
    _, train_loss = get_trainer(iteration=1, input_lengths=bt["input_lengths"].clone(), txt_lengths=bt["txt_lengths"].clone(),
                                flow_type="train", **kw)
    print(name, "train loss", abs(train_loss - float(Gd["loss"])))
    assert abs(train_loss - float(Gd["loss"])) <= 1e-5


@pytest.mark.parametrize("name,tag", MODELS)
def test_bf16_build_is_finite_and_close(name, tag):
    """the bf16 build (grouped launches of the three streams): logits and every gradient finite, both losses within the bounds the
    benchmarked model's bf16 step is held to"""
    from medical_tri_modal_pilot_amd import ops
    from tests.test_noshnoavgtr_gpu import G, _build, _forward
    Gd = G(tag + "_step")
    a, model = _build(name, tag, "bf16")
    bt = filler.make_batch(int(Gd["seed"]), int(Gd["B"]), int(Gd["T"]))
    mnum = torch.from_numpy(Gd["missing_num"])
    out, _, _ = _forward(model, bt, mnum)
    loss = ops.bce_rows_masked_mean(torch.nn.BCEWithLogitsLoss(), out.float(), bt["y"].float().to(DEV), mnum.to(DEV))
    torch.autograd.backward([loss], [ops.unit_grad(loss)])
    o = out.float().reshape(4, -1)
    test_loss = torch.nn.BCEWithLogitsLoss()(o[mnum.to(DEV), torch.arange(4, device=DEV)], bt["y"].float().to(DEV))
    print(name, "bf16 loss", abs(float(loss) - float(Gd["loss"])), "test loss", abs(float(test_loss) - float(Gd["test_loss"])))
    assert torch.isfinite(out).all()
    names = set(str(s) for s in Gd["grad_names"])
    for n_, p in model.named_parameters():
        assert (p.grad is not None) == (n_ in names), n_
        assert p.grad is None or torch.isfinite(p.grad).all(), n_
    assert abs(float(loss) - float(Gd["loss"])) <= BF16_LOSS and abs(float(test_loss) - float(Gd["test_loss"])) <= BF16_TEST_LOSS
