"""CPU: tests/head_model.py can be trusted.  The written-out float64 chain equals the real torch modules in float64, every entry of
SEEDS keeps the ReLU gates clear of zero, the three cancelling gradients are zero to round-off where they must be, and the metric
with bound(e_torch) catches the mistakes a head kernel could make -- each one seeded into the float64 model at the batch size where
a kernel would make it."""
import pytest
import torch
import torch.nn as nn

from tests import head_model as H
from tests import row_kernels_model as R

F32, F64, BF16 = H.F32, H.F64, H.BF16
TRAIN_BATCHES = [B for B in H.BATCHES if B > 1]


def _torch_chain(inp, training):
    """the modules the kernels replace, in float64, on the same tensors: outputs, gradients by autograd, running statistics"""
    dm = nn.Sequential(nn.Linear(2, 256), nn.LayerNorm(256, eps=H.LN_EPS), nn.ReLU()).double()
    ln = nn.LayerNorm(256, eps=H.LN_EPS).double()
    fc = nn.Sequential(nn.Linear(512, 256), nn.BatchNorm1d(256, eps=H.BN_EPS, momentum=H.MOMENTUM), nn.ReLU(), nn.Linear(256, 1)).double()
    prm = [dm[0].weight, dm[0].bias, dm[1].weight, dm[1].bias, ln.weight, ln.bias, fc[0].weight, fc[0].bias, fc[1].weight, fc[1].bias,
           fc[3].weight, fc[3].bias]
    with torch.no_grad():
        for p, v in zip(prm, inp["params"]):
            p.copy_(v.double())
        fc[1].running_mean.copy_(inp["run_mean"].double()), fc[1].running_var.copy_(inp["run_var"].double())
    for m in (dm, ln, fc):
        m.train(training)
    cls = inp["cls"].double().requires_grad_()
    o = fc(torch.cat([ln(cls), dm(torch.stack([inp["age"], inp["gender"]], 1).double())], 1))
    grads = torch.autograd.grad((o * inp["w"].double()).sum(), [cls] + prm)
    out = dict(o=o.detach(), dcls=grads[0], run_mean=fc[1].running_mean.clone(), run_var=fc[1].running_var.clone())
    out.update(zip(H.GRAD_NAMES, grads[1:]))
    return out, int(fc[1].num_batches_tracked)


@pytest.mark.parametrize("cls_dt", [F32, BF16], ids=R.dt_name)
@pytest.mark.parametrize("B,training", [(B, tr) for B in H.BATCHES for tr in H.modes(B)])
def test_model_equals_torch_modules_in_float64(B, training, cls_dt):
    c = H.case(B, cls_dt, training)
    tor, nbt = _torch_chain(c["inp"], training)
    assert nbt == int(training)
    for name in H.CHECKED:
        e = H.err_of(name, tor[name], c["ref"], training)
        assert e <= 1e-12, (name, e)
    if not training:
        for k in ("run_mean", "run_var"):
            assert torch.equal(c["ref"][k], c["inp"][k].double()), k


def test_inputs_are_fp32_and_cls_rows_hold_their_type():
    for dt in (F32, BF16):
        inp = H.head_inputs(65, dt, 0)
        assert all(t.dtype == F32 for t in [inp[k] for k in ("cls", "age", "gender", "w", "run_mean", "run_var")] + inp["params"])
        assert torch.equal(inp["cls"].to(dt).float(), inp["cls"])
    a, b = H.head_inputs(65, F32, 0), H.head_inputs(65, BF16, 0)
    assert all(torch.equal(p, q) for p, q in zip(a["params"], b["params"])) and torch.equal(a["w"], b["w"])
    assert len({H.LN_EPS, H.BN_EPS, H.MOMENTUM, 1.0 - H.MOMENTUM}) == 4


def test_every_seed_keeps_the_gates_clear_of_zero():
    assert set(H.SEEDS) == set(H.BATCHES)
    for B in H.BATCHES:
        for dt in (F32, BF16):
            for tr in H.modes(B):
                assert H.case(B, dt, tr)["ref"]["margin"] > H.GATE_MARGIN, (B, dt, tr)


def test_seeds_are_the_first_that_qualify():
    assert H.find_seeds() == H.SEEDS


@pytest.mark.parametrize("cls_dt", [F32, BF16], ids=R.dt_name)
@pytest.mark.parametrize("B", TRAIN_BATCHES)
def test_cancelling_gradients_are_zero_to_round_off(B, cls_dt):
    """training mode: db1 and dln_b in every column, ddemo_be in the columns whose demo gate is the same for every sample"""
    ref = H.case(B, cls_dt, True)["ref"]
    const = ref["gate_const"]
    assert bool((ref["db1"].abs() <= 1e-12 * ref["A_db1"]).all())
    assert bool((ref["dln_b"].abs() <= 1e-12 * ref["A_dln_b"]).all())
    assert bool((ref["ddemo_be"].abs() <= 1e-12 * ref["A_ddemo_be"])[const].all())
    # (age in [0,1) and gender in {0,1} move a normalised demo value little: with these gate weights most demo columns, often all,
    #  keep one gate for the whole batch -- ddemo_be is then a cancelling sum in every live column)
    assert int(const.sum()) > 128 and int((const & (ref["A_ddemo_be"] > 0)).sum()) > 64
    if not bool(const.all()):                                     # a column whose gate depends on the sample does NOT cancel
        assert float((ref["ddemo_be"].abs() / ref["A_ddemo_be"].clamp_min(1e-300))[~const].max()) > 1e-3
    if B >= 63:
        assert float(ref["A_dln_b"].min()) > 0 and int((ref["A_db1"] > 0).sum()) > 64      # (a feature with y < 0 in every row has dh = 0)
    # in eval mode nothing cancels: the ordinary metric applies there
    ev = H.case(B, cls_dt, False)["ref"]
    assert float(ev["db1"].abs().max()) > 1e-3 and float(ev["dln_b"].abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------ seeded faults
def _fault(B, training, fault, cls_dt=F32, **kw):
    """{name: (error of the faulty float64 model, bound of the sound one)}"""
    inp = H.head_inputs(B, cls_dt, H.SEEDS[B])
    ref, et = H.e_torch_of(inp, training, **kw)
    bad = H.head_chain(inp, training, ft=F64, fault=fault, **kw)
    return {k: (H.err_of(k, bad[k], ref, training), R.bound(et[k])) for k in H.CHECKED}


def _caught(res, names):
    for k in names:
        e, b = res[k]
        assert e > b, f"{k}: the fault moves it by {e:.3e}, inside the bound {b:.3e}"


def _untouched(res, names):
    for k in names:
        assert res[k][0] == 0.0, k


ROW_SUMS = ["db1", "dln_g", "dln_b", "ddemo_g", "ddemo_be", "ddemo_w", "ddemo_b"]


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("B", [65, 129, 255])
def test_fault_last_row_left_out_of_the_row_sums(B, training):
    res = _fault(B, training, "drop_last_row")
    _caught(res, ROW_SUMS)
    _untouched(res, [k for k in H.CHECKED if k not in ROW_SUMS])


@pytest.mark.parametrize("B", [63, 127, 255])
def test_fault_rows_past_B_counted_into_the_batch_mean(B):
    """(the variance about a mean that is off by b1 / B moves by its square only: running_var does not show this one)"""
    _caught(_fault(B, True, "pad_rows_in_mean"), ["o", "run_mean", "dcls", "dw1", "dbn_g"])


@pytest.mark.parametrize("B", [2, 5, 256])
def test_fault_unbiased_variance_used_for_normalisation(B):
    res = _fault(B, True, "unbiased_norm")
    _caught(res, ["o", "dw2"] + (["dcls", "dw1", "dbn_g"] if B > 3 else []))
    _untouched(res, ["run_mean", "run_var"])


@pytest.mark.parametrize("B", [2, 3, 5, 256])
def test_fault_biased_variance_written_to_running_var(B):
    res = _fault(B, True, "biased_running_var")
    _caught(res, ["run_var"])
    _untouched(res, [k for k in H.CHECKED if k != "run_var"])


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("B", [5, 65])
def test_fault_bn_eps_and_ln_eps_swapped(B, training):
    _caught(_fault(B, training, "eps_swapped"), ["o", "dcls", "dw1", "dbn_g", "dw2"])


@pytest.mark.parametrize("B", [2, 65])
def test_fault_momentum_applied_to_the_wrong_term(B):
    res = _fault(B, True, "momentum_swapped")
    _caught(res, ["run_mean", "run_var"])
    _untouched(res, [k for k in H.CHECKED if k not in ("run_mean", "run_var")])


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("B", [5, 65, 256])
def test_fault_gate_taken_from_y_ge_0(B, training):
    """one BatchNorm output is made exactly 0 (through fc_list.1.bias, in the float64 and in the fp32 chain alike): ReLU'(0) = 0"""
    inp = H.head_inputs(B, F32, H.SEEDS[B])
    zg = (B - 1, int(inp["params"][10].abs().argmax()))
    for ft in (F64, F32):
        sound = H.head_chain(inp, training, ft=ft, zero_gate=zg)
        assert sound["margin"] == 0.0
    _caught(_fault(B, training, "gate_ge", zero_gate=zg), ["dbn_b", "dbn_g", "dw1", "dcls"])


# ------------------------------------------------------------------------------------------ the BCE model
@pytest.mark.parametrize("planted", [False, True], ids=["randn", "planted"])
@pytest.mark.parametrize("n", H.BCE_N)
def test_bce_model_equals_torch_in_float64(n, planted):
    c = H.bce_case(n, planted)
    o = c["o"].double().requires_grad_()
    loss = nn.functional.binary_cross_entropy_with_logits(o, c["t"].double())
    (d,) = torch.autograd.grad(loss, o)
    assert R.err(c["ref"]["loss"], loss.detach().reshape(1)) <= 1e-12
    assert float((c["ref"]["dlogit"] - d).abs().max()) <= 1e-16 / n * 8                # (absolute: torch's sigmoid(104) - 1 is 0)
    assert bool(torch.isfinite(c["ref"]["dlogit"]).all()) and float(c["ref"]["dlogit"].abs().max()) <= 1.0 / n
    if planted and n >= 2 * len(H.BCE_PLANTED):
        assert c["o"][:18].tolist() == [v for v in H.BCE_PLANTED for _ in (0, 1)] and c["t"][:18].tolist() == [0.0, 1.0] * 9
