"""The device-side evaluator on the GPU (csrc/evaluator.hip through builder/utils/device_evaluator.DeviceEvaluator) against the
numpy model (tests/evaluator_model.py).  Everything that is integer counting followed by one correctly rounded float64 division
(n, positives, AUROC, both F1 values) is compared bit for bit; AP, a float64 sum in another order than the model's, within the
bound of a reordered sum; the logits-mode predictions within one float32 ulp (the device's float64 exp is within a few float64
ulps of numpy's, so the single rounding to float32 can differ only next to a rounding boundary)."""
import math

import numpy as np
import pytest
import torch

from tests import evaluator_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from medical_tri_modal_pilot_amd import ops as _ops
    return _ops


def _args(**kw):
    from medical_tri_modal_pilot_amd.control.config import parse_args
    a = parse_args(["--input-types", "vslt_img_txt", "--model", "tri_mbt_vsltcls", "--modality-inclusion",
                    "train-missing_test-missing", "--lr-init", "1e-5", "--batch-size", "4"])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _evaluator(capacity, **kw):
    from medical_tri_modal_pilot_amd.builder.utils.device_evaluator import DeviceEvaluator
    return DeviceEvaluator(_args(), DEV, capacity, **kw)


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64).tolist()


def _ulps32(a, b):
    """distance in float32 steps between two arrays of finite non-negative floats"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ---------------------------------------------------------------------------------------------------------------- append
LOGITS = [np.float32(v) for v in (0.0, -0.0, 100.0, -100.0, np.inf, -np.inf, np.nan, 0.3, -2.5, 17.0, -17.0, 88.0, -88.0, -104.0, 1e-8)]


def _logit_batch(g, n):
    x = (6.0 * g.standard_normal(n)).astype(np.float32)
    x[:min(n, len(LOGITS))] = LOGITS[:min(n, len(LOGITS))]
    t = (g.random(n) < 0.4).astype(np.float32)
    t[-1] = 2.0                                                  # the target is stored as t != 0
    return x, t


def test_append_against_the_model():
    g = np.random.default_rng(11)
    ev, st = _evaluator(1000, keep_logits=True), M.State(1000, keep_logits=True)
    losses = [np.float32(0.7310586), np.float32(0.1234567), np.float32(1e-3)]
    host_sum = np.float64(0.0)
    for n, loss in zip((64, 257, 5), losses):
        x, t = _logit_batch(g, n)
        ev.add_logits(torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV), torch.tensor(loss, device=DEV))
        st.append(x, t, 0, loss)
        host_sum = host_sum + np.float64(loss)                   # the same float64 additions in the same order
    probs = np.array([-0.0, np.nan, np.inf, -np.inf, 1.5, -0.25, 0.5, 1e-45, 0.0099999, 0.01], np.float32)
    pt = np.array([1, 0, 1, 0, 0, 1, 1, 0, 1, 0], np.float32)
    ev.add_batch(torch.from_numpy(pt).to(DEV), torch.from_numpy(probs).to(DEV))
    st.append(probs, pt, 1)
    pred, tgt, logit = (a.cpu().numpy() for a in ev.predictions())
    n = 64 + 257 + 5
    assert pred.shape == tgt.shape == logit.shape == (n + 10,) and ev.appended == n + 10
    assert ev.ctr.cpu().tolist() == st.ctr.tolist() == [n + 10, 3, 0, 0]
    assert np.array_equal(tgt, st.tgt[:n + 10])
    assert np.array_equal(logit[:n].view(np.uint32), st.logit[:n].view(np.uint32))              # raw logits, NaN and -0.0 bits kept
    assert np.array_equal(pred[n:].view(np.uint32), st.pred[n:n + 10].view(np.uint32))           # probabilities mode: bit-exact
    assert pred[n:].view(np.uint32)[0] == 0 and pred[n + 2] == M.FLT_MAX and pred[n + 3] == -M.FLT_MAX and pred[n + 1] == 0
    assert np.all(np.isfinite(pred)) and np.all(pred[:n] >= 0) and not np.signbit(pred[:n]).any()
    d = _ulps32(pred[:n], st.pred[:n])
    print(f"append: logits-mode predictions differ from the model by at most {int(d.max())} float32 ulp ({int((d > 0).sum())} of {n})")
    assert d.max() <= 1
    assert float(ev.loss_sum.cpu()[0]) == float(host_sum) == float(st.loss_sum)
    m = ev.metrics()
    assert m["loss"] == float(host_sum / np.float64(3)) and m["n"] == n + 10 and m["n_pos"] == int(st.tgt.sum()) and m["status"] == 0
    ev.reset()
    assert ev._state.cpu().tolist() == [0] * 6 and ev.appended == 0 and ev.predictions()[0].numel() == 0
    m0 = ev.metrics()
    assert (m0["auroc"], m0["f1"], m0["best_f1"], m0["n"], m0["n_pos"], m0["status"]) == (0.0, 0.0, 0.0, 0, 0, 0)
    assert math.isnan(m0["ap"]) and math.isnan(m0["loss"])
    with pytest.raises(ValueError, match="is on cpu"):
        ev.add_logits(torch.zeros(4), torch.zeros(4, device=DEV))
    with pytest.raises(ValueError, match="is on cpu"):
        ev.add_batch(torch.zeros(4), torch.zeros(4, device=DEV))


def test_append_past_the_capacity_drops_and_writes_nothing_out_of_range():
    g = np.random.default_rng(12)
    ev, st = _evaluator(70, keep_logits=True), M.State(70, keep_logits=True)
    guard = 4096
    fbuf = [torch.full((70 + guard,), 123.0, dtype=torch.float32, device=DEV) for _ in range(2)]
    bbuf = torch.full((70 + guard,), 77, dtype=torch.uint8, device=DEV)
    ev.pred, ev.logit, ev.tgt = fbuf[0][:70], fbuf[1][:70], bbuf[:70]            # the state, with a guard region behind it
    for _ in range(2):
        x, t = _logit_batch(g, 64)
        ev.add_logits(torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV), torch.tensor(0.5, device=DEV))
        st.append(x, t, 0, np.float32(0.5))
    assert ev.ctr.cpu().tolist() == st.ctr.tolist() == [70, 2, 58, 0]
    for b in fbuf:
        assert bool((b[70:] == 123.0).all())
    assert bool((bbuf[70:] == 77).all())
    pred, tgt, logit = (a.cpu().numpy() for a in ev.predictions())
    assert pred.shape == (70,) and np.array_equal(tgt, st.tgt) and _ulps32(pred, st.pred).max() <= 1
    assert np.array_equal(logit.view(np.uint32), st.logit.view(np.uint32))
    with pytest.raises(RuntimeError, match="capacity 70 was too small.*128 predictions were added, 58 dropped"):
        ev.performance_metric()
    with pytest.raises(RuntimeError, match="58 dropped"):
        ev.metrics()
    ev.reset()
    ev.add_batch(torch.ones(3, device=DEV), torch.tensor([0.9, 0.8, 0.7], device=DEV))
    assert ev.ctr.cpu().tolist() == [3, 0, 0, 0] and ev.metrics()["n"] == 3


# ---------------------------------------------------------------------------------------------------------------- metrics
def _sizes(ops):
    T = ops.EVAL_SORT_TILE
    return [1, 2, 255, 256, 257, T - 1, T, T + 1, 3 * T + 17, 70001, 1100003]


def _run(ev, pred, tgt):
    """the metrics kernel on a state filled directly: (pred, tgt) need not come from an append"""
    n = pred.size
    ev.reset()
    ev.pred[:n].copy_(torch.from_numpy(pred))
    ev.tgt[:n].copy_(torch.from_numpy(tgt))
    ev.ctr[0] = n
    ev.appended = n
    ev.metrics()
    return ev._out.cpu().numpy().copy()


@pytest.fixture(scope="module")
def big_evaluator():
    return _evaluator(1100003)


@pytest.mark.parametrize("kind", M.KINDS)
@pytest.mark.parametrize("size_index", range(11))
def test_metrics_against_the_model(ops, big_evaluator, kind, size_index):
    from medical_tri_modal_pilot_amd.builder.utils import metrics as R
    n = _sizes(ops)[size_index]
    pred, tgt = M.case(kind, n)
    want = M.metrics(pred, tgt, stored=n)
    got = _run(big_evaluator, pred, tgt)
    print(f"metrics[{kind}, n {n}]: device {got.tolist()} model {want}")
    names = ("auroc", "ap", "f1", "best_f1", "loss", "n", "n_pos", "status")
    for i in (0, 2, 3, 5, 6, 7):
        assert _bits(got[i]) == _bits(want[i]), (names[i], got[i], want[i])
    assert math.isnan(got[4])                                    # no batch carried a loss
    if math.isnan(want[1]):
        assert math.isnan(got[1]) and int(tgt.sum()) == 0
    else:
        # a reordered float64 sum of n terms of size <= 1, three roundings each: 3 n 2^-53, 1e-10 at the largest size
        assert abs(got[1] - want[1]) <= 1e-10, (got[1], want[1])
    # twice, then shuffled: all eight outputs bit-identical
    again = _run(big_evaluator, pred, tgt)
    perm = np.random.default_rng(n).permutation(n)
    shuffled = _run(big_evaluator, pred[perm], tgt[perm])
    assert got.view(np.uint64).tolist() == again.view(np.uint64).tolist() == shuffled.view(np.uint64).tolist()
    # the package's float32 metrics on the same device tensors: 1e-6
    tp, tt = big_evaluator.pred[:n], big_evaluator.tgt[:n]
    for i, ref in ((0, R.binary_auroc(tp, tt)), (1, R.binary_average_precision(tp, tt)), (2, R.binary_f1(tp, tt, 0.01)),
                   (3, R.best_f1_over_thresholds(tp, tt))):
        ref = float(ref)
        assert (math.isnan(ref) and math.isnan(got[i])) or abs(got[i] - ref) <= 1e-6, (names[i], got[i], ref)


def test_status_names_a_count_that_differs(ops):
    ev = _evaluator(100)
    ev.add_batch(torch.ones(10, device=DEV), torch.rand(10, device=DEV))
    ev.ctr[0] = 9                                                # the state changed behind the evaluator
    with pytest.raises(RuntimeError, match="another number of predictions than the 10 the host counted"):
        ev.metrics()


def test_performance_metric_equals_the_evaluator_of_metrics_py(ops):
    """DeviceEvaluator alone in the unchanged test flow: add_batch(y_true, sigmoid) per batch, performance_metric() at the end"""
    from medical_tri_modal_pilot_amd.builder.utils.metrics import Evaluator
    g = torch.Generator().manual_seed(3)
    a, b = Evaluator(_args()), _evaluator(64)
    for n in (8, 8, 8, 5):
        t = (torch.rand(n, generator=g) < 0.4).float().to(DEV)
        p = torch.sigmoid(2.0 * torch.randn(n, generator=g)).to(DEV)
        a.add_batch(t, p)
        b.add_batch(t, p)
    want, got = a.performance_metric(), b.performance_metric()
    print("performance_metric: Evaluator", want, "DeviceEvaluator", got)
    assert len(got) == 3 and [float(v) for v in got] == [float(v) for v in want] and b.best_auc == a.best_auc == 0
