"""Plain-numpy model of csrc/evaluator.hip (the device-side evaluator): the append's value rules, the sort key, the stable LSD
radix sort, the tie groups, the integer AUROC numerator, AP, the F1 counts.  Vectorised: the largest GPU case (1.1 M values)
takes a fraction of a second here.  Integer quantities are exact (int64 / Python integers); AP is a float64 sum whose ORDER is
numpy's, not the kernel's -- the tests compare it within the bound of a reordered sum and everything else bit for bit."""
import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)
SIZES = (1, 2, 3, 17, 255, 256, 257, 1000, 4099, 70001)
KINDS = ("continuous", "ties20", "all_equal", "all_positive", "all_negative", "wide")


# ------------------------------------------------------------------------------------------------------------- the append
def settle(v):
    """torch.nan_to_num on float32 (NaN -> 0, +inf -> FLT_MAX, -inf -> -FLT_MAX), then -0.0 -> +0.0"""
    v = np.array(v, np.float32, copy=True).reshape(-1)
    v[np.isnan(v)] = 0.0
    v[np.isposinf(v)] = FLT_MAX
    v[np.isneginf(v)] = -FLT_MAX
    v[v == 0] = 0.0                      # -0.0 == 0 is true: both zeros become +0.0
    return v


def sigmoid_f32(x):
    """1 / (1 + exp(-x)) evaluated in float64, rounded ONCE to float32"""
    with np.errstate(over="ignore", invalid="ignore"):
        return (1.0 / (1.0 + np.exp(-np.asarray(x, np.float32).reshape(-1).astype(np.float64)))).astype(np.float32)


class State:
    """pred / tgt / logit / ctr / loss_sum as builder/utils/device_evaluator.py holds them"""

    def __init__(self, capacity, keep_logits=False):
        self.capacity = capacity
        self.pred = np.zeros(capacity, np.float32)
        self.tgt = np.zeros(capacity, np.uint8)
        self.logit = np.zeros(capacity, np.float32) if keep_logits else None
        self.ctr = np.zeros(4, np.int64)
        self.loss_sum = np.float64(0.0)

    def append(self, values, targets, mode, loss=None):
        """mode 0: logits, 1: probabilities; loss: a float32 value or None"""
        values = np.asarray(values, np.float32).reshape(-1)
        targets = np.asarray(targets, np.float32).reshape(-1)
        cursor, count = int(self.ctr[0]), values.size
        take = max(0, min(count, self.capacity - cursor))
        p = settle(sigmoid_f32(values) if mode == 0 else values)
        self.pred[cursor:cursor + take] = p[:take]
        self.tgt[cursor:cursor + take] = targets[:take] != 0
        if self.logit is not None and mode == 0:
            self.logit[cursor:cursor + take] = values[:take]
        self.ctr[0] = cursor + take
        self.ctr[2] += count - take
        if loss is not None:
            self.loss_sum = np.float64(self.loss_sum + np.float64(np.float32(loss)))
            self.ctr[1] += 1


# ------------------------------------------------------------------------------------------------------------- the sort
def sort_key(p):
    """uint32 key that DESCENDS with the float: a = bits ^ (sign ? 0xFFFFFFFF : 0x80000000) ascends, key = ~a"""
    b = np.asarray(p, np.float32).reshape(-1).view(np.uint32)
    a = b ^ np.where(b >> 31 == 1, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))
    return ~a


def key_to_float(key):
    a = ~np.asarray(key, np.uint32)
    return np.where(a >> 31 == 1, a ^ np.uint32(0x80000000), ~a).astype(np.uint32).view(np.float32)


def radix_sort(keys, vals):
    """the kernel's sort: four stable counting passes over 8-bit digits, least significant first"""
    keys, vals = np.asarray(keys, np.uint32), np.asarray(vals, np.uint8)
    for shift in (0, 8, 16, 24):
        order = np.argsort((keys >> np.uint32(shift)) & np.uint32(255), kind="stable")
        keys, vals = keys[order], vals[order]
    return keys, vals


def stable_sort(keys, vals):
    order = np.argsort(np.asarray(keys, np.uint32), kind="stable")
    return np.asarray(keys, np.uint32)[order], np.asarray(vals, np.uint8)[order]


# ------------------------------------------------------------------------------------------------------------- the curves
def tie_group_ends(sorted_keys):
    """True at the last element of every run of equal keys"""
    k = np.asarray(sorted_keys, np.uint32)
    last = np.ones(k.size, bool)
    last[:-1] = k[1:] != k[:-1]
    return last


def curve(pred, tgt):
    """(sorted keys, inclusive positives at every position, indices of the tie-group ends)"""
    keys, vals = radix_sort(sort_key(pred), np.asarray(tgt, np.uint8) != 0)
    tps = np.cumsum(vals.astype(np.int64))
    return keys, tps, np.flatnonzero(tie_group_ends(keys))


def auroc_numerator(tps, ends):
    """2 P N AUROC = sum over tie groups of fp_g * (2 * tp_before_g + tp_g), a Python integer"""
    tp_e = tps[ends]
    tp_p = np.concatenate([[0], tp_e[:-1]])
    size = np.diff(np.concatenate([[-1], ends]))
    tp_g = tp_e - tp_p
    fp_g = size - tp_g
    return int(np.sum(fp_g.astype(np.int64) * (2 * tp_p + tp_g).astype(np.int64)))      # < 2 P N < 2^63: exact


def average_precision(tps, ends, P):
    if P == 0:
        return float("nan")
    tp_e = tps[ends].astype(np.float64)
    recall = tp_e / np.float64(P)
    prev = np.concatenate([[0.0], recall[:-1]])
    precision = tp_e / (ends + 1).astype(np.float64)
    return float(np.sum((recall - prev) * precision))


def f1_sweep(keys, tps, P):
    """F1 at (double)p >= i / 100.0 for i = 1 .. 99: 2 tp / (predicted + positives), 0 when that is 0"""
    neg = -key_to_float(keys).astype(np.float64)              # ascending
    thr = np.arange(1, 100) / 100.0
    predicted = np.searchsorted(neg, -thr, side="right")      # #{p >= thr}
    tp = np.where(predicted > 0, tps[np.maximum(predicted, 1) - 1], 0)
    denom = predicted + P
    return [2.0 * int(t) / int(d) if d > 0 else 0.0 for t, d in zip(tp, denom)]


def metrics(pred, tgt, loss_sum=0.0, batches=0, stored=None, dropped=0):
    """the eight float64 of mtmp_eval_metrics: auroc, ap, f1 at 0.01, best f1, mean loss, n, positives, status"""
    pred, tgt = np.asarray(pred, np.float32).reshape(-1), np.asarray(tgt).reshape(-1)
    n = pred.size
    loss = float(np.float64(loss_sum) / np.float64(batches)) if batches > 0 else float("nan")
    status = float((0 if stored is None or stored == n else 1) + (2 if dropped else 0))
    if n == 0:
        return [0.0, float("nan"), 0.0, 0.0, loss, 0.0, 0.0, status]
    keys, tps, ends = curve(pred, tgt)
    P = int(tps[-1])
    N = n - P
    auroc = float(np.float64(auroc_numerator(tps, ends)) / np.float64(2 * P * N)) if P > 0 and N > 0 else 0.0
    f1s = f1_sweep(keys, tps, P)
    return [auroc, average_precision(tps, ends, P), f1s[0], max(f1s), loss, float(n), float(P), status]


# ------------------------------------------------------------------------------------------------------------- the cases
def case(kind, n, seed=0):
    """(pred float32 [n], tgt uint8 [n]) of one of the six input kinds; the predictions are already settled"""
    g = np.random.default_rng(1000003 * seed + 7919 * n + KINDS.index(kind))
    tgt = (g.random(n) < 0.3).astype(np.uint8)
    if kind == "continuous":
        pred = g.random(n, np.float32)
    elif kind == "ties20":
        pred = (g.integers(0, 20, n) / 19.0).astype(np.float32)
    elif kind == "all_equal":
        pred = np.full(n, 0.25, np.float32)
    elif kind == "all_positive":
        pred, tgt = g.random(n, np.float32), np.ones(n, np.uint8)
    elif kind == "all_negative":
        pred, tgt = g.random(n, np.float32), np.zeros(n, np.uint8)
    elif kind == "wide":
        # every exponent, both signs, denormals, +-0, +-FLT_MAX: all four digits of the key matter
        bits = g.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        pred = bits.view(np.float32).copy()
        pred[0::7] = g.choice(np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 0.5, -0.5], np.float32), pred[0::7].size)
        pred = settle(pred)
    else:
        raise ValueError(kind)
    return pred, tgt
