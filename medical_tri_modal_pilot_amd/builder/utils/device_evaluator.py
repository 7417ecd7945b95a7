"""``DeviceEvaluator``: the ``Evaluator`` of builder/utils/metrics.py with its state on the device (csrc/evaluator.hip).

``Evaluator`` keeps a Python list of every batch's tensors and computes the metrics with a dozen torch launches on float64
copies; the trainer's test flow ends every batch with ``loss.item()``.  Here a batch is ONE small launch that appends behind a
cursor kept on the device (no host value: the launch can sit inside a captured hipGraph), and the pass ends with
``mtmp_eval_metrics`` and one device-to-host copy of 64 bytes -- the only wait of a pass.

Drop-in for ``logger.evaluator``: ``best_auc``, ``reset()``, ``add_batch(y_true, y_pred)`` (probabilities, as the trainer's test
flow hands them over) and ``performance_metric()`` (the same list, rounded to 4 decimals the same way).  New: ``add_logits`` (the
sigmoid is evaluated in float64 inside the append, the batch's loss is summed on the device), ``metrics()`` (the eight
unrounded values), ``predictions()`` (what was stored, for a caller that wants to re-threshold; it syncs).

Definitions are metrics.py's: exact curves over the distinct prediction values, AUROC 0 when a class is absent, AP NaN
without positives, F1 at ``pred >= 0.01``.  ``capacity`` is fixed at construction (at most 2^24); a pass that appends more
raises in ``metrics()`` / ``performance_metric()`` and names how many predictions were dropped.
"""
import numpy as np
import torch

from medical_tri_modal_pilot_amd import ops
from medical_tri_modal_pilot_amd.builder.data import resolve_device

METRIC_NAMES = ("auroc", "ap", "f1", "best_f1", "loss", "n", "n_pos", "status")


class DeviceEvaluator(object):
    def __init__(self, args, device, capacity, keep_logits=False):
        if "rmse" in getattr(args, "auxiliary_loss_type", ""):
            raise ValueError("DeviceEvaluator: 'rmse' in args.auxiliary_loss_type -- the rmse list is not kept on the device "
                             "(the trainer never hands one over); keep builder.utils.metrics.Evaluator for that")
        device = resolve_device(device)
        if device.type != "cuda":
            raise RuntimeError(f"DeviceEvaluator runs on an MI355X only (device {device}); there is no CPU fallback")
        capacity = int(capacity)
        if not 1 <= capacity <= ops.EVAL_MAX_CAPACITY:
            raise ValueError(f"DeviceEvaluator: capacity {capacity} is not in 1 .. {ops.EVAL_MAX_CAPACITY} (2^24)")
        self.args, self.device, self.capacity = args, device, capacity
        self.n_labels = args.output_dim
        self.batch_size = args.batch_size
        if args.model_types == "classification" and args.loss_types == "rmse":
            self.best_auc = float("inf")
        else:
            self.best_auc = 0
        self.pred = torch.zeros(capacity, dtype=torch.float32, device=device)
        self.tgt = torch.zeros(capacity, dtype=torch.uint8, device=device)
        self.logit = torch.zeros(capacity, dtype=torch.float32, device=device) if keep_logits else None
        # ctr int64 [4] and loss_sum float64 [1] share ONE allocation: reset() is one memset
        self._state = torch.zeros(6, dtype=torch.int64, device=device)
        self.ctr = self._state[:4]
        self.loss_sum = self._state[4:5].view(torch.float64)
        self._out = torch.zeros(8, dtype=torch.float64, device=device)
        self._ws = None
        self.appended = 0                    # the HOST's count of values handed over since reset() (no device value is read)
        self._metrics = None                 # metrics() of the state as it stands (performance_metric() copies nothing again)

    # ------------------------------------------------------------------------------------------------ the Evaluator surface
    def reset(self):
        self._state.zero_()
        self.appended = 0
        self._metrics = None

    def add_batch(self, y_true, y_pred_multi, rmse=None):
        if rmse is not None:
            raise ValueError("DeviceEvaluator.add_batch: an rmse value was handed over; keep builder.utils.metrics.Evaluator for that")
        self._append(y_pred_multi, y_true, ops.EVAL_PROBS, None)

    def performance_metric(self):
        """[auc, apr, f1] rounded to 4 decimals like Evaluator.performance_metric (which rounds the float32 its metrics return)."""
        m = self.metrics()
        vals = [np.float32(m["auroc"]), np.float32(m["ap"]), np.float32(m["f1"])]
        return list(np.round(np.array(vals, dtype=np.float64), 4))

    # ------------------------------------------------------------------------------------------------ new
    def add_logits(self, logits, y_true, loss=None):
        """A batch of raw logits (the sigmoid is part of the append) and, optionally, its mean loss as a device tensor."""
        self._append(logits, y_true, ops.EVAL_LOGITS, loss)

    def metrics(self) -> dict:
        """The eight values of mtmp_eval_metrics, unrounded.  One device-to-host copy of 64 bytes: the only wait of a pass."""
        if self._metrics is not None:
            return dict(self._metrics)
        n = min(self.appended, self.capacity)
        need = ops.eval_workspace_bytes(n)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            ops.eval_metrics(self.pred, self.tgt, n, self.ctr, self.loss_sum, self._ws, self._out)
        vals = self._out.cpu().tolist()
        m = dict(zip(METRIC_NAMES, vals))
        status = int(m["status"])
        if status & 2 or self.appended > self.capacity:
            raise RuntimeError(f"DeviceEvaluator: capacity {self.capacity} was too small for this pass: {self.appended} predictions "
                               f"were added, {self.appended - self.capacity} dropped; build it with a larger capacity")
        if status:
            raise RuntimeError(f"DeviceEvaluator: the device holds another number of predictions than the {n} the host counted "
                               "(was the state changed behind the evaluator, or a captured append replayed without add_logits?)")
        m["n"], m["n_pos"], m["status"] = int(m["n"]), int(m["n_pos"]), status
        self._metrics = m
        return dict(m)

    def predictions(self):
        """(pred float32 [n], tgt uint8 [n], logit float32 [n] | None): copies of what the pass stored.  Waits for the device."""
        n = int(self.ctr[0].item())
        return (self.pred[:n].clone(), self.tgt[:n].clone(), None if self.logit is None else self.logit[:n].clone())

    def count_replayed(self, count: int):
        """A captured append was replayed (builder/trainer/validate.py): the host's count follows."""
        self.appended += int(count)
        self._metrics = None

    # ------------------------------------------------------------------------------------------------
    def _flat(self, t, what):
        if not torch.is_tensor(t) or t.device != self.device:
            raise ValueError(f"DeviceEvaluator: {what} is {'on ' + str(t.device) if torch.is_tensor(t) else 'not a tensor'}, "
                             f"the evaluator is on {self.device}")
        t = t.detach().reshape(-1)
        if t.dtype != torch.float32:
            t = t.float()
        return t if t.is_contiguous() else t.contiguous()

    def _append(self, values, y_true, mode, loss):
        v, t = self._flat(values, "the prediction tensor"), self._flat(y_true, "the target tensor")
        if v.numel() != t.numel() or v.numel() < 1:
            raise ValueError(f"DeviceEvaluator: {v.numel()} predictions for {t.numel()} targets")
        if loss is not None:
            loss = self._flat(loss, "the loss")
            if loss.numel() != 1:
                raise ValueError("DeviceEvaluator: the loss of a batch is one value")
        with torch.cuda.device(self.device):
            ops.eval_append(v, t, mode, self.pred, self.tgt, self.logit, self.ctr, self.loss_sum, loss)
        self._metrics = None
        if not torch.cuda.is_current_stream_capturing():      # (a captured append runs at its replays: count_replayed)
            self.appended += v.numel()
