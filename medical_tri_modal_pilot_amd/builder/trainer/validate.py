"""``validate``: the validation loop of the reference's ``2_train.py:213-287`` (and the test loop of ``:316-376``) as one call.

The reference walks the loader through ``get_trainer(flow_type="test")``: a forward of eager launches (host-bound, ~750 of
them), ``loss.item()`` at the end of every batch, and an evaluator that keeps a list of tensors.  Here the batch is prepared by
the trainer's own input side (trainer.prepare_step_inputs), the forward + BCE + append run under ``torch.no_grad()`` -- with
``--hip-graph 1`` replayed from a hipGraph of a SECOND graph.GraphedTrainStep kept on the model (``model._mtmp_graph_eval``; a
graph captured in eval mode is never replayed for a training step, nor the other way round) -- and predictions, targets and the
loss sum stay on the device (builder/utils/device_evaluator.py).  Nothing inside the loop waits for the device; the pass ends
with one 64-byte copy.

Replays read the live parameters (the per-layer derived weights are re-made inside the captured step), so nothing is captured
again after an optimizer step.  A short last batch is a signature of its own and runs as that signature's warm-up step, eagerly.
Past the capture budget the steps run eagerly, as in training.  Without ``--hip-graph 1`` the same function runs eagerly.
"""
import torch

from medical_tri_modal_pilot_amd import ops

from .trainer import _run_model, prepare_step_inputs, eval_logits


def _use_eval_graph(args, device) -> bool:
    """trainer._use_graph without the optimizer conditions, which only matter for training"""
    return int(getattr(args, "hip_graph", 0)) == 1 and torch.device(device).type == "cuda"


def validate(args, model, batches, device, criterion, evaluator) -> dict:
    """Runs ``batches`` (an iterable of the loader's 12-tuples, 2_train.py:223) through the model in eval mode and returns
    ``evaluator.metrics()`` (auroc, ap, f1, best_f1, loss = the mean of the batches' losses, n, n_pos, status) plus
    ``performance_metric`` (the reference's rounded list) and ``batches``.  ``evaluator``: a DeviceEvaluator on ``device``.
    The model's training / eval flags are put back as they were."""
    if int(getattr(args, "ddp", 0)) == 1:
        raise ValueError("validate: --ddp 1 is not supported: a sharded validation needs a gather of the evaluator state across "
                         "the ranks; run the pass on one rank, or keep get_trainer(flow_type='test')")
    if getattr(args, "auxiliary_loss_input", None) is not None:
        raise ValueError("validate: output_lengths / feasible (--auxiliary-loss-input) is not supported: missing_trainer does not "
                         "replay such a step from a graph either; keep get_trainer(flow_type='test')")
    if "rmse" in getattr(args, "auxiliary_loss_type", ""):
        raise ValueError("validate: the rmse auxiliary target is not supported; keep get_trainer(flow_type='test') and Evaluator")
    if not hasattr(evaluator, "add_logits"):
        raise TypeError("validate: the evaluator must be a DeviceEvaluator (add_logits, metrics)")
    device = torch.device(device)
    graphed = _use_eval_graph(args, device)
    gs = None
    modes = [(m, m.training) for m in model.modules()]
    model.eval()
    n_batches = 0
    infer = bool(int(getattr(args, "infer_forward", 0)))     # --infer-forward 1: layers that keep nothing, the fused FFN block
    try:
        evaluator.reset()
        for batch in batches:
            x, static, y, in_len, img, img_time, txt, txt_len, txt_time, missing, f_indices, _y2 = batch
            inp = prepare_step_inputs(args, x, static, in_len, y, model, device, graphed, graphed, None, img, txt, txt_len,
                                      (img_time, txt_time), missing)

            def step(t):
                with torch.no_grad(), ops.inference_forward(infer):
                    logits = eval_logits(args, _run_model(model, t, None, "test"), t)      # (un-averaged heads: the candidate mean)
                    loss = ops.bce_with_logits(criterion, logits, t["final_target"])
                    evaluator.add_logits(logits, t["final_target"], loss)
                return loss.detach()

            inputs = inp.tensors(target=True)
            if graphed:
                if gs is None:
                    gs = _eval_graph_step(args, model, inp.data.device, evaluator, criterion, infer)
                replays = gs.replays
                gs.run(inputs, step, None, reducer=None, round_fp16=inp.deferred)
                if gs.replays != replays:            # the captured append ran on the device, not in Python
                    evaluator.count_replayed(inp.final_target.numel())
            else:
                step(inputs)
            n_batches += 1
        result = evaluator.metrics()
        result["performance_metric"] = evaluator.performance_metric()
        result["batches"] = n_batches
        return result
    finally:
        for m, was in modes:
            m.training = was


def _eval_graph_step(args, model, device, evaluator, criterion, infer=False):
    from medical_tri_modal_pilot_amd.graph import GraphedTrainStep
    gs = getattr(model, "_mtmp_graph_eval", None)
    if gs is None or gs.device != device:
        # GraphedTrainStep registers its dropout step word with ops at construction; the training step's word stays the
        # registered one (eval mode draws no mask)
        word = ops._seed_word
        gs = model._mtmp_graph_eval = GraphedTrainStep(device, max_graphs=int(getattr(args, "hip_graph_max", 12)),
                                                       fallback=bool(int(getattr(args, "hip_graph_fallback", 0))))
        ops.set_seed_word(word)
    # a captured step appends into the buffers of the evaluator it was captured with and holds that criterion's launches -- and the
    # launches of the forward it was captured under (--infer-forward: other kernels): with another of any of the three, the
    # signatures are captured afresh (the old graphs stay parked, graph._ALIVE), so a graph captured under one setting is never
    # replayed under the other
    held = getattr(gs, "_mtmp_eval_objects", None)
    if held is None or held[0] is not evaluator or held[1] is not criterion or held[2] != bool(infer):
        if held is not None:
            gs.invalidate()
        gs._mtmp_eval_objects = (evaluator, criterion, bool(infer))
    enc = getattr(model, "fusion_transformer", None)
    if enc is not None and getattr(enc, "supports_segments", False):
        enc.graph_segments = None
    return gs
