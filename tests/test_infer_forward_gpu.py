"""-m gpu: the inference forward (--infer-forward 1, ops.inference_forward) end to end, on the model and batches of
tests/test_validation_gpu.py (TRI_MBT_VSLTCLS, 2 layers, batch 8, TIE-len 48): validate() with the flag on against the flag off in
fp32 and bf16, replayed from a hipGraph against eager, the training step that follows a flag-on pass, the "test" flow of
TRI_MBT_V1 and tri_mbt_vmultivslt, the kernels that go through ops.call, and the nodes' refusal of a backward.  Replayed cases run
in a pytest process of their own, as in test_validation_gpu.py."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_gpu_parity import DEV, ROOT, _product_model
from tests.test_validation_gpu import SIZES, T_LEN, _batches, _train_steps, _validate

pytestmark = pytest.mark.gpu
IN_CHILD = os.environ.get("MTMP_TEST_CHILD") == "1"


def _in_child(test_id):
    r = subprocess.run([sys.executable, "-m", "pytest", f"{os.path.abspath(__file__)}::{test_id}", "-x", "-q", "-s", "-m", "gpu",
                        "-p", "no:cacheprovider"], env=dict(os.environ, MTMP_TEST_CHILD="1"), cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0 and "1 passed" in r.stdout


def _model(dtype, hip_graph, infer):
    args, model = _product_model(2, 0, dtype, hip_graph=hip_graph, batch_size=8, TIE_len=T_LEN, infer_forward=infer)
    model.train()
    model.img_encoder.eval()
    return args, model


def _logits(dtype, hip_graph, infer, batches):
    args, model = _model(dtype, hip_graph, infer)
    return _validate(args, model, batches)[4].double().cpu(), args, model


def _rms(t):
    return float(t.pow(2).mean().sqrt())


class _Calls:
    """records the entry names that go through _lib.call while it is active"""

    def __enter__(self):
        from medical_tri_modal_pilot_amd import _lib, ops
        self.mods, self.orig, self.names, self.chain_rows = (_lib, ops), _lib.call, [], []

        def call(name, *a):
            self.names.append(name)
            if name == "mtmp_ln_gemm_signs_grouped":      # (dtype, n, x, gamma, beta, w, bias, y, xn, stats, signs, M, ...)
                self.chain_rows.append(sum(a[11][i] for i in range(a[1])))
            return self.orig(name, *a)

        for m in self.mods:
            m.call = call
        return self

    def __exit__(self, *exc):
        for m in self.mods:
            m.call = self.orig

    def has(self, prefix):
        return any(n.startswith(prefix) for n in self.names)


def test_fp32_flag_on_equals_flag_off():
    """(a) the project's fp32 tolerance"""
    batches = _batches()
    off, on = _logits("fp32", 0, 0, batches)[0], _logits("fp32", 0, 1, batches)[0]
    e = float((on - off).abs().max() / off.abs().max())
    print(f"fp32 validate() logits, flag on against off: {e:.3e}")
    assert on.numel() == sum(SIZES) and bool(torch.isfinite(on).all()) and e <= 1e-4


def test_bf16_flag_on_is_as_close_to_fp32_as_flag_off():
    """(b) both bf16 paths round at the same points and differ in summation order only: a factor of two over the existing path's own
    error against the fp32 logits, plus 2^-8 of their size, is the margin"""
    batches = _batches()
    ref = _logits("fp32", 0, 0, batches)[0]
    off, on = _logits("bf16", 0, 0, batches)[0], _logits("bf16", 0, 1, batches)[0]
    e_off, e_on = _rms(off - ref), _rms(on - ref)
    print(f"bf16 validate() logits against fp32: e_on {e_on:.4e} e_off {e_off:.4e} rms(fp32) {_rms(ref):.4e}")
    assert bool(torch.isfinite(on).all()) and e_on <= 2 * e_off + 2.0 ** -8 * _rms(ref)


def test_replayed_equals_eager_and_a_flip_captures_afresh():
    """(c)"""
    if not IN_CHILD:
        return _in_child("test_replayed_equals_eager_and_a_flip_captures_afresh")
    batches = _batches()
    eager_on = _logits("bf16", 0, 1, batches)[0]
    eager_off = _logits("bf16", 0, 0, batches)[0]
    on, args, model = _logits("bf16", 1, 1, batches)
    assert torch.equal(on, eager_on)
    st = model._mtmp_graph_eval.stats()
    assert not model._mtmp_graph_eval.disabled and st["captures"] == 1 and st["replays"] == 3
    args.infer_forward = 0                               # the same model, the other setting: nothing is replayed from the first
    with _Calls() as rec:
        off = _validate(args, model, batches)[4].double().cpu()
    st2 = model._mtmp_graph_eval.stats()
    print("eval graph after the flip:", st2)
    assert torch.equal(off, eager_off) and st2["captures"] == 2 and st2["replays"] == 6
    assert not rec.has("mtmp_ffn_block")                 # the warm-up step and the capture ran the training forward
    args.infer_forward = 1
    again = _validate(args, model, batches)[4].double().cpu()
    assert torch.equal(again, eager_on) and model._mtmp_graph_eval.stats()["captures"] == 3


def test_training_step_after_a_flag_on_pass():
    """(d) loss, parameters and BatchNorm statistics, bit for bit"""
    import tests.test_validation_gpu as V
    model_fn = V._model
    try:
        V._model = lambda hip_graph, **over: model_fn(hip_graph, infer_forward=1, **over)
        l_val, p_val, s_val, _ = _train_steps(0, True)
    finally:
        V._model = model_fn
    l_ref, p_ref, s_ref, _ = _train_steps(0, False)
    print(f"training around a flag-on validation pass: losses {l_val} without {l_ref}")
    assert all(math.isfinite(v) for v in l_val)
    assert [np.float32(v).tobytes() for v in l_val] == [np.float32(v).tobytes() for v in l_ref]
    assert torch.equal(p_val, p_ref) and all(torch.equal(s_val[k], s_ref[k]) for k in s_val)


@pytest.mark.parametrize("name,tag", [("tri_mbt_v1", "tri_v1"), ("tri_mbt_vmultivslt", "tri_vmultivslt")])
def test_test_flow_of_the_other_nodes(name, tag):
    """(e) the "test" flow through a dense last layer (FusionStackFn) and through MultiTokenStackFn (prefix masks), fp32"""
    import filler
    from medical_tri_modal_pilot_amd.builder.trainer import get_trainer
    from tests.test_noshnoavgtr_gpu import G, _Logger, _build, _trainer_kw
    Gd = G(tag + "_step")
    a, model = _build(name, tag)
    bt = filler.make_batch(int(Gd["seed"]), int(Gd["B"]), int(Gd["T"]))
    model.eval()
    got = {}
    for flag in (0, 1):
        a.infer_forward = flag
        lg = _Logger()
        with _Calls() as rec:
            _, loss = get_trainer(iteration=1, input_lengths=bt["input_lengths"].clone(), txt_lengths=bt["txt_lengths"].clone(),
                                  flow_type="test", **_trainer_kw(a, model, bt, lg))
        (_t, prob), = lg.evaluator.calls
        got[flag] = (loss, prob.double().cpu())
        assert flag or not rec.has("mtmp_ffn_block"), name
    e = float((got[1][1] - got[0][1]).abs().max() / got[0][1].abs().max())
    print(f"{name}: test-flow probabilities, flag on against off {e:.3e}; losses {got[1][0]} {got[0][0]}")
    assert e <= 1e-4 and abs(got[1][0] - got[0][0]) <= 1e-4 * max(1.0, abs(got[0][0]))


def test_kernels_that_run():
    """(f)"""
    from medical_tri_modal_pilot_amd import ops
    batches = _batches()[:1]
    args, model = _model("bf16", 0, 0)
    with _Calls() as rec:
        off = _validate(args, model, batches)[4]
    assert not rec.has("mtmp_ffn_block") and rec.has("mtmp_ln_gemm_signs")
    rows_off = list(rec.chain_rows)
    args.infer_forward = 1
    with _Calls() as rec:
        on = _validate(args, model, batches)[4]
    print("flag on:", sorted(set(rec.names)), "rows of the chain's launches", rec.chain_rows, "flag off", rows_off)
    # the dense layers (8 samples x 53 rows or more) run the fused block; what is left of the chain are the few-row launches below
    # tuning.FFN_BLOCK_MIN_ROWS: the four exchange rows per sample of the image / text streams (ffn_rows) and the CLS rows of the
    # last layer (cls_tok)
    assert rec.has("mtmp_ffn_block") and max(rows_off) >= 8 * 53
    assert all(r <= 2 * 8 * 4 for r in rec.chain_rows) and len(rec.chain_rows) < len(rows_off), (rec.chain_rows, rows_off)
    assert not any(n.startswith("mtmp_ln_gemm_signs") and n != "mtmp_ln_gemm_signs_grouped" for n in rec.names)
    assert bool(torch.isfinite(on).all())
    # under grad mode the flag changes nothing; without it a uni-modal layer (EncoderLayerFn) takes the fused block too
    model.eval()
    z = torch.randn(8, 512, 256, device=DEV, dtype=torch.bfloat16)
    layer = model.fusion_transformer.layer_stacks[0][0]
    with ops.inference_forward(True), torch.enable_grad(), _Calls() as rec:
        out, _ = layer(z, None)
    assert not rec.has("mtmp_ffn_block") and rec.has("mtmp_ln_gemm_signs") and out.requires_grad
    with ops.inference_forward(True), torch.no_grad(), _Calls() as rec:
        out2, _ = layer(z, None)
    assert rec.has("mtmp_ffn_block") and not rec.has("mtmp_ln_gemm_signs") and not out2.requires_grad
    with torch.no_grad(), _Calls() as rec:                     # flag off
        layer(z, None)
    assert not rec.has("mtmp_ffn_block")


def test_a_node_run_with_infer_raises_on_backward():
    """(g) through autograd: the node ran with grad mode on and StackPlan(infer=True); its outputs carry no gradient, and its
    backward, called with what it kept, raises naming the switch"""
    from types import SimpleNamespace
    from medical_tri_modal_pilot_amd import ops
    from medical_tri_modal_pilot_amd.stack_plan import StackPlan
    from tests.test_layer_engine_gpu import _layer
    B, N, dt = 2, 24, torch.bfloat16
    P, fused = _layer(dt, 3)
    zs = [torch.randn(B, N, 256, device=DEV, dtype=dt, requires_grad=True) for _ in range(3)]
    missing = torch.zeros(B, dtype=torch.int64, device=DEV)
    plan = StackPlan(n_layers=1, kv=[None, None, None], missing=missing, drop_p=0.0, seeds=[[(0, 0)] * 3], fused=[[fused] * 3],
                     dtype=dt, prebuilt=True, infer=True)
    bott = torch.zeros(1, 4, 256, device=DEV)
    outs = ops.FusionStackFn.apply(zs[0], zs[1], zs[2], bott, *(list(P) * 3), plan)
    assert all(not o.requires_grad for o in outs if o is not None)
    with pytest.raises(RuntimeError, match="infer"):
        ops.FusionStackFn.backward(SimpleNamespace(plan=plan, saved=[]), *([None] * 4))
    with pytest.raises(RuntimeError):
        outs[0].float().sum().backward()
