"""CPU checks for TRI_MBT_VNOSHNOAVGTR (no HIP kernel is launched): the model's torch forms and the trainer's two losses against
tests/golden/tri_vnoshnoavgtr_step.npz -- the reference's class driven by the reference's own ``missing_trainer``
(tests/golden/gen/make_golden_noshnoavgtr.py) --, the set table, the constructor's refusals, the C surface and get_model's message.

The fusion encoder has no CPU form in this package (its layers are HIP kernels), so the model test computes the three streams'
encoder outputs with the CPU oracle and runs the model's own head, loss and candidate mean -- the torch fallbacks -- on them."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import filler
from oracle import tri_mbt_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "medical_tri_modal_pilot_amd", "libmtmp_hip.so")
NEW_SYMBOLS = ["mtmp_head3_ws_floats", "mtmp_head3_bwd_ws_floats", "mtmp_head3_fwd", "mtmp_head3_bwd", "mtmp_candidate_mean_fwd",
               "mtmp_candidate_mean_bwd", "mtmp_bce_masked_mean"]


def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "tri_vnoshnoavgtr_step.npz"), allow_pickle=False)


def _args(*extra, model="tri_mbt_vnoshnoavgtr", input_types="vslt_img_txt"):
    from medical_tri_modal_pilot_amd.control.config import parse_args
    a = parse_args(["--input-types", input_types, "--model", model, "--modality-inclusion", "train-missing_test-missing",
                    "--batch-size", "4", "--transformer-num-layers", "2", "--imgtxt-time", "1", "--mbt-only-vslt", "1",
                    "--dropout", "0.0", "--compute-dtype", "fp32", *extra])
    a.device, a.output_dim = torch.device("cpu"), 1
    return a


def _digest(t):
    f = t.detach().reshape(-1).double().cpu()
    idx = torch.linspace(0, f.numel() - 1, 8).long()
    return torch.cat([f.norm().view(1), f[idx]])


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _state_dict():
    with open(os.path.join(ROOT, "tests", "golden", "state_shapes_tri_vnoshnoavgtr_L2.json")) as f:
        shapes = json.load(f)
    sd = {k: filler.fill_tensor(k, torch.zeros(s)) for k, (s, dt_) in shapes.items() if dt_.startswith("float")}
    sd["fusion_transformer.positional_encoding.pe"] = O.sinusoid_table(2500, 256).unsqueeze(0)
    return sd, shapes


def test_golden_holds_all_four_patterns_and_the_set_table_is_the_loss_mask():
    """S(missing_num) of ops._present_rows == the mask the reference's trainer takes from the raw flags (trainer.py:170-173)"""
    from medical_tri_modal_pilot_amd import ops
    from medical_tri_modal_pilot_amd.builder.trainer import missing_to_num
    Gd = _golden()
    missing, mnum = torch.from_numpy(Gd["missing"]), torch.from_numpy(Gd["missing_num"])
    assert sorted(mnum.tolist()) == [0, 1, 2, 3] and tuple(Gd["logits"].shape) == (3, 4, 1)
    assert torch.equal(missing_to_num(missing, "txt1_img1")[0], mnum)
    mask = ops._present_rows(mnum)
    assert torch.equal(mask, missing.T == 0)
    want = {0: [True, True, True], 1: [True, True, False], 2: [True, False, True], 3: [True, False, False]}
    for b, c in enumerate(mnum.tolist()):
        assert mask[:, b].tolist() == want[c]
    assert torch.equal(ops._present_rows(mnum + 4), mask)                    # read as id & 3


def test_model_head_loss_and_candidate_mean_on_cpu_vs_golden():
    from medical_tri_modal_pilot_amd import ops
    from medical_tri_modal_pilot_amd.builder.models import get_model
    from medical_tri_modal_pilot_amd.builder.trainer.trainer import eval_logits, train_loss
    Gd = _golden()
    sd, shapes = _state_dict()
    a = _args()
    model = get_model(a)(a)
    assert type(model).__name__ == "TRI_MBT_VNOSHNOAVGTR"
    res = model.load_state_dict(sd, strict=False)
    assert not [k for k in res.missing_keys if "relative_position_index" not in k and "idx" not in k], res
    assert set(model.state_dict()) == set(shapes)
    pnames = [n for n, _ in model.named_parameters()]
    assert pnames == [k for k in shapes if k in set(pnames)]                 # registration order = the reference's
    assert sorted(n for n, _ in model.hot_parameters()) == sorted(str(s) for s in Gd["grad_names"])
    bt = filler.make_batch(int(Gd["seed"]), int(Gd["B"]), int(Gd["T"]))
    mnum = torch.from_numpy(Gd["missing_num"])
    assert torch.equal(bt["missing_num"], mnum) and np.array_equal(bt["missing"].numpy(), Gd["missing"])
    tmax = int(bt["input_lengths"].max())
    img_time, txt_time = bt["img_time"].half().float().reshape(-1), bt["txt_time"].half().float()
    with torch.no_grad():                                                    # the three streams' encoder outputs: CPU oracle
        v = O.tie_embedding(sd, bt["x"][:, :tmax])
        t = F.linear(bt["txt"], sd["txt_embedding.weight"], sd["txt_embedding.bias"])
        feat = O.swin_forward(sd, "img_encoder", bt["img"].reshape(-1, 1, bt["img"].shape[-2], bt["img"].shape[-1]))
        i = F.linear(feat.flatten(1, 2), sd["linear.weight"], sd["linear.bias"])
        i = i + O.lin_ln_relu(sd, "ie_time", img_time.unsqueeze(1)).unsqueeze(1) + sd["ie_feat.weight"][18]
        t = t + O.lin_ln_relu(sd, "ie_time", txt_time.unsqueeze(1)).unsqueeze(1) + sd["ie_feat.weight"][19]
        outs, _ = O.mbt_encoder(sd, "fusion_transformer", [v, i, t], bt["input_lengths"], bt["txt_lengths"], img_time, mnum,
                                n_layers=2, n_head=4, vsltonly=0)
    assert len(outs) == 3
    model.train()
    demo = model.ie_demo(torch.stack([bt["age"], bt["gen"]], dim=1))
    out, o2, o3 = model._head(outs, demo, bt["age"], bt["gen"], mnum, False)
    assert o2 is None and o3 is None and tuple(out.shape) == (3, 4, 1)
    assert _rel(out, torch.from_numpy(Gd["logits"])) <= 1e-4
    crit = torch.nn.BCEWithLogitsLoss()
    tens = dict(final_target=bt["y"].float(), missing_num=mnum)
    loss = train_loss(a, crit, out.squeeze(), tens)
    assert abs(float(loss) - float(Gd["loss"])) <= 1e-5
    loss.backward()
    prm = dict(model.named_parameters())
    med = float(np.median(Gd["grad_digest"][:, 0]))
    checked = 0
    for n_, gd in zip((str(s) for s in Gd["grad_names"]), Gd["grad_digest"]):
        if not n_.startswith(("fc_lists.", "ie_demo.", "layer_norms_after_concat.")):
            continue                                                         # (the encoder's side has no CPU form)
        assert gd[0] >= 1e-4 * med, n_
        assert _rel(_digest(prm[n_].grad), torch.from_numpy(gd)) <= 1e-4, n_
        checked += 1
    assert checked == 6 + 3 * 6
    with torch.no_grad():                                                    # the test flow (trainer.py:223-234)
        mean = eval_logits(a, out.squeeze(), tens)
        assert tuple(mean.shape) == (4,)
        assert abs(float(crit(mean, tens["final_target"])) - float(Gd["test_loss"])) <= 1e-5
        assert _rel(torch.sigmoid(mean), torch.from_numpy(Gd["test_prob"])) <= 1e-4
    # for every other model the two helpers are the plain calls
    b = _args(model="tri_mbt_vnoshavgtr")
    assert eval_logits(b, mean, tens) is mean
    assert float(train_loss(b, crit, mean, tens)) == float(crit(mean, tens["final_target"]))


def test_constructor_refusals():
    from medical_tri_modal_pilot_amd.builder.models import get_model
    cls = get_model(_args())
    with pytest.raises(NotImplementedError, match="--input-types vslt_img_txt"):
        a = _args()
        a.input_types = "vslt_txt"
        cls(a)
    with pytest.raises(NotImplementedError, match="--fullmodal-definition txt1_img1"):
        a = _args()
        a.fullmodal_definition = "img1"
        cls(a)
    with pytest.raises(NotImplementedError, match="swin"):                   # what its parents refuse
        a = _args()
        a.img_model_type = "vit"
        cls(a)
    with pytest.raises(ValueError, match="transformer_dim must be 256"):
        a = _args()
        a.transformer_dim = 128
        cls(a)


def test_new_symbols_are_exported_and_abi_stays_6():
    if not os.path.exists(LIB):
        import __graft_entry__ as ge
        ge.build()
    from medical_tri_modal_pilot_amd import _lib
    from tests import abi
    lib = ctypes.CDLL(LIB)
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(abi.declaration(name)[1]), name
        assert hasattr(lib, name), f"{name} is not exported"
    lib.mtmp_abi_version.restype = ctypes.c_int
    assert lib.mtmp_abi_version() == 6
    lib.mtmp_head3_ws_floats.restype = lib.mtmp_head3_bwd_ws_floats.restype = ctypes.c_int
    assert lib.mtmp_head3_ws_floats(256) == 3 * 256 * 769 and lib.mtmp_head3_bwd_ws_floats(5) == 5 * 256 * 10


def test_ops_and_switch_are_there_and_get_model_names_the_model():
    from medical_tri_modal_pilot_amd import ops, tuning
    from medical_tri_modal_pilot_amd.builder.models import get_model
    assert tuning.HIP_TRI_HEAD in (True, False)
    for name in ("TriHeadFn", "CandidateMeanFn", "BceMaskedMean", "bce_masked_mean", "candidate_mean"):
        assert hasattr(ops, name), name
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.TriHeadFn.apply(*([torch.zeros(2, 256)] * 3), torch.zeros(2), torch.zeros(2), *([torch.zeros(1)] * 12))
    a = _args()
    a.model = "tri_mbt_vmulti"
    with pytest.raises(NotImplementedError, match="tri_mbt_vnoshnoavgtr"):
        get_model(a)
