"""CPU-only: the host side of the multi-token bottleneck encoder's building blocks -- the exchange weight table against the
reference's b_out_mean_map enumerated (mbt_encoder.py:98-101, 183-191), the trained-rows table against ``missing_multitoken == 0``
(trainer.py:79-83), the off-GPU form of ops.bce_rows_masked_mean, and what the new C entry points refuse before any launch (in the
style of tests/test_abi_refusals_cpu.py: the "device pointers" are made-up addresses that a refused call never reads; the mask
words are real host arrays, which the checks do read)."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MTMP_ERR_ARG = 1
P = 0x1000

BOTTLENECKS_MAP = [[0, 1, 2], [0, 1, 3], [0, 2, 3]]
B_OUT_MEAN_MAP = {0: [[0, 1, 2], [0, 1], [0, 2], [0]], 1: [[0, 1], [0, 1], [0], [0]],
                  2: [[0, 1], [0], [0, 1], [0]], 3: [[0, 1], [0], [1], [0]]}
NEW_SYMBOLS = ["mtmp_attn_prefix_fwd", "mtmp_attn_prefix_bwd", "mtmp_attn_prefix_fwd_grouped", "mtmp_attn_prefix_bwd_grouped",
               "mtmp_bottleneck_exchange_multi_fwd", "mtmp_bottleneck_exchange_multi_bwd", "mtmp_bce_rows_masked_mean"]


@pytest.fixture(scope="module")
def lib():
    from medical_tri_modal_pilot_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


def test_exchange_weight_table_is_b_out_mean_map_enumerated():
    from medical_tri_modal_pilot_amd import ops
    w = ops.multi_exchange_weights()
    assert w.shape == (4, 4, 3)
    # unit "outputs": stream m's rows of set s are the one-hot vector e_m, so a mean over holders reads off its weights
    for s in range(4):
        holders = [m for m in range(3) if s in BOTTLENECKS_MAP[m]]
        stack = torch.stack([torch.eye(3)[m] for m in holders])
        for pat in range(4):
            want = torch.mean(stack[torch.tensor(B_OUT_MEAN_MAP[s][pat])], dim=0)
            assert torch.allclose(w[s, pat], want, atol=0, rtol=0) or torch.allclose(w[s, pat], want, atol=1e-7), (s, pat, w[s, pat], want)
    assert [list(r) for r in ops.MULTI_BOTTLENECKS_MAP] == BOTTLENECKS_MAP and ops.N_PREFIX == 12


def test_loss_table_and_off_gpu_form():
    from medical_tri_modal_pilot_amd import ops
    mm = torch.tensor([[0., 0., 0., 0.], [1., 0., 1., 0.], [1., 1., 0., 0.], [1., 1., 1., 0.]])          # trainer.py:79-83
    assert torch.equal(torch.tensor(ops.MULTI_LOSS_TABLE), mm == 0)
    crit = torch.nn.BCEWithLogitsLoss()
    g = torch.Generator().manual_seed(4)
    for B, ids in ((4, [0, 1, 2, 3]), (7, [3, 3, 2, 2, 3, 2, 3]), (1, [1])):
        mnum = torch.tensor(ids)
        o = torch.randn(4, B, generator=g, requires_grad=True)
        y = (torch.rand(B, generator=g) > 0.5).float()
        miss = mm[mnum].permute(1, 0).reshape(-1)
        ref = crit(o.reshape(-1)[miss == 0], y.unsqueeze(0).repeat(4, 1).reshape(-1)[miss == 0])
        got = ops.bce_rows_masked_mean(crit, o, y, mnum)
        assert torch.equal(got, ref)
        assert torch.equal(torch.autograd.grad(got, o)[0], torch.autograd.grad(ref, o)[0])
    with pytest.raises(ValueError, match="logits"):
        ops.bce_rows_masked_mean(crit, torch.zeros(5, 3), torch.zeros(3), torch.zeros(3, dtype=torch.long))


def _words(vals):
    return (ctypes.c_uint16 * len(vals))(*vals)


OK12, HIDDEN12 = _words([0xFF0] * 4 + [0xF0F] * 4 + [0x0FF] * 4), _words([0xFF0] * 4 + [0xFFF] + [0xF0F] * 3 + [0x0FF] * 4)
W17 = _words([0] * 17)
PA, PA0 = (ctypes.c_void_p * 3)(P, P, P), (ctypes.c_void_p * 3)(None, P, P)


def _ints(*v):
    return (ctypes.c_int * 3)(*(v + (v[-1],) * (3 - len(v))))


def _mptr(w):
    return (ctypes.c_void_p * 3)(ctypes.addressof(w), None, None)


FWD = [1, P, P, P, P, None, None, P, None, None, OK12, 12, 2, 100, 4, 768, 256, 0.125, None]
BWD = [1, P, P, P, P, P, P, None, OK12, 12, P, P, P, P, 2, 100, 4, 768, 256, 256, 768, 0.125, None]
FWD_G = [1, 1, PA, PA, PA, PA, None, None, PA, None, None, None, _mptr(OK12), _ints(12), _ints(100), _ints(768), _ints(256), 2, 4, 0.125, None]
BWD_G = [1, 1, PA, PA, PA, PA, PA, PA, None, None, _mptr(OK12), _ints(12), PA, PA, PA, PA, _ints(100), _ints(768), _ints(256), _ints(256),
         _ints(768), 2, 4, 0.125, None]
CALLS = {
    "mtmp_attn_prefix_fwd": (FWD, [("P17", {10: W17, 11: 17}), ("N_below_P", {13: 10}), ("hidden_row", {10: HIDDEN12}), ("null", {1: None}),
                                   ("dtype7", {0: 7}), ("Pneg", {11: -1})]),
    "mtmp_attn_prefix_bwd": (BWD, [("P17", {8: W17, 9: 17}), ("N_below_P", {15: 10}), ("hidden_row", {8: HIDDEN12}), ("null", {1: None}),
                                   ("dtype7", {0: 7})]),
    "mtmp_attn_prefix_fwd_grouped": (FWD_G, [("P17", {12: _mptr(W17), 13: _ints(17)}), ("N_below_P", {14: _ints(10)}),
                                             ("hidden_row", {12: _mptr(HIDDEN12)}), ("null", {2: PA0}), ("dtype7", {0: 7}),
                                             ("n0", {1: 0}), ("n4", {1: 4})]),
    "mtmp_attn_prefix_bwd_grouped": (BWD_G, [("P17", {10: _mptr(W17), 11: _ints(17)}), ("N_below_P", {16: _ints(10)}),
                                             ("hidden_row", {10: _mptr(HIDDEN12)}), ("null", {2: PA0}), ("dtype7", {0: 7}),
                                             ("n0", {1: 0}), ("n4", {1: 4})]),
    "mtmp_bottleneck_exchange_multi_fwd": ([1, P, P, P, 4, 20, 12, 40, P, P, None],
                                           [("null", {3: None}), ("n_i", {6: 11}), ("weights", {9: None}), ("dtype7", {0: 7})]),
    "mtmp_bottleneck_exchange_multi_bwd": ([1, P, P, P, 4, 20, 12, 40, P, P, None],
                                           [("null", {1: None}), ("n_v", {5: 4}), ("missing", {8: None}), ("dtype7", {0: 7})]),
    "mtmp_bce_rows_masked_mean": ([P, P, P, 0x8CAF, P, P, 4, 8, None],
                                  [("null", {4: None}), ("R5", {6: 5}), ("R0", {6: 0}), ("B0", {7: 0}), ("table", {3: 0x10000})]),
}


def _cases():
    for entry, (good, cases) in CALLS.items():
        for label, change in cases:
            args = list(good)
            for i, v in change.items():
                args[i] = v
            yield pytest.param(entry, args, id=f"{entry}-{label}")


@pytest.mark.parametrize("entry,args", _cases())
def test_refused_before_any_launch(lib, entry, args):
    rc = getattr(lib, entry)(*args)
    msg = (lib.mtmp_last_error() or b"").decode()
    assert rc == MTMP_ERR_ARG, (entry, rc, msg)
    said = msg.split(":")[0].split(" ")[0]
    assert said.startswith("mtmp_") and (entry == said or entry.startswith(said + "_")), (entry, msg)


def test_new_symbols_are_declared_bound_and_exported(lib):
    from medical_tri_modal_pilot_amd import _lib
    from tests import abi
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(abi.declaration(name)[1]), name
        assert hasattr(lib, name), name


def test_ops_take_the_mask_and_default_to_none():
    import inspect
    from medical_tri_modal_pilot_amd import ops
    for fn, arg in ((ops.attn_fwd, "qk_mask"), (ops.attn_bwd, "qk_mask"), (ops.attn_fwd_grouped, "qk_masks"),
                    (ops.attn_bwd_grouped, "qk_masks"), (ops.layer_forward, "qk_masks")):
        assert inspect.signature(fn).parameters[arg].default is None, fn.__name__
    assert "qk_mask" in ops.LayerSaved._fields and ops.LayerSaved._field_defaults["qk_mask"] is None
    assert ops._mask_words(None) == (None, 0)
    w, n = ops._mask_words([0xFF0, 1])
    assert n == 2 and list(w) == [0xFF0, 1]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bottleneck_exchange_multi([torch.zeros(1, 12, 256)] * 3, torch.zeros(1, dtype=torch.long))


# ------------------------------------------------------------------ the two models and their encoder against the goldens
import json  # noqa: E402

import numpy as np  # noqa: E402

MODELS = [("tri_mbt_vmultivslt", "tri_vmultivslt"), ("tri_mbt_vmulti2", "tri_vmulti2")]


def _model(name):
    from medical_tri_modal_pilot_amd.builder.models import get_model
    from medical_tri_modal_pilot_amd.control.config import parse_args
    a = parse_args(["--input-types", "vslt_img_txt", "--model", name, "--modality-inclusion", "train-missing_test-missing",
                    "--lr-init", "1e-5", "--batch-size", "4", "--transformer-num-layers", "2", "--imgtxt-time", "1",
                    "--mbt-only-vslt", "1", "--dropout", "0.0", "--compute-dtype", "fp32"])
    a.device, a.output_dim = torch.device("cpu"), 1
    cls = get_model(a)
    assert cls.__name__ == name.upper()
    return a, cls(a)


@pytest.mark.parametrize("name,tag", MODELS)
def test_state_dict_and_hot_parameters_equal_the_goldens(name, tag):
    _, model = _model(name)
    with open(os.path.join(ROOT, "tests", "golden", f"state_shapes_{tag}_L2.json")) as f:
        shapes = json.load(f)
    sd = model.state_dict()
    mine = [k for k in sd if "relative_position_index" not in k]
    theirs = [k for k in shapes if "relative_position_index" not in k]
    assert mine == theirs                                                    # keys AND order
    assert all(list(sd[k].shape) == shapes[k][0] for k in mine)
    assert [n for n, _ in model.named_parameters()] == [k for k in theirs if k in dict(model.named_parameters())]
    enc = model.fusion_transformer
    assert tuple(enc.cls_token.shape) == (1, 4, 256) and tuple(enc.bottlenecks.shape) == (1, 4, 256)
    Gd = np.load(os.path.join(ROOT, "tests", "golden", tag + "_step.npz"), allow_pickle=False)
    assert set(n for n, _ in model.hot_parameters()) == set(str(s) for s in Gd["grad_names"])
    assert not hasattr(model, "rmse_layer") or name == "tri_mbt_vmulti2"
    assert type(model).TRAINS_ENCODER_IN_REFERENCE == (name == "tri_mbt_vmulti2")


@pytest.mark.parametrize("name,tag", MODELS)
def test_kv_len_and_mask_words_expand_to_the_recorded_masks(name, tag):
    import filler
    _, model = _model(name)
    enc = model.fusion_transformer
    Gd = np.load(os.path.join(ROOT, "tests", "golden", tag + "_step.npz"), allow_pickle=False)
    bt = filler.make_batch(int(Gd["seed"]), int(Gd["B"]), int(Gd["T"]))
    lens_in, txt_in = bt["input_lengths"].clone(), bt["txt_lengths"].clone()
    B, Ns = 4, [int(Gd["T"]) + 4, 49, bt["txt"].shape[1]]
    kv = enc.key_lengths([lens_in, 49, txt_in + 2], [(B, n) for n in Ns], torch.device("cpu"))
    assert torch.equal(lens_in, bt["input_lengths"]) and torch.equal(txt_in, bt["txt_lengths"])      # the caller's tensors stay
    words = enc.mask_words()
    for m in range(3):
        rec = Gd[f"mask{m}"]
        if rec.size == 0:
            assert kv[m] is None and words[m] is None and not enc.mask[m]
            continue
        N = 12 + Ns[m]
        assert rec.shape == (B, N, N) and kv[m].dtype == torch.int32
        P = len(words[m])
        assert P == (16 if m == 0 else 12)
        full = (torch.arange(N)[None, None, :] >= kv[m].long().clamp(max=N)[:, None, None]).expand(B, N, N).clone()
        blk = torch.tensor([[bool((words[m][i] >> j) & 1) for j in range(P)] for i in range(P)])
        full[:, :P, :P] |= blk
        assert torch.equal(full, torch.from_numpy(rec)), m
        assert all(int(k) >= P for k in kv[m])                              # the prefix rows are never pad rows
    assert torch.equal(kv[2], torch.tensor([12 + 30, 12 + 2, 12 + 109, 12 + 2], dtype=torch.int32))


def test_text_length_artefact_and_get_model_message():
    from medical_tri_modal_pilot_amd.builder.models import get_model
    a, model = _model("tri_mbt_vmultivslt")
    enc = model.fusion_transformer
    kv = enc.key_lengths([torch.tensor([5, 0]), 49, torch.tensor([1, 0]) + 2], [(2, 9), (2, 49), (2, 8)], torch.device("cpu"))
    assert kv[0].tolist() == [12 + 4 + 5, 12 + 4] and kv[1] is None and kv[2].tolist() == [12, 14]     # txt_lengths == 1 -> 0
    a.model = "tri_mbt_vmulti"
    with pytest.raises(NotImplementedError, match="tri_mbt_vnoshnoavgtr.*tri_mbt_vmultivslt.*tri_mbt_vmulti2"):
        get_model(a)
