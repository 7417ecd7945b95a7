"""No GPU: the float64 model of the R-row head and the flexible combine (tests/row_head_model.py) against the torch module chain,
the seeded faults against the bounds tests/test_row_head_gpu.py uses, the new C entries, the staged-backward parameter list of the
flexible models, and ops.flex_combine on CPU tensors."""
import math

import pytest
import torch
import torch.nn as nn

from tests import row_head_model as M

F64 = torch.float64
HEAD_BOUND = 1e-4            # the project's fp32 bound, relative to the tensor's scale (tests/test_row_head_gpu.py)


def _torch_chain(c, T=None, ids=None, a=None, g=None):
    """The module chain of the models (LayerNorm of the source means, ie_demo appended, one fc_list per row or one for all) in
    float64 under autograd; with T: followed by the reference's flexible chain.  Returns (o | out, d blocks, parameter gradients
    [, d a])."""
    prm = [p.clone().requires_grad_() for p in c["params"]]
    demo = nn.Sequential(nn.Linear(2, 256), nn.LayerNorm(256), nn.ReLU()).double()
    ln = nn.LayerNorm(256).double()
    heads = [nn.Sequential(nn.Linear(512, 256), nn.LayerNorm(256), nn.ReLU(), nn.Linear(256, 1)).double() for _ in range(c["n_sets"])]
    mods = [demo[0], demo[1], ln] + [l for fc in heads for l in (fc[0], fc[1], fc[3])]
    slots = [q for m_ in mods for q in (m_.weight, m_.bias)]
    with torch.no_grad():
        for q, p in zip(slots, c["params"]):
            q.copy_(p)
    blocks = [b.double().requires_grad_() for b in c["blocks"]]
    rows = torch.stack([torch.stack([blocks[s][:, r] for s, r in srcs]).mean(0) for srcs in c["table"]])
    x = torch.cat([ln(rows), demo(torch.stack([c["age"], c["gender"]], 1).double()).unsqueeze(0).expand(len(rows), -1, -1)], dim=2)
    o = torch.stack([heads[m % c["n_sets"]](x[m]).squeeze(-1) for m in range(len(rows))])
    if T is None:
        got = torch.autograd.grad((o * c["w"].double()).sum(), blocks + slots)
        return o.detach(), list(got[:len(blocks)]), list(got[len(blocks):])
    a = a.double().requires_grad_()
    out = M.reference_flex_chain(o, a, T, ids, len(rows))
    got = torch.autograd.grad((out * g.double()).sum(), blocks + slots + [a])
    return out.detach(), list(got[:len(blocks)]), list(got[len(blocks):-1]), got[-1]


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape and M.rel(a, b) <= tol, M.rel(a, b)


@pytest.mark.parametrize("form", ["r4_block", "r4_multi2"])
def test_model_equals_the_torch_chain_multi_token_heads(form):
    c = M.case(form, 5)
    o, dblocks, grads = _torch_chain(c)
    _close(c["o"], o)
    for a, b in zip(c["dblocks"] + c["grads"], dblocks + grads):
        _close(a, b)


@pytest.mark.parametrize("form,T", [("r3_shared", 1.0), ("r3_shared", 10.0), ("r3_shared", 3.334), ("r2_shared", 1.0)])
def test_model_equals_the_torch_chain_flexible_heads(form, T):
    """head + flexible combine: the closed-form gradients against autograd of masked_fill(-1e9) / softmax / candidate sums / gather"""
    B = 9
    c = M.case(form, B)
    R = len(c["table"])
    gen = torch.Generator().manual_seed(11)
    a, g = 0.7 * torch.randn(R, generator=gen, dtype=F64), torch.randn(B, generator=gen, dtype=F64)
    ids = M.mixed_ids(B, 0, 4 if R == 3 else 2)
    table = M.TRI_PRESENT if R == 3 else M.BI_PRESENT
    out, p = M.flex_forward(c["o"], a, T, ids, table)
    d_o, d_a, d_a_abs = M.flex_backward(c["o"], a, T, ids, table, g)
    dblocks, grads = M.head_backward(c["cache"], d_o)
    assert bool((p[~M._present(ids, table, R)] == 0).all())
    t_out, t_dblocks, t_grads, t_da = _torch_chain(c, T, ids, a, g)
    _close(out, t_out)
    # d a: autograd's softmax backward subtracts terms of this size (row_head_model.flex_da_terms)
    scale = M.flex_da_terms(c["o"], a, T, ids, table, g)
    assert bool(((d_a - t_da).abs() <= 1e-12 * scale).all()), ((d_a - t_da).abs() / scale)
    for x, y in zip(dblocks + grads, t_dblocks + t_grads):
        _close(x, y)


def test_seeded_faults_exceed_the_gpu_bounds():
    """every seeded fault of the model moves a result by far more than the bound the GPU tests hold the kernels to"""
    c = M.case("r4_multi2", 5)
    blocks = [b.double() for b in c["blocks"]]
    f = M.head_forward(blocks, c["table"], c["age"].double(), c["gender"].double(), c["params"], fault="source_sum")
    # LayerNorm removes the scale of its input but for eps: at O(1) rows a sum in place of the mean is no measurable fault ...
    assert M.rel(f["o"], c["o"]) < HEAD_BOUND
    # ... so the GPU test also runs rows whose variance is near eps, where it is one
    small = M.case("r4_multi2", 5, scale=M.SMALL_SCALE)
    f = M.head_forward([b.double() for b in small["blocks"]], small["table"], small["age"].double(), small["gender"].double(),
                       small["params"], fault="source_sum")
    assert M.rel(f["o"], small["o"]) > 100 * HEAD_BOUND
    db, _ = M.head_backward(c["cache"], c["w"].double(), fault="no_div_nsrc")
    err, ref = (db[1] - c["dblocks"][1]).abs(), c["dblocks"][1].abs()
    assert bool((err > HEAD_BOUND * ref.max() + 2.0 ** -8 * ref).any()) and M.rel(db[1], c["dblocks"][1]) > 100 * HEAD_BOUND
    s = M.case("r3_shared", 5)
    _, gr = M.head_backward(s["cache"], s["w"].double(), fault="shared_row0")
    assert all(M.rel(a, b) > 100 * HEAD_BOUND for a, b in zip(gr[6:], s["grads"][6:]))
    for R, T in ((3, 3.334), (2, 1.0)):
        r = M.flex_reference(R, 8, T)
        o, a, g = r["o"].double(), r["a"].double(), r["g"].double()
        assert r["bound"] < 1e-5                                           # (the bound itself is an fp32 rounding level)
        for fault in ("absent_weight", "softmax_all"):
            out, _ = M.flex_forward(o, a, T, r["ids"], r["table"], fault)
            d_o, _, _ = M.flex_backward(o, a, T, r["ids"], r["table"], g, fault)
            assert M.rel(out, r["out"]) > 100 * r["bound"] and M.rel(d_o, r["d_o"]) > 100 * r["bound"], fault
    r = M.flex_reference(3, 8, 3.334)
    _, d_a, _ = M.flex_backward(r["o"].double(), r["a"].double(), 3.334, r["ids"], r["table"], r["g"].double(), "no_temperature")
    assert bool(((d_a - r["d_a"]).abs() > 100 * r["bound"] * r["d_a_abs"]).all())


NEW_SYMBOLS = ["mtmp_headr_fwd", "mtmp_headr_bwd", "mtmp_headr_ws_floats", "mtmp_headr_bwd_ws_floats", "mtmp_flex_combine_fwd",
               "mtmp_flex_combine_bwd"]


def test_new_symbols_are_declared_exported_and_abi_stays_6():
    from medical_tri_modal_pilot_amd import _lib
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.mtmp_abi_version() == 6
    assert lib.mtmp_headr_ws_floats(4, 256) == 4 * 256 * 769 and lib.mtmp_headr_bwd_ws_floats(2, 5) == 5 * 256 * 9
    assert lib.mtmp_headr_ws_floats(3, 7) == lib.mtmp_head3_ws_floats(7)


def test_bad_tables_are_refused_by_message():
    """argument checks run before anything touches the device: a source row that feeds two head rows, a source that is not there,
    n_sets that is neither 1 nor R, B past 256"""
    import ctypes
    from medical_tri_modal_pilot_amd import _lib, ops
    lib = _lib.lib()
    buf = (ctypes.c_float * 4096)()
    base = (ctypes.addressof(buf) + 15) & ~15
    ptrs = lambda n: (ctypes.c_void_p * n)(*[base] * n)
    LL, I = ctypes.c_longlong, ctypes.c_int

    def fwd(n_blocks=1, rows=(4,), R=2, n_src=(1, 1), src=((0, 0), (0, 1)), n_sets=1, B=2):
        flat = [0] * (6 * R)
        for m, (s, r) in enumerate(src):
            flat[6 * m], flat[6 * m + 1] = s, r
        return lib.mtmp_headr_fwd(0, n_blocks, ptrs(n_blocks), (LL * n_blocks)(*[1024] * n_blocks), (LL * n_blocks)(*[256] * n_blocks),
                                  (I * n_blocks)(*rows), R, (I * R)(*n_src), (I * (6 * R))(*flat), base, base, ptrs(30), n_sets, base,
                                  base, B, 1e-5, None)

    for kw, word in ((dict(src=((0, 1), (0, 1))), "more than one head row"), (dict(src=((0, 0), (0, 4))), "not there"),
                     (dict(src=((1, 0), (0, 1))), "not there"), (dict(n_sets=3), "n_sets"), (dict(B=257), "B=257"),
                     (dict(n_src=(1, 4)), "sources"), (dict(rows=(5,)), "rows")):
        assert fwd(**kw) == 1, kw
        assert word in lib.mtmp_last_error().decode(), (kw, lib.mtmp_last_error())
    with pytest.raises(ValueError, match="more than one head row"):
        ops._row_table((((0, 0),), ((0, 0),)), [torch.zeros(2, 4, 256)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.RowHeadFn.apply(torch.zeros(2, 4, 256), torch.zeros(2), torch.zeros(2), (((0, 0),), ((0, 1),)), *([torch.zeros(1)] * 12))


def _model(name, input_types):
    from medical_tri_modal_pilot_amd.builder.models import get_model
    from medical_tri_modal_pilot_amd.control.config import parse_args
    a = parse_args(["--input-types", input_types, "--model", name, "--modality-inclusion", "train-missing_test-missing",
                    "--lr-init", "1e-5", "--batch-size", "4", "--transformer-num-layers", "2", "--imgtxt-time", "1",
                    "--mbt-only-vslt", "1", "--dropout", "0.0", "--compute-dtype", "fp32"])
    a.device, a.output_dim = torch.device("cpu"), 1
    return a, get_model(a)(a)


@pytest.mark.parametrize("name", ["tri_mbt_vflexible", "tri_mbt_vflexible2", "tri_mbt_vflexible3"])
def test_head_stage_of_the_flexible_models_names_flexibleavg(name):
    """a staged step differentiates with respect to exactly this list (trainer._staged_step): without flexibleavg in it the learned
    weights never receive a gradient under --ddp 1"""
    from medical_tri_modal_pilot_amd import tuning
    _, model = _model(name, "vslt_img_txt")
    assert tuning.HIP_ROW_HEAD in (True, False) and model.head_fusable == tuning.HIP_ROW_HEAD
    head = model.backward_stage_params(1, 2, head=True)
    assert sum(q is model.flexibleavg for q in head) == 1
    assert not any(q is model.flexibleavg for q in model.backward_stage_params(0, 1, head=False))
    assert len(head) == len({id(q) for q in head})
    hot = {id(q) for _, q in model.hot_parameters()}
    assert id(model.flexibleavg) in hot


@pytest.mark.parametrize("R,T", [(3, 1.0), (3, 10.0), (3, 3.334), (2, 1.0)])
def test_flex_combine_on_cpu_tensors_is_the_reference_chain(R, T):
    from medical_tri_modal_pilot_amd import ops
    r = M.flex_reference(R, 8, T)
    o, a = r["o"].double().requires_grad_(), r["a"].double().requires_grad_()
    ids = r["ids"] & 3
    table = ops.FLEX_TRI_TABLE if R == 3 else ops.FLEX_BI_TABLE
    assert table == (M.TRI_PRESENT if R == 3 else M.BI_PRESENT)
    got = ops.flex_combine(o, a.reshape(R, 1), T, ids, table)
    want = M.reference_flex_chain(o, a, T, ids, R)
    assert got.shape == want.shape and M.rel(got, want) <= 1e-15
    d_got, d_want = torch.autograd.grad((got * r["g"].double()).sum(), [o, a]), torch.autograd.grad((want * r["g"].double()).sum(), [o, a])
    scale = M.flex_da_terms(r["o"].double(), r["a"].double(), T, r["ids"], r["table"], r["g"].double())
    assert M.rel(d_got[0], d_want[0]) <= 1e-14
    assert bool(((d_got[1] - d_want[1]).abs() <= 1e-13 * scale).all())     # (the same chain twice: the same roundings)
    _close(got.detach(), r["out"], 1e-14)                                  # ... which is the model's closed form
    assert bool(((d_got[1] - r["d_a"]).abs() <= 1e-12 * scale).all())
    assert ops._table_bits(table, R) == sum(1 << (4 * p + m) for p in range(4) for m in range(R) if table[p][m])
