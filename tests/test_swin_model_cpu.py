"""Pins tests/swin_model.py -- the float64 references of the Swin image-encoder kernels, the additive table, the launch arithmetic
the cases of tests/test_swin_model_gpu.py are derived from, and every condition its probes rely on -- against independent
formulations (the oracle's window attention and torch autograd, F.layer_norm, F.conv2d, the package's own table builder), so that
the references cannot be wrong together with the kernels.  Runs without a GPU."""
import time

import pytest
import torch
import torch.nn.functional as F

from oracle import tri_mbt_oracle as O
from tests import swin_model as S

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
TIGHT = 1e-11            # two float64 formulations of one expression
T0 = time.time()


def _d(t):
    return None if t is None else t.to(F64)


# ------------------------------------------------------------------------------------------ window attention against the oracle
ATTN_SHAPES = [(14, 14), (14, 21), (21, 14), (7, 7), (5, 5), (8, 8), (13, 13), (9, 16), (16, 9)]
ATTN_CASES = [(H, W, s) for H, W in ATTN_SHAPES for s in (0, 3)] + [(14, 14, 1), (14, 14, 6)]


def _to_map(t, B, H, W, sh, sw):
    """the oracle's own way back from [B nW, 49, c] to the map (reverse windows, reverse cyclic shift, unpad)"""
    Hp, Wp = -(-H // 7) * 7, -(-W // 7) * 7
    t = t.view(B, Hp // 7, Wp // 7, 7, 7, -1).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, -1)
    if sh + sw > 0:
        t = torch.roll(t, shifts=(sh, sw), dims=(1, 2))
    return t, t[:, :H, :W]


@pytest.mark.parametrize("H,W,shift", ATTN_CASES)
def test_window_attn_model_vs_oracle_and_its_autograd(monkeypatch, H, W, shift):
    """o, dqkv, dtab (scattered into relative_position_bias_table) and dbias of the float64 model against O.swin_window_attention in
    float64 with an identity output projection: the qkv map is the oracle's own projection of a random input, captured with its
    gradient; the pad tokens' rows of that gradient are dbias, and dbias + column sums of dqkv the whole qkv.bias gradient"""
    heads, B = 2, 2
    C = heads * S.DH
    g = torch.Generator().manual_seed(100 * H + W + shift)
    x = torch.randn(B, H, W, C, generator=g, dtype=F64)
    sd = {"a.qkv.weight": (torch.randn(3 * C, C, generator=g) / C ** 0.5).to(F64).requires_grad_(),
          "a.qkv.bias": (0.5 * torch.randn(3 * C, generator=g)).to(F64).requires_grad_(),
          "a.proj.weight": torch.eye(C, dtype=F64), "a.proj.bias": torch.zeros(C, dtype=F64),
          "a.relative_position_bias_table": S.rpb_table(heads, g).to(F64).requires_grad_()}
    d_out = torch.randn(B, H, W, C, generator=g, dtype=F64)
    seen, linear = [], F.linear

    def spy(inp, w, b=None):
        y = linear(inp, w, b)
        if y.shape[-1] == 3 * C and y.requires_grad:
            y.retain_grad()
            seen.append(y)
        return y

    monkeypatch.setattr(O.F, "linear", spy)
    o_ref = O.swin_window_attention(sd, "a", x, heads, shift)
    (o_ref * d_out).sum().backward()
    monkeypatch.undo()
    assert len(seen) == 1
    Hp, Wp = -(-H // 7) * 7, -(-W // 7) * 7
    sh, sw = (0 if 7 >= Hp else shift), (0 if 7 >= Wp else shift)
    qkv_full, qkv_map = _to_map(seen[0].detach(), B, H, W, sh, sw)
    dq_full, dq_map = _to_map(seen[0].grad, B, H, W, sh, sw)
    padded = (Hp, Wp) != (H, W)
    bias32 = sd["a.qkv.bias"].detach().float()
    assert torch.equal(bias32.double(), sd["a.qkv.bias"].detach())                     # (an fp32 value: the model's rounding is a no-op)
    m = S.window_attn_model(qkv_map, sd["a.relative_position_bias_table"].detach().float(), heads, shift,
                            bias32 if padded else None, d_out, dt=F32, ft=F64)         # (the float64 map is taken as it is)
    assert qkv_map.shape == (B, H, W, 3 * C) and torch.equal(qkv_full[:, :H, :W], qkv_map)
    assert S.err(m["o"], o_ref.detach()) < TIGHT
    assert S.err(m["dqkv"], dq_map) < TIGHT
    assert S.err(S.scatter_dtab(m["dtab"], heads), sd["a.relative_position_bias_table"].grad) < 1e-10
    pad_rows = dq_full.sum((0, 1, 2)) - dq_map.sum((0, 1, 2))
    assert torch.equal(m["dbias"][:C], torch.zeros(C, dtype=F64))
    if padded:
        assert S.err(m["dbias"][C:], pad_rows[C:]) < 1e-10
        assert float(pad_rows[:C].abs().max()) < 1e-12                                 # (a pad query's d_out is zero)
    else:
        assert not m["dbias"].any()
    assert S.err(m["dbias"] + m["dqkv"].sum((0, 1, 2)), sd["a.qkv.bias"].grad) < 1e-10
    # pad queries' rows of dtab and, at shift 0, the planes of the other window types are exactly zero
    if shift == 0 or sh + sw == 0:
        assert not m["dtab"][1:].any()
    pix, types = S.window_geometry(H, W, shift)[0], S.window_types(H, W, shift)
    for t in range(4):
        if bool((types == t).any()):
            rows = (pix[types == t] < 0).all(0)                                        # slots that hold a pad token in every window of the type
            assert not m["dtab"][t][:, :49][:, rows].any()
    assert not m["dtab"][:, :, 49:].any() and not m["dtab"][..., 49:].any()


def test_one_window_axis_is_not_shifted():
    """swin_transformer.py:155-160: the geometry of a 7 x 7 (5 x 5) map at shift 3 is that of shift 0"""
    for H in (7, 5):
        a, b = S.window_geometry(H, H, 3), S.window_geometry(H, H, 0)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == (0, 0)
    assert S.window_geometry(7, 14, 3)[2] == (0, 3)
    assert S.window_types(7, 14, 3).tolist() == [0, 1]                                  # (masked along the shifted axis only)
    assert S.window_types(14, 21, 3).tolist() == [0, 0, 1, 2, 2, 3] and S.window_types(21, 14, 3).tolist() == [0, 1, 0, 1, 2, 3]
    assert S.window_types(14, 21, 0).tolist() == [0] * 6 and S.window_types(15, 15, 3).tolist() == [0, 0, 1, 0, 0, 1, 2, 2, 3]


@pytest.mark.parametrize("shift", [0, 1, 3, 6])
def test_table_model_vs_the_package_table(shift):
    from medical_tri_modal_pilot_amd.builder.models.src.swin_transformer import ShiftedWindowAttention
    heads = 3
    att = ShiftedWindowAttention(96, [7, 7], [shift, shift], heads)
    rpb = S.rpb_table(heads, torch.Generator().manual_seed(5))
    with torch.no_grad():
        att.relative_position_bias_table.copy_(rpb)
    want = att.additive_table(shift, F32, "cpu")
    got = S.table_model(rpb, heads, shift, F32)
    assert torch.equal(got[:, :, :49, :49], want[:, :, :49, :49]) and torch.equal(got, want)
    acc = att.additive_table(shift, F32, "cpu", acc_order=True)
    undone = torch.empty_like(acc)
    for g in range(4):
        for h in range(2):
            for j in range(8):
                undone[..., 16 * g + (j & 3) + 8 * (j >> 2) + 4 * h] = acc[..., 16 * g + 8 * h + j]
    assert torch.equal(undone, got) and torch.equal(S.table_model(rpb, heads, shift, F32, acc_order=True), acc)
    assert torch.equal(S.table_model(rpb, heads, shift, BF16), want.to(BF16).float())
    assert torch.equal(S.rel_index(), O.swin_relative_position_index(7))


# ------------------------------------------------------------------------------------------ LayerNorm, GELU
@pytest.mark.parametrize("rows,C", [(1, 8), (5, 96), (7, 1536)])
def test_ln_models_vs_layer_norm_and_autograd(rows, C):
    p = S.ln_inputs(rows, C, F32, seed=1)
    x = _d(p["x"]).requires_grad_()
    w, b = _d(p["w"]).requires_grad_(), _d(p["b"]).requires_grad_()
    y = F.layer_norm(x, (C,), w, b, 1e-5)
    (y * _d(p["dy"])).sum().backward()
    assert S.err(S.ln_rows_model(p["x"], p["w"], p["b"], dt=F32, ft=F64)["y"], y.detach()) < TIGHT
    m = S.ln_rows_bwd_model(p["x"], p["w"], p["dy"], dt=F32, ft=F64)
    assert S.err(m["dx"], x.grad) < 1e-10 and S.err(m["dw"], w.grad) < 1e-10 and S.err(m["db"], b.grad) < 1e-10
    part = S.ln_rows_bwd_model(p["x"], p["w"], p["dy"], keep=(rows - 1, rows), dt=F32, ft=F64)
    assert S.err(part["db"], _d(p["dy"])[rows - 1]) < TIGHT and S.err(part["dx"], x.grad) < 1e-10


@pytest.mark.parametrize("n,H,W,Cs", S.MERGE_CASES)
def test_merge_mode_vs_the_cat_form(n, H, W, Cs):
    p = S.merge_inputs(n, H, W, Cs, F32)
    x = _d(p["x"])
    cat = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1)
    want = F.layer_norm(cat, (4 * Cs,), _d(p["w"]), _d(p["b"]), 1e-5)
    got = S.ln_rows_model(p["x"], p["w"], p["b"], merge_hw=(H, W), dt=F32, ft=F64)["y"]
    assert got.shape == (n, H // 2, W // 2, 4 * Cs) and S.err(got, want) < TIGHT


def test_gelu_models():
    p = S.gelu_inputs(4104, F32)
    x = _d(p["x"]).requires_grad_()
    y = F.gelu(x)
    (y * _d(p["dy"])).sum().backward()
    assert float(p["x"].abs().max()) == 6.0
    assert S.err(S.gelu_model(p["x"], dt=BF16, ft=F64)["y"], y.detach()) < TIGHT
    assert S.err(S.gelu_grad_model(p["x"], p["dy"], dt=BF16, ft=F64)["dx"], x.grad) < 1e-10
    # the bf16 chain's derivative is the derivative of the bf16 chain's form
    xb = p["x"].double().requires_grad_()
    (xb * torch.sigmoid(xb * (1.5957691216 + 0.0713548163 * xb * xb))).sum().backward()
    assert S.err(S.gelu_grad_model(p["x"], torch.ones_like(p["x"]), dt=BF16, ft=F32)["dx"], xb.grad) < 1e-5


# ------------------------------------------------------------------------------------------ block pieces against the oracle's
@pytest.mark.parametrize("M,C", [(5, 96), (33, 192)])
def test_mlp_and_ln_linear_models_vs_torch(M, C):
    p = S.mlp_inputs(M, C, F32, seed=2)
    x = _d(p["x"])
    h = F.layer_norm(x, (C,), _d(p["ln_w"]), _d(p["ln_b"]), 1e-5)
    f = F.linear(F.gelu(F.linear(h, _d(p["w1"]), _d(p["b1"]))), _d(p["w2"]), _d(p["b2"]))
    args = [p[k] for k in ("x", "ln_w", "ln_b")] + [1e-5] + [p[k] for k in ("w1", "b1", "w2", "b2")]
    assert S.err(S.swin_mlp_model(*args, dt=BF16, ft=F64)["y"], x + f) < TIGHT
    rs = S.row_scales(M, 4)
    want = x + _d(rs)[torch.arange(M) // 4][:, None] * f
    assert S.err(S.swin_mlp_model(*args, rs, 4, dt=BF16, ft=F64)["y"], want) < TIGHT
    q = S.ln_linear_inputs(M, C, 288, F32, seed=2)
    h = F.layer_norm(_d(q["x"]), (C,), _d(q["ln_w"]), _d(q["ln_b"]), 1e-5)
    assert S.err(S.ln_linear_model(q["x"], q["ln_w"], q["ln_b"], 1e-5, q["w"], q["bias"], dt=BF16, ft=F64)["y"],
                 F.linear(h, _d(q["w"]), _d(q["bias"]))) < TIGHT
    assert S.err(S.ln_linear_model(q["x"], q["ln_w"], q["ln_b"], 1e-5, q["w"], None, dt=BF16, ft=F64)["y"], F.linear(h, _d(q["w"]))) < TIGHT


@pytest.mark.parametrize("n,H,W,shift", S.BLOCK_CASES + S.BLOCK_PAD_CASES)
def test_attn_block_model_vs_oracle(n, H, W, shift):
    C, heads = 96, 3
    p = S.block_inputs(n, H, W, C, F32, seed=3)
    sd = {"a.qkv.weight": _d(p["wqkv"]), "a.qkv.bias": _d(p["bqkv"]), "a.proj.weight": _d(p["wproj"]), "a.proj.bias": _d(p["bproj"]),
          "a.relative_position_bias_table": _d(p["rpb"])}
    x = _d(p["x"])
    h = F.layer_norm(x, (C,), _d(p["ln_w"]), _d(p["ln_b"]), 1e-5)
    branch = O.swin_window_attention(sd, "a", h, heads, shift)
    args = [p["x"], p["ln_w"], p["ln_b"], 1e-5, p["wqkv"], p["bqkv"], p["rpb"], heads, shift, p["wproj"], p["bproj"]]
    # (dt = fp32: the table's values are operands of the compute type, and the oracle's table is the fp32 one)
    assert S.err(S.attn_block_model(*args, dt=F32, ft=F64)["y"], x + branch) < 1e-10
    rs = S.row_scales(n, 1)
    got = S.attn_block_model(*args, rs, dt=F32, ft=F64)["y"]
    assert S.err(got, x + _d(rs).view(-1, 1, 1, 1) * branch) < 1e-10
    if n > 1:
        assert torch.equal(got[1], x[1])                                               # (the image with factor 0)


@pytest.mark.parametrize("n,H,W", S.STEM_CASES)
def test_stem_model_vs_conv2d(n, H, W):
    p = S.stem_inputs(n, H, W)
    y = F.conv2d(_d(p["img"]), _d(p["w"]), _d(p["bias"]), stride=4).permute(0, 2, 3, 1)
    y = F.layer_norm(y, (96,), _d(p["ln_w"]), _d(p["ln_b"]), 1e-5)
    assert S.err(S.stem_model(*[p[k] for k in ("img", "w", "bias", "ln_w", "ln_b")], dt=F32, ft=F64)["y"], y) < TIGHT
    order = torch.arange(n - 1, -1, -1, dtype=torch.int32)
    assert S.err(S.stem_model(*[p[k] for k in ("img", "w", "bias", "ln_w", "ln_b")], order, dt=F32, ft=F64)["y"], y.flip(0)) < TIGHT


def test_launch_arithmetic_of_the_cases():
    assert [S.ln_rpw(C) for C in S.LN_WIDTHS] == [4, 4, 2, 1, 1, 1]
    assert S.ln_bwd_slab_rows(16384, 96) == 1024 and S.ln_bwd_slab_rows(16385, 96) == 1024 and S.ln_bwd_slab_rows(17, 96) == 2
    assert S.ln_bwd_slab_rows(4097, 768) == 1024 and S.ln_bwd_slab_rows(1, 1536) == 1
    for C, rows in S.LN_WRAP:                                                           # 4096 workgroups of 4 waves of RPW rows
        assert rows == 4096 * 4 * S.ln_rpw(C) + 1
    for C, rows in S.LN_BWD_WRAP:
        assert rows == 1024 * 4 * S.ln_rpw(C) + 1
    assert S.GELU_N[-1] == 8192 * 256 * 8 + 8
    assert (1 * 1 * 1 * 3) % 4 != 0                                                     # (1,7,7,3): dead waves in the last workgroup


# ------------------------------------------------------------------------------------------ every case's bound
def _bounds_ok(e, bf16_out, names=None):
    for k, v in e.items():
        if names is None or k in names:
            b = S.bound(v, bf16_out)
            assert b <= S.PROBE_BOUND, (k, v, b)


@pytest.mark.parametrize("dt", S.DTS, ids=S.dt_name)
def test_bounds_of_the_row_cases(dt):
    for C in S.LN_WIDTHS:
        for rows in sorted(set(S.ln_rows_cases(C)) | set(S.ln_bwd_rows_cases(C))):
            p = S.ln_inputs(rows, C, dt)
            _bounds_ok(S.e_chain_of(S.ln_rows_model, p["x"], p["w"], p["b"], dt=dt)[1], dt == BF16)
            e = S.e_chain_of(S.ln_rows_bwd_model, p["x"], p["w"], p["dy"], dt=dt)[1]
            _bounds_ok(e, dt == BF16, ("dx",))
            _bounds_ok(e, False, ("dw", "db"))
    for C, rows in S.LN_WRAP + S.LN_BWD_WRAP:
        p = S.ln_inputs(rows, C, dt)
        _bounds_ok(S.e_chain_of(S.ln_rows_model, p["x"], p["w"], p["b"], dt=dt)[1], dt == BF16)
        e = S.e_chain_of(S.ln_rows_bwd_model, p["x"], p["w"], p["dy"], dt=dt)[1]
        _bounds_ok(e, dt == BF16, ("dx",))
        _bounds_ok(e, False, ("dw", "db"))
    for c in S.MERGE_CASES:
        p = S.merge_inputs(*c, dt)
        _bounds_ok(S.e_chain_of(S.ln_rows_model, p["x"], p["w"], p["b"], merge_hw=c[1:3], dt=dt)[1], dt == BF16)
    for n in S.GELU_N:
        p = S.gelu_inputs(n, dt)
        _bounds_ok(S.e_chain_of(S.gelu_model, p["x"], dt=dt)[1], dt == BF16)
        _bounds_ok(S.e_chain_of(S.gelu_grad_model, p["x"], p["dy"], dt=dt)[1], dt == BF16)
    for c in S.STEM_CASES:
        p = S.stem_inputs(*c)
        _bounds_ok(S.e_chain_of(S.stem_model, *[p[k] for k in ("img", "w", "bias", "ln_w", "ln_b")], dt=dt)[1], dt == BF16)


@pytest.mark.parametrize("dt", S.DTS, ids=S.dt_name)
@pytest.mark.parametrize("c", S.WATTN_CASES + S.WATTN_PAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_bounds_of_the_window_attention_cases(c, dt):
    n, H, W, heads, shift = c
    p = S.attn_inputs(n, H, W, heads, dt, pad=H % 7 != 0 or W % 7 != 0)
    _, e = S.e_chain_of(S.window_attn_model, p["qkv"], p["rpb"], heads, shift, p["bias"], p["d_out"], dt=dt)
    _bounds_ok(e, dt == BF16, ("o", "dqkv"))
    _bounds_ok(e, False, ("dtab",) + (("dbias",) if p["bias"] is not None else ()))


@pytest.mark.parametrize("C", [96, 192])
def test_bounds_of_the_fused_cases(C):
    for M in S.M_EDGES:
        p = S.mlp_inputs(M, C)
        args = [p[k] for k in ("x", "ln_w", "ln_b")] + [1e-5] + [p[k] for k in ("w1", "b1", "w2", "b2")]
        _bounds_ok(S.e_chain_of(S.swin_mlp_model, *args, dt=BF16)[1], True)
        _bounds_ok(S.e_chain_of(S.swin_mlp_model, *args, S.row_scales(M, 49), 49, dt=BF16)[1], True)
        for N in (32, 288, 576):
            for bias in (True, False):
                q = S.ln_linear_inputs(M, C, N, bias=bias)
                _bounds_ok(S.e_chain_of(S.ln_linear_model, q["x"], q["ln_w"], q["ln_b"], 1e-5, q["w"], q["bias"], dt=BF16)[1], True)
    for n, H, W, shift in S.BLOCK_CASES + S.BLOCK_PAD_CASES:
        p = S.block_inputs(n, H, W, C)
        args = [p["x"], p["ln_w"], p["ln_b"], 1e-5, p["wqkv"], p["bqkv"], p["rpb"], C // 32, shift, p["wproj"], p["bproj"]]
        _bounds_ok(S.e_chain_of(S.attn_block_model, *args, dt=BF16)[1], True)
        _bounds_ok(S.e_chain_of(S.attn_block_model, *args, S.row_scales(n, 1), dt=BF16)[1], True)


# ------------------------------------------------------------------------------------------ the probes, on the reference alone
def _probe_ok(lost, ref, e_chain, bf16_out):
    b, loss = S.bound(e_chain, bf16_out), S.err(lost, ref)
    assert b <= S.PROBE_BOUND and loss >= S.PROBE_LOSS, (b, loss)


@pytest.mark.parametrize("C", [96, 192])
def test_probe_last_hidden_panel_of_swin_mlp(C):
    p = S.mlp_probe_inputs(C)
    args = lambda q: [q[k] for k in ("x", "ln_w", "ln_b")] + [1e-5] + [q[k] for k in ("w1", "b1", "w2", "b2")]
    assert not p["w2"][:, :4 * C - S.MLP_PANEL[C]].any() and S.MLP_PANEL[C] * (6 if C == 96 else 24) == 4 * C
    ref, e = S.e_chain_of(S.swin_mlp_model, *args(p), dt=BF16)
    lost = S.swin_mlp_model(*args(S.mlp_probe_lost(p)), dt=BF16, ft=F64)
    _probe_ok(lost["y"], ref["y"], e["y"], True)


@pytest.mark.parametrize("dt", S.DTS, ids=S.dt_name)
def test_probe_last_window_row_and_column(dt):
    c = S.CORNER_PROBE
    p = S.corner_probe_inputs(dt)
    ref, e = S.e_chain_of(S.window_attn_model, p["qkv"], p["rpb"], c["heads"], c["shift"], None, p["d_out"], dt=dt)
    types = S.window_types(c["H"], c["W"], c["shift"])
    assert [int(types[w]) for w, _ in S.corner_probe_windows()] == [1, 2, 3]
    inside = torch.zeros(c["H"], c["W"], dtype=torch.bool)
    for w, _ in S.corner_probe_windows():
        tok = S.window_tokens(c["H"], c["W"], c["shift"], w)
        inside |= tok
        for name, bf in (("o", dt == BF16), ("dqkv", dt == BF16)):
            lost = ref[name].clone()
            lost[:, tok] = 0
            _probe_ok(lost, ref[name], e[name], bf)
    assert not ref["o"][:, ~inside].any()                                               # nothing but the three windows' outputs
    C = c["heads"] * S.DH
    assert not ref["dqkv"][:, ~inside][..., :2 * C].any()                               # (dv of the other windows: p^T d_out = 0 as well)
    assert not ref["dtab"][0].any() and all(bool(ref["dtab"][t].any()) for t in (1, 2, 3))
    _probe_ok(torch.zeros_like(ref["dtab"]), ref["dtab"], e["dtab"], False)


@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("dt", S.DTS, ids=S.dt_name)
def test_probe_pad_keys(dt, shift):
    c = S.PAD_PROBE
    p = S.pad_probe_inputs(dt, shift)
    run = lambda q, ft: S.window_attn_model(q["qkv"], q["rpb"], c["heads"], shift, q["bias"], q["d_out"], dt=dt, ft=ft)
    ref, ch = run(p, F64), run(p, F32)
    lost = run(S.pad_probe_lost(p), F64)
    assert not lost["o"].any()
    _probe_ok(lost["o"], ref["o"], S.err(ch["o"], ref["o"]), dt == BF16)
    _probe_ok(torch.zeros_like(ref["dbias"]), ref["dbias"], S.err(ch["dbias"], ref["dbias"]), False)
    assert not ref["dbias"][:c["heads"] * S.DH].any()


@pytest.mark.parametrize("dt", S.DTS, ids=S.dt_name)
def test_probe_second_trip_of_layernorm_rows_bwd(dt):
    p = S.ln_bwd_probe_inputs(dt)
    rows, C = S.LN_BWD_PROBE["rows"], S.LN_BWD_PROBE["C"]
    assert S.ln_bwd_slab_rows(rows, C) == 1024 and 1024 * 4 * S.ln_rpw(C) == 16384 < rows
    ref, e = S.e_chain_of(S.ln_rows_bwd_model, p["x"], p["w"], p["dy"], dt=dt)
    first = S.ln_rows_bwd_model(p["x"], p["w"], p["dy"], keep=(0, 16384), dt=dt, ft=F64)      # a single-trip kernel's sums
    assert not first["dw"].any() and not first["db"].any()
    for name in ("dw", "db"):
        _probe_ok(first[name], ref[name], e[name], False)


def test_wall_time_is_reported():
    print(f"test_swin_model_cpu.py: {time.time() - T0:.1f} s up to here")
