"""Pins tests/gemm_model.py -- the float64 references of the projection GEMMs, the key-norm table, the sign-bit decoder, the launch
arithmetic the cases of tests/test_gemm_model_gpu.py are derived from, and every condition its one-tile probes rely on -- against
independent formulations, so that the references cannot be wrong together with the kernels.  Runs without a GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import tri_mbt_oracle as O
from tests import gemm_model as G

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
TIGHT = 1e-11            # two float64 formulations of one expression


def _d(t):
    return None if t is None else t.to(F64)


# ------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("M,N,act", [(1, 64, None), (33, 768, None), (130, 1024, "relu")])
def test_ln_gemm_model_vs_oracle(M, N, act):
    """O.custom_layernorm + F.linear (+ ReLU) at float64; the statistics against row_kernels_model.ln_stats' definition"""
    p = G.ln_gemm_inputs(M, N, F32, seed=1)
    x, gam, bet, w, b = (_d(p[k]) for k in ("x", "gamma", "beta", "w", "bias"))
    xn = O.custom_layernorm(x, gam, bet)
    y = F.linear(xn, w, b)
    y = torch.relu(y) if act else y
    m = G.ln_gemm_model(p["x"], p["gamma"], p["beta"], p["w"], p["bias"], act, dt=F32, ft=F64)
    assert G.err(m["xn"], xn) < TIGHT and G.err(m["y"], y) < TIGHT
    assert G.err(m["mean"], x.mean(-1)) < TIGHT and G.err(m["rstd"], 1 / (x.std(-1) + 1e-6)) < TIGHT
    assert ("knorm" in m) == (N == 768)
    m0 = G.ln_gemm_model(p["x"], p["gamma"], p["beta"], p["w"], None, act, dt=F32, ft=F64)
    y0 = F.linear(xn, w)
    assert G.err(m0["y"], torch.relu(y0) if act else y0) < TIGHT


@pytest.mark.parametrize("B,N", [(3, 45), (2, 133), (1, 32), (5, 7), (1, 1)])
def test_key_norm_model_is_the_table_of_test_key_norms_table(B, N):
    """the definition tests/test_gpu_parity.py::test_key_norms_table holds mtmp_key_norms to: max ||k_h|| per block of 32 rows"""
    g = torch.Generator().manual_seed(11)
    qkv = (torch.randn(B, N, 768, generator=g) * torch.rand(B, N, 1, generator=g) * 3).to(F64)
    k = qkv[..., 256:512].reshape(B * N, 4, 64).norm(dim=-1)
    nblk = (B * N + 31) // 32
    want = torch.stack([k[32 * i:32 * i + 32].max(0).values for i in range(nblk)])
    got = G.knorm_model(qkv.reshape(B * N, 768))
    assert got.shape == want.shape and G.err(got, want) < TIGHT


@pytest.mark.parametrize("act", G.ACTS)
@pytest.mark.parametrize("M,N,K", [(1, 32, 8), (65, 160, 72), (50, 96, 200)])
def test_gemm_nt_model_vs_torch(M, N, K, act):
    p = G.nt_inputs(M, N, K, F32, seed=2, res=True, gate=True, row_scale=49, lda=K + 16, ldr=N + 8)
    a, w, b, res, gate, rsc = (_d(p[k]) for k in ("a", "w", "bias", "res", "gate", "row_scale"))
    v = F.linear(a, w, b)
    v = torch.relu(v) if act == "relu" else F.gelu(v) if act == "gelu" else v            # (F.gelu: the exact, erf form)
    assert G.err(G.gemm_nt_model(p["a"], p["w"], p["bias"], act=act, dt=F32, ft=F64)["y"], v) < TIGHT
    assert G.err(G.gemm_nt_model(p["a"], p["w"], None, act=act, dt=F32, ft=F64)["y"],
                 torch.relu(F.linear(a, w)) if act == "relu" else F.gelu(F.linear(a, w)) if act == "gelu" else F.linear(a, w)) < TIGHT
    full = torch.where(gate > 0, v * 0.75, torch.zeros_like(v)) * rsc[torch.arange(M) // 49][:, None] + res
    m = G.gemm_nt_model(p["a"], p["w"], p["bias"], p["res"], act, p["gate"], 0.75, p["row_scale"], 49, dt=F32, ft=F64)
    assert G.err(m["y"], full) < TIGHT
    assert float((gate == 0).sum()) > 0 or M == 1                                        # exact zeros of the gate are closed
    assert G.err(G.gemm_nt_model(p["a"], p["w"], p["bias"], p["res"], act, dt=F32, ft=F64)["y"], v + res) < TIGHT


def test_gelu_forms():
    """the bf16 kernels' tanh form is within 5e-4 of the exact GELU (N4): a deviation the bf16 bound (2^-8 + 8 e_chain) holds, and
    one the chain carries"""
    x = torch.linspace(-8, 8, 4001, dtype=F64)
    exact, tanh_form = G.gelu_model(x, F32, F64), G.gelu_model(x.float(), BF16, F32).double()
    assert G.err(exact, F.gelu(x)) < TIGHT
    assert float((exact - tanh_form).abs().max()) < 5e-4
    assert G.err(G.gelu_model(x.float(), F32, F32), exact) < 1e-6


@pytest.mark.parametrize("M,N", [(1, 64), (33, 1024)])
def test_gated_and_lnbwd_models_vs_autograd_of_the_ffn(M, N):
    """z -> LN -> conv1 (W1 [N,256]) -> ReLU -> conv2 (W2 [256,N]) by autograd at float64: dH through the ReLU is gated_model with the
    gate h > 0, and dz is gemm_lnbwd_model of dH with Wt = W1^T (module.py:74-80, 138-144; encoder.py:24-32 for the residual)"""
    g = torch.Generator().manual_seed(5 + M)
    z = (torch.randn(M, 256, generator=g, dtype=F64) * 2 + 0.3).requires_grad_()
    gam = (1 + 0.1 * torch.randn(256, generator=g, dtype=F64)).requires_grad_()
    bet = torch.zeros(256, dtype=F64, requires_grad=True)
    w1 = (0.08 * torch.randn(N, 256, generator=g, dtype=F64)).requires_grad_()
    b1 = 0.3 * torch.randn(N, generator=g, dtype=F64)
    w2 = (0.06 * torch.randn(256, N, generator=g, dtype=F64)).requires_grad_()
    d_out = torch.randn(M, 256, generator=g, dtype=F64)
    d_res = torch.randn(M, 256, generator=g, dtype=F64)
    xn = O.custom_layernorm(z, gam, bet)
    pre = F.linear(xn, w1, b1)
    pre.retain_grad()
    xn.retain_grad()
    h = torch.relu(pre)
    (F.linear(h, w2) * d_out).sum().backward()
    dh = G.gated_model(d_out, w2.detach().t().contiguous(), pre.detach() > 0, 1.0, dt=F32, ft=F64)["y"]
    assert G.err(dh, pre.grad) < TIGHT
    assert G.err(G.gated_model(d_out, w2.detach().t().contiguous(), pre.detach() > 0, 1.25, dt=F32, ft=F64)["y"], 1.25 * pre.grad) < TIGHT
    zd = z.detach()
    stats = torch.stack([zd.mean(-1), 1 / (zd.std(-1) + 1e-6)], 1)
    wt = w1.detach().t().contiguous()                                                # [256, N] = W1^T
    m = G.gemm_lnbwd_model(pre.grad, wt, zd, stats, gam.detach(), d_res, dt=F32, ft=F64)
    assert G.err(m["dz"], z.grad + d_res) < TIGHT and G.err(m["dgamma"], gam.grad) < TIGHT and G.err(m["dbeta"], bet.grad) < TIGHT
    m = G.gemm_lnbwd_model(pre.grad, wt, zd, stats, gam.detach(), None, dt=F32, ft=F64)
    assert G.err(m["dz"], z.grad) < TIGHT
    # the weight gradients of both convolutions
    tn = G.gemm_tn_model(pre.grad, xn.detach(), dt=F32, ft=F64)
    assert G.err(tn["dw"], w1.grad) < TIGHT and G.err(tn["db"], pre.grad.sum(0)) < TIGHT
    assert G.err(G.gemm_tn_model(d_out, h.detach(), dt=F32, ft=F64)["dw"], w2.grad) < TIGHT


@pytest.mark.parametrize("dt", G.DTS, ids=G.dt_name)
def test_gemm_tn_model_splits_and_drop(dt):
    p = G.tn_inputs(300, 128, 128, dt, seed=3)
    ref = G.gemm_tn_model(p["dy"], p["x"], dt=dt, ft=F64)
    for splits in (1, 2, 5):
        ch = G.gemm_tn_model(p["dy"], p["x"], splits, dt=dt, ft=F32)
        assert G.err(ch["dw"], ref["dw"]) < 2e-6 and G.err(ch["db"], ref["db"]) < 2e-6
    lost = G.gemm_tn_model(p["dy"], p["x"], drop=(256, 300), dt=dt, ft=F64)
    assert G.err(lost["dw"], p["dy"][:256].double().t() @ p["x"][:256].double()) < TIGHT
    assert G.tn_rows_per_split(300, 2) == 192 and G.tn_rows_per_split(6181, 12) == 576 and G.tn_rows_per_split(1, 1) == 64
    assert G.tn_last_step(6181, 12) == (6144, 6181)                 # 11 x 576 = 6336 > 6181: split 11 has no rows, split 10 ends in 37
    assert G.tn_last_step(6700, 12) == (6656, 6700) and G.tn_last_step(64, 1) == (0, 64) and G.tn_last_step(65, 1) == (64, 65)


# ------------------------------------------------------------------------------------------ the chains
@pytest.mark.parametrize("dt", G.DTS, ids=G.dt_name)
def test_chains_stay_near_their_references(dt):
    """e_chain of the working-precision chains: fp32 round-off for fp32 kernels; for bf16 what the rounding points leave -- each a
    rounding of an intermediate to 2^-9 of itself, so e_chain stays below a few 2^-9 and the bounds below 5 %"""
    cap = 2e-5 if dt == F32 else 4 * 2.0 ** -9
    p = G.ln_gemm_inputs(129, 768, dt, seed=4)
    _, e = G.e_chain_of(G.ln_gemm_model, p["x"], p["gamma"], p["beta"], p["w"], p["bias"], dt=dt)
    assert max(e.values()) < cap, e
    assert e["xn"] < 2e-6 and e["mean"] < 1e-6 and e["rstd"] < 1e-6          # (the stored xn's rounding is the bound's 2^-8, not the chain's)
    p = G.nt_inputs(65, 160, 200, dt, seed=4, res=True, gate=True, row_scale=49)
    for act in G.ACTS:
        _, e = G.e_chain_of(G.gemm_nt_model, p["a"], p["w"], p["bias"], p["res"], act, p["gate"], 0.75, p["row_scale"], 49, dt=dt)
        assert e["y"] < cap, (act, e)
    p = G.lnbwd_inputs(129, 72, dt, seed=4)
    _, e = G.e_chain_of(G.gemm_lnbwd_model, p["dy"], p["wt"], p["z"], p["stats"], p["gamma"], p["d_res"], dt=dt)
    assert max(e.values()) < cap, e


def test_initial_accumulator_and_k_steps_are_in_the_chain():
    """P1 / P2: with a bias 1000 times the product every partial sum is rounded at the bias' magnitude; the chain that starts from the
    bias carries that error, one that adds the bias at the end would not"""
    p = G.ln_gemm_inputs(64, 64, F32, seed=6)
    b = 300.0 * torch.ones(64)
    ref, e = G.e_chain_of(G.ln_gemm_model, p["x"], p["gamma"], p["beta"], p["w"], b, dt=F32)
    late = G.ln_gemm_model(p["x"], p["gamma"], p["beta"], p["w"], None, dt=F32, ft=F32)["y"] + b
    assert e["y"] > 2 * G.err(late, ref["y"])


# ------------------------------------------------------------------------------------------ sign bits
def _encode_signs(pos):
    """written from the kernel's comment alone, lane by lane: for panel j, group g, row, lane half: a 16-bit word collected register
    by register (t = 0 first) as word = 2 word + bit; register t of half `half` is feature 16 (t >> 3) + 8 half + (t & 7)"""
    M, N = pos.shape
    words = [0] * ((N // 32) * M * 2)
    for j in range(N // 64):
        for g in range(2):
            for row in range(M):
                for half in range(2):
                    word = 0
                    for t in range(16):
                        f = 16 * (t >> 3) + 8 * half + (t & 7)
                        word = 2 * word + int(pos[row, 64 * j + 32 * g + f])
                    words[((2 * j + g) * M + row) * 2 + half] = word
    raw = torch.tensor([[w & 255, w >> 8] for w in words], dtype=torch.uint8)
    return raw.reshape(-1)


@pytest.mark.parametrize("M,N", [(1, 64), (3, 128), (33, 192)])
def test_sign_decoder_inverts_the_encoder(M, N):
    g = torch.Generator().manual_seed(M + N)
    pos = torch.rand(M, N, generator=g) < 0.5
    raw = _encode_signs(pos)
    assert raw.numel() == (N // 32) * M * 4                             # mtmp_sign_bits_bytes
    assert torch.equal(G.decode_signs(raw, M, N), pos)
    one = torch.zeros(M, N, dtype=torch.bool)
    one[M - 1, 37] = True                                               # group 1, feature 5: half 0, register 5 -> bit 10
    raw = _encode_signs(one)
    assert int(raw.to(torch.int32).sum()) == 4 and int(raw[((1 * M + M - 1) * 2 + 0) * 2 + 1]) == 4
    live = G.live_words(raw, M, N, M - 1)
    assert int(live.sum()) == (N // 32) * (M - 1) * 4 and not bool(live[((1 * M + M - 1) * 2) * 2])


# ------------------------------------------------------------------------------------------ launch arithmetic of the cases
def test_panel_shares_of_the_walk_cases():
    """launch_ln_gemm_dma: nsplit = clamp(512 / mtiles, need, npanels), per = ceil(npanels / nsplit)"""
    assert [n for _, n in G.panel_shares(257, 1024)] == [1] * 16
    assert [n for _, n in G.panel_shares(4097, 1024)] == [2] * 8 + [0] * 7                  # 33 row blocks: per 2
    assert [n for _, n in G.panel_shares(8193, 1024)] == [3, 3, 3, 3, 3, 1, 0]              # 65 row blocks: per 3, one empty workgroup
    assert [n for _, n in G.panel_shares(32769, 1024)] == [16]                              # 257 row blocks: per 16 = MAXP
    assert [n for _, n in G.panel_shares(8193, 768)] == [2] * 6 + [0]
    assert [n for _, n in G.panel_shares(32769, 768)] == [12]
    assert G.panel_probe_panels() == [2, 5, 8, 11, 14]


# ------------------------------------------------------------------------------------------ the one-tile probes, on the reference alone
def _probe_ok(lost, ref, e_chain, bf16_out):
    b, loss = G.bound(e_chain, bf16_out), G.err(lost, ref)
    assert b <= G.PROBE_BOUND and loss >= G.PROBE_LOSS, (b, loss)
    return b, loss


@pytest.mark.parametrize("dt", G.DTS, ids=G.dt_name)
def test_probe_k_tail_chunk_of_gemm_nt(dt):
    p = G.nt_probe_inputs(dt)
    ref, e = G.e_chain_of(G.gemm_nt_model, p["a"], p["w"], dt=dt)
    q = G.nt_probe_lost(p)
    lost = G.gemm_nt_model(q["a"], q["w"], dt=dt, ft=F64)
    _probe_ok(lost["y"], ref["y"], e["y"], dt == BF16)
    last = slice(64, 65)                                                # the one row of the last row tile, as a tensor of its own
    _probe_ok(lost["y"][last], ref["y"][last], G.err(G.gemm_nt_model(p["a"], p["w"], dt=dt, ft=F32)["y"][last], ref["y"][last]), dt == BF16)


def test_probe_last_panel_of_a_share():
    dt = BF16                                                           # (ln_gemm_dma_kernel is the bf16 build)
    p = G.panel_probe_inputs(dt)
    args = lambda q: (q["x"], q["gamma"], q["beta"], q["w"], q["bias"], "relu")
    ref, e = G.e_chain_of(G.ln_gemm_model, *args(p), dt=dt)
    for j in G.panel_probe_panels():
        lost = G.ln_gemm_model(*args(G.panel_probe_lost(p, j)), dt=dt, ft=F64)
        _probe_ok(lost["y"], ref["y"], e["y"], True)
        cols = slice(64 * j, 64 * j + 64)
        assert G.err(lost["y"][:, cols], ref["y"][:, cols]) >= G.PROBE_LOSS


@pytest.mark.parametrize("splits", [12])
def test_probe_last_token_step_of_a_gemm_tn_split(splits):
    """splits = 12: tn_launch_splits for (6700, 256, 1024) in bf16 -- 16 tiles: 192 / 16 = 12 splits, 12 * 512 <= M: mode 3"""
    dt = BF16
    p = G.tn_probe_inputs(dt, splits)
    lo, hi = G.tn_last_step(G.TN_PROBE["M"], splits)
    assert (lo, hi) == (6656, 6700)
    sub = slice(0, 64)                                                  # (the conditions on 64 of the 256 output rows: a quarter of the work)
    dy = p["dy"][:, sub]
    ref, e = G.e_chain_of(G.gemm_tn_model, dy, p["x"], splits, dt=dt)
    lost = G.gemm_tn_model(dy, p["x"], splits, drop=(lo, hi), dt=dt, ft=F64)
    for name in ("dw", "db"):
        _probe_ok(lost[name], ref[name], e[name], False)
