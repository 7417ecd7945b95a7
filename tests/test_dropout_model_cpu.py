"""No GPU: the replayed dropout mask (tests/dropout_model.py) and the masked float64 models, before tests/test_dropout_model_gpu.py
holds the kernels to them.

  mask    the vectorised hash against a second writing in Python integers, against literal known answers (computed once with the
          Python-integer writing and frozen here; the GPU file ties them to the kernels, whose masks must equal the model's bit for
          bit), the thresholds, and the keep fraction within 4 sigma of the binomial
  models  the masked models against plain torch float64 chains with `mask * keep_scale` multiplied in, backwards by autograd, to 1e-12;
          keep=None against an all-true mask of scale 1, bit for bit
  faults  every mistake of dropout_model.FAULTS, made in the float64 model at the shapes of the GPU file, must move an output past the
          bound of the sound model -- max(8 e_chain, 16 * 2^-24) (+ 2^-8 for a bf16 output), which comes from the reference alone.
          ONE fault cannot be seen and is named here with its measured ratio instead: the scale applied after the rounding to bf16
          moves a bf16 result by at most one rounding of the parked value: the largest err / bound over the shapes is 0.49
          (test_fault_scale_after_the_rounding_cannot_be_seen).  The bound stays as it is.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dropout_model as DM
from tests import gemm_model as G
from tests import row_kernels_model as R

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
P, WORD = DM.P, DM.WORD


# ------------------------------------------------------------------------------------------ the mask
def scalar_fields(seed_eff, g):
    """the four fields of group g, in Python integers"""
    m = 0xFFFFFFFF
    x = ((g * 0x9E3779B1) & m) ^ seed_eff
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & m
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & m
    x ^= x >> 16
    y = (x * 0x27D4EB2F) & m
    y ^= y >> 15
    return [x & 0xFFFF, x >> 16, y & 0xFFFF, y >> 16]


def test_vectorised_mask_equals_the_scalar_writing():
    rng = np.random.default_rng(5)
    seeds = rng.integers(0, 1 << 32, 4000, dtype=np.uint64)
    groups = rng.integers(0, 1 << 30, 4000, dtype=np.uint64)
    groups[:4] = [0, 1, (1 << 30) - 1, (1 << 30) - 2]
    for s, g in zip(seeds.tolist(), groups.tolist()):
        got = DM.fields_of(np.arange(4 * g, 4 * g + 4, dtype=np.uint64), s)
        assert got.tolist() == scalar_fields(s, g), (s, g)
    # ... and with a seed word: only its low 32 bits count
    for s, g in zip(seeds[:200].tolist(), groups[:200].tolist()):
        got = DM.fields_of(np.arange(4 * g, 4 * g + 4, dtype=np.uint64), s, WORD)
        assert got.tolist() == scalar_fields(s ^ (WORD & 0xFFFFFFFF), g), (s, g)


#         seed,        word,  group, the four fields
KNOWN = [
    (0, None, 0, [0, 0, 0, 0]),
    (0, None, 1, [747, 4605, 53087, 50876]),
    (1234, None, 0, [49163, 3884, 31807, 37788]),
    (1234, None, 255, [13201, 50351, 58806, 48021]),
    (0xFFFFFFFF, None, 7, [25908, 14696, 25806, 6689]),
    (0xFFFFFFFF, None, 1048577, [48699, 435, 48941, 54653]),
    (1234, WORD, 0, [41485, 63809, 52806, 12434]),
    (77, WORD, 33791, [39273, 620, 54312, 11447]),
]


@pytest.mark.parametrize("seed,word,g,want", KNOWN)
def test_known_answers(seed, word, g, want):
    assert DM.fields_of(np.arange(4 * g, 4 * g + 4, dtype=np.uint64), seed, word).tolist() == want
    thr = DM.threshold(P)
    mask = DM.keep_mask((4 * g + 4,), P, seed, word)[4 * g:]
    assert mask.tolist() == [f >= thr for f in want]


def test_thresholds():
    got = [DM.threshold(p) for p in (0.0, -1.0, 2.0 ** -17, 2.0 ** -16, 0.1, 0.5, 0.999)]
    assert got == [0, 0, 1, 1, 6554, 32768, 65470], got
    assert bool(DM.keep_mask((1024,), 0.0, 3).all())


def test_keep_scale_is_the_fp32_quotient():
    for p in (0.1, 0.5, 2.0 ** -16, 0.999, 0.2):
        s = DM.keep_scale(p)
        assert s == float(np.float32(s))
        assert s == float(torch.ones((), dtype=F32) / (torch.ones((), dtype=F32) - torch.tensor(p, dtype=F32)))
    assert DM.keep_scale(0.5) == 2.0 and DM.keep_scale(0.0) == 1.0


@pytest.mark.parametrize("p", [0.1, 0.5, 2.0 ** -16, 0.999])
@pytest.mark.parametrize("seed,word", [(0, None), (1234, None), (0xFFFFFFFF, WORD)])
def test_keep_fraction(p, seed, word):
    n = 1 << 20
    q = (65536 - DM.threshold(p)) / 65536
    kept = int(DM.keep_mask((n,), p, seed, word).sum())
    assert abs(kept - n * q) <= 4 * math.sqrt(n * q * (1 - q)), (kept, n * q)


def test_stream_input_numbering():
    B, N = 3, 5
    e = DM.stream_input_elements(B, N)
    assert e.shape == (B, N + 1, 256) and e.reshape(-1).tolist() == list(range(B * (N + 1) * 256))
    c = DM.stream_input_elements(B, N, nb=4)
    assert int(c[0, 0, 0]) == 4 * 256 and int(c[1, 0, 0]) == (N + 1 + 4 + 4) * 256 and int(c[2, N, 255]) == 3 * (N + 5) * 256 - 1


# ------------------------------------------------------------------------------------------ the models against explicit torch chains
TOL = 1e-12


def _close(got, want):
    assert got.dtype == F64 and got.shape == want.shape
    assert float((got - want).abs().max()) <= TOL * max(1.0, float(want.abs().max()))


def _mult(keep):
    return keep.mask.to(F64) * keep.scale


@pytest.mark.parametrize("dt", G.DTS, ids=G.dt_name)
def test_ln_gemm_model_with_a_mask(dt):
    M, N = 33, 1024
    p = G.ln_gemm_inputs(M, N, dt, seed=0)
    keep = DM.keep((M, N), P, DM.FFN1_SEED)
    got = G.ln_gemm_model(p["x"], p["gamma"], p["beta"], p["w"], p["bias"], "relu", keep, dt=dt, ft=F64)
    x = p["x"].double()
    xn = p["gamma"].double() * (x - x.mean(-1, keepdim=True)) / (x.std(-1, keepdim=True) + R.LN_EPS) + p["beta"].double()
    want = torch.relu(xn @ p["w"].double().t() + p["bias"].double()) * _mult(keep)
    _close(got["y"], want)
    _close(got["xn"], xn)
    assert bool((got["y"][~keep.mask] == 0).all())


@pytest.mark.parametrize("dt", G.DTS, ids=G.dt_name)
@pytest.mark.parametrize("c", DM.NT_DROP_CASES[:4], ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}")
def test_gemm_nt_model_with_a_mask(c, dt):
    M, N, K, o = c
    p = G.nt_inputs(M, N, K, dt, res=o.get("res", False), lda=o.get("lda"), ldr=o.get("ldr"))
    keep = DM.keep((M, N), P, DM.FFN2_SEED)
    got = G.gemm_nt_model(p["a"], p["w"], p["bias"], p["res"], o.get("act"), keep=keep, dt=dt, ft=F64)["y"]
    v = p["a"].double() @ p["w"].double().t() + p["bias"].double()
    v = torch.relu(v) if o.get("act") == "relu" else F.gelu(v) if o.get("act") == "gelu" else v
    want = v * _mult(keep) + (0 if p["res"] is None else p["res"].double())
    _close(got, want)


@pytest.mark.parametrize("dt", G.DTS, ids=G.dt_name)
def test_dropout_bwd_model_is_autograd_of_the_masked_product(dt):
    g = torch.Generator().manual_seed(3)
    gr = R.rnd(torch.randn(33, 256, generator=g), dt)
    keep = DM.keep((33, 256), P, 5)
    leaf = torch.zeros(33, 256, requires_grad=True)
    (leaf * (keep.mask.float() * keep.scale) * gr).sum().backward()
    got = G.dropout_bwd_model(gr, keep, dt=dt)["y"]
    assert got.dtype == F32 and torch.equal(got, leaf.grad.to(dt).float())
    assert bool((got[~keep.mask] == 0).all()) and bool((got[keep.mask] != 0).all())


def test_operand_drop_model_is_the_gated_product_of_the_rounded_operand():
    M, N = 33, 1024
    q = G.gated_inputs(M, N, BF16)
    keep = DM.keep((M, 256), P, DM.FFN2_SEED)
    gate = torch.rand(M, N, generator=torch.Generator().manual_seed(1)) < 0.5
    got = G.operand_drop_model(q["a"], keep, q["w"], gate, 1.25, dt=BF16, ft=F64)
    ad = (q["a"] * keep.scale).to(BF16).double() * keep.mask
    assert torch.equal(got["a"].double(), ad)
    _close(got["y"], (ad @ q["w"].double().t()) * 1.25 * gate)


@pytest.mark.parametrize("dt", G.DTS, ids=G.dt_name)
@pytest.mark.parametrize("B,N,nb,use_pe,kv", [c + (None,) for c in DM.STREAM_DROP_CASES[:2]] + [R.STREAM_PACKED[:3] + (False, R.STREAM_PACKED[3])])
def test_stream_input_model_with_a_mask(B, N, nb, use_pe, kv, dt):
    c = R.stream_case(B, N, nb, use_pe, dt, kv)
    keep = DM.Keep(DM.keep_of_elements(DM.stream_input_elements(B, N), P, DM.STREAM_SEED), DM.keep_scale(P))
    got = R.stream_input_model(c["x"], c["cls"], c["gamma"], c["beta"], c["pe"], c["bott"], c["w"], c["kv_len"], keep, dt=dt, ft=F64)
    x, cls, gam, bet, bott = (t.double().requires_grad_() for t in (c["x"], c["cls"].to(dt), c["gamma"], c["beta"], c["bott"]))
    y = F.layer_norm(torch.cat([cls.expand(B, 1, 256), x], 1), (256,), gam, bet, 1e-5)
    if c["pe"] is not None:
        y = y + c["pe"][:N + 1].double()
    z = torch.cat([bott.expand(B, nb, 256), y * _mult(keep)], 1)
    live = got["live"]
    (z * c["w"].double() * live[..., None]).sum().backward()
    _close(got["z"], z.detach())
    for name, t in (("dx", x), ("dcls", cls), ("dgamma", gam), ("dbeta", bet), ("dbott", bott)):
        _close(got[name], t.grad.reshape(got[name].shape))
    assert bool((got["z"][:, nb:][~keep.mask] == 0).all())
    assert torch.equal(got["z"][:, :nb], c["bott"].double().expand(B, nb, 256))           # the bottleneck rows are never masked


@pytest.mark.parametrize("dt", G.DTS, ids=G.dt_name)
def test_keep_none_is_an_all_true_mask_of_scale_one(dt):
    """(the existing CPU files pass unedited on the keep=None path; this pins the masked path to it)"""
    ones = lambda *s: DM.Keep(torch.ones(*s, dtype=torch.bool), 1.0)
    p = G.ln_gemm_inputs(33, 1024, dt)
    args = (p["x"], p["gamma"], p["beta"], p["w"], p["bias"], "relu")
    q = G.nt_inputs(65, 160, 72, dt, res=True)
    c = R.stream_case(2, 5, 1, False, dt)
    sargs = (c["x"], c["cls"], c["gamma"], c["beta"], c["pe"], c["bott"], c["w"], None)
    for ft in (F64, F32):
        a, b = G.ln_gemm_model(*args, dt=dt, ft=ft), G.ln_gemm_model(*args, ones(33, 1024), dt=dt, ft=ft)
        assert all(torch.equal(a[k], b[k]) for k in a)
        a = G.gemm_nt_model(q["a"], q["w"], q["bias"], q["res"], "gelu", dt=dt, ft=ft)["y"]
        assert torch.equal(a, G.gemm_nt_model(q["a"], q["w"], q["bias"], q["res"], "gelu", keep=ones(65, 160), dt=dt, ft=ft)["y"])
        a, b = R.stream_input_model(*sargs, dt=dt, ft=ft), R.stream_input_model(*sargs, ones(2, 6, 256), dt=dt, ft=ft)
        assert all(torch.equal(a[k], b[k]) for k in a)


# ------------------------------------------------------------------------------------------ seeded faults
def _ffn1(M, dt, seed=DM.FFN1_SEED, word=None):
    p = G.ln_gemm_inputs(M, 1024, dt)
    args = (p["x"], p["gamma"], p["beta"], p["w"], p["bias"], "relu")
    ref, e = G.e_chain_of(G.ln_gemm_model, *args, DM.keep((M, 1024), P, seed, word), dt=dt)
    return args, ref["y"], G.bound(e["y"], dt == BF16)


def _ffn2(c, dt, seed=DM.FFN2_SEED):
    M, N, K, o = c
    p = G.nt_inputs(M, N, K, dt, res=o.get("res", False), lda=o.get("lda"), ldr=o.get("ldr"))
    args = (p["a"], p["w"], p["bias"], p["res"], o.get("act"))
    ref, e = G.e_chain_of(G.gemm_nt_model, *args, keep=DM.keep((M, N), P, seed), dt=dt)
    return args, ref["y"], G.bound(e["y"], dt == BF16)


def _stream(B, N, nb, use_pe, dt, kv=None):
    c = R.stream_case(B, N, nb, use_pe, dt, kv)
    args = (c["x"], c["cls"], c["gamma"], c["beta"], c["pe"], c["bott"], c["w"], c["kv_len"])
    keep = DM.Keep(DM.keep_of_elements(DM.stream_input_elements(B, N), P, DM.STREAM_SEED), DM.keep_scale(P))
    ref, et = R.e_torch_of(R.stream_input_model, *args, keep, dt=dt)
    bounds = {k: R.bound(et[k], dt == BF16 and k in ("z", "dx")) for k in et}
    return args, keep, ref, bounds


def _caught(bad, ref, b, what=""):
    e = G.err(bad, ref)
    assert e > b, f"{what}: the fault moves the output by {e:.3e}, inside the bound {b:.3e}"


SMALL_NT = DM.NT_DROP_CASES[:4]


@pytest.mark.parametrize("dt", G.DTS, ids=G.dt_name)
@pytest.mark.parametrize("fault", ["fields_hi_lo", "other_seed", "word_ignored", "ld_indexed"])
def test_fault_in_the_mask_of_a_gemm_epilogue(fault, dt):
    """another mask than the sound one, at every FFN1 and (small) FFN2 shape of the GPU file.  ld_indexed: the row stride of a windowed
    output (ldy 176 for N 160), of the residual (136 for 128) or of FFN1's x buffer (320 for 1024 would be FEWER columns: 1032 here)"""
    word = WORD if fault == "word_ignored" else None
    for M in DM.FFN1_M:
        args, ref, b = _ffn1(M, dt, word=word)
        bad = DM.faulty_keep(fault, (M, 1024), P, DM.FFN1_SEED, word, ld=1032, other_seed=DM.FFN1_SEED + 1)
        if fault == "ld_indexed" and M == 1:                  # (one row: the stride is never used)
            continue
        _caught(G.ln_gemm_model(*args, bad, dt=dt, ft=F64)["y"], ref, b, f"ffn1 M={M}")
    for c, ld in [(c, c[3].get("ldr", c[1] + 8)) for c in SMALL_NT] + [(DM.NT_WINDOW_CASE[:4], DM.NT_WINDOW_CASE[4])]:
        M, N = c[:2]
        args, ref, b = _ffn2(c, dt)
        if fault == "word_ignored":                           # (no word in this reference: set one, and ignore it)
            ref = G.gemm_nt_model(*args, keep=DM.keep((M, N), P, DM.FFN2_SEED, WORD), dt=dt, ft=F64)["y"]
        bad = DM.faulty_keep(fault, (M, N), P, DM.FFN2_SEED, word, ld=ld, other_seed=DM.FFN2_SEED + 1)
        _caught(G.gemm_nt_model(*args, keep=bad, dt=dt, ft=F64)["y"], ref, b, f"ffn2 {c[:3]}")


@pytest.mark.parametrize("dt", G.DTS, ids=G.dt_name)
def test_fault_scale_left_out(dt):
    for M in DM.FFN1_M:
        args, ref, b = _ffn1(M, dt)
        _caught(G.ln_gemm_model(*args, DM.keep((M, 1024), P, DM.FFN1_SEED), "no_scale", dt=dt, ft=F64)["y"], ref, b, f"ffn1 M={M}")
    for c in SMALL_NT:
        args, ref, b = _ffn2(c, dt)
        _caught(G.gemm_nt_model(*args, keep=DM.keep(c[:2], P, DM.FFN2_SEED), fault="no_scale", dt=dt, ft=F64)["y"], ref, b, f"ffn2 {c[:3]}")
    for B, N, nb, pe in DM.STREAM_DROP_CASES:
        args, keep, ref, bd = _stream(B, N, nb, pe, dt)
        bad = R.stream_input_model(*args, DM.Keep(keep.mask, 1.0), dt=dt, ft=F64)
        for k in ("z", "dx", "dcls", "dgamma", "dbeta"):
            _caught(bad[k], ref[k], bd[k], f"stream {B}x{N} {k}")


def test_fault_scale_after_the_rounding_cannot_be_seen():
    """bf16: T(T(v) * s) for T(v * s) moves a result by at most one rounding of the parked value, and the bound of a bf16 output allows
    one rounding (2^-8 of |ref| + rms against 2^-9 |ref|).  Measured: the largest err / bound over these cases is 0.49 -- this fault
    is invisible to the element-wise bound, which is not tightened to fit; the test states that it stays below 1."""
    worst = 0.0
    for M in DM.FFN1_M:
        args, ref, b = _ffn1(M, BF16)
        bad = G.ln_gemm_model(*args, DM.keep((M, 1024), P, DM.FFN1_SEED), "scale_after_round", dt=BF16, ft=F64)["y"]
        worst = max(worst, G.err(bad.to(BF16), ref) / b)
    for c in SMALL_NT:
        args, ref, b = _ffn2(c, BF16)
        bad = G.gemm_nt_model(*args, keep=DM.keep(c[:2], P, DM.FFN2_SEED), fault="scale_after_round", dt=BF16, ft=F64)["y"]
        worst = max(worst, G.err(bad.to(BF16), ref) / b)
    print(f"scale_after_round: worst err / bound {worst:.3f}")
    assert 0.0 < worst < 1.0, worst


@pytest.mark.parametrize("dt", G.DTS, ids=G.dt_name)
def test_fault_dropout_behind_the_residual(dt):
    for c in [c for c in SMALL_NT if c[3].get("res")]:
        args, ref, b = _ffn2(c, dt)
        _caught(G.gemm_nt_model(*args, keep=DM.keep(c[:2], P, DM.FFN2_SEED), fault="behind_residual", dt=dt, ft=F64)["y"], ref, b, str(c[:3]))


@pytest.mark.parametrize("dt", G.DTS, ids=G.dt_name)
@pytest.mark.parametrize("B,N,nb,use_pe", DM.STREAM_DROP_CASES)
def test_faults_of_the_stream_input(B, N, nb, use_pe, dt):
    args, keep, ref, bd = _stream(B, N, nb, use_pe, dt)
    scale = keep.scale
    grads = ("dx", "dcls", "dgamma", "dbeta")
    # the backward's mask one group late: the forward is untouched, every gradient moves
    bad = R.stream_input_model(*args, keep, DM.Keep(DM.shifted_group(keep.mask), scale), dt=dt, ft=F64)
    assert torch.equal(bad["z"], ref["z"])
    for k in grads:
        _caught(bad[k], ref[k], bd[k], f"bwd_shifted_group {k}")
    # the two halves of each hash word swapped
    bad = R.stream_input_model(*args, DM.Keep(DM.keep_of_elements(DM.stream_input_elements(B, N), P, DM.STREAM_SEED, order=(1, 0, 3, 2)), scale),
                               dt=dt, ft=F64)
    for k in ("z",) + grads:
        _caught(bad[k], ref[k], bd[k], f"fields_hi_lo {k}")
    # the bottleneck rows masked as well (numbered as rows of the whole buffer)
    allrows = DM.keep_of_elements(DM.elements((B, nb + 1 + N, 256)), P, DM.STREAM_SEED)
    bad = R.stream_input_model(*args, keep, None, DM.Keep(allrows[:, :nb], scale), dt=dt, ft=F64)
    for k in ("z", "dbott"):
        _caught(bad[k], ref[k], bd[k], f"bott_masked {k}")
    # a row numbering that counts the bottleneck rows
    bad = R.stream_input_model(*args, DM.Keep(DM.keep_of_elements(DM.stream_input_elements(B, N, nb), P, DM.STREAM_SEED), scale), dt=dt, ft=F64)
    for k in ("z",) + grads:
        _caught(bad[k], ref[k], bd[k], f"bott_counted {k}")


@pytest.mark.parametrize("dt", G.DTS, ids=G.dt_name)
def test_fault_shifted_or_foreign_mask_in_dropout_bwd(dt):
    """dropout_bwd and the operand drop are held bit for bit: any other mask shows"""
    gr = R.rnd(torch.randn(33, 256, generator=torch.Generator().manual_seed(3)), dt)
    keep = DM.keep((33, 256), P, DM.FFN2_SEED, WORD)
    ref = G.dropout_bwd_model(gr, keep, dt=dt)["y"]
    for bad in (DM.Keep(DM.shifted_group(keep.mask), keep.scale), DM.faulty_keep("word_ignored", (33, 256), P, DM.FFN2_SEED, WORD),
                DM.faulty_keep("fields_hi_lo", (33, 256), P, DM.FFN2_SEED, WORD), DM.Keep(keep.mask, 1.0)):
        assert not torch.equal(G.dropout_bwd_model(gr, bad, dt=dt)["y"], ref)


@pytest.mark.parametrize("dt", G.DTS, ids=G.dt_name)
@pytest.mark.parametrize("M", DM.FFN1_M)
def test_seeds_eq_show_greater_for_greater_equal(M, dt):
    """`>` for `>=` differs only where a field EQUALS the threshold: SEEDS_EQ[M] is the first seed (from 1000) with such an element
    where the FFN1 output is well above zero, so the fault drops a value the sound kernel keeps"""
    p = G.ln_gemm_inputs(M, 1024, dt)
    plain = G.ln_gemm_model(p["x"], p["gamma"], p["beta"], p["w"], p["bias"], "relu", dt=dt, ft=F64)["y"]
    matters = plain > plain.pow(2).mean().sqrt()
    if dt == F32:                                            # (the seeds were searched with the fp32 inputs; bf16 must agree)
        assert DM.find_seed_eq((M, 1024), P, matters) == DM.SEEDS_EQ[M]
    seed = DM.SEEDS_EQ[M]
    assert bool((DM.equal_fields((M, 1024), P, seed) & matters).any())
    args, ref, b = _ffn1(M, dt, seed=seed)
    _caught(G.ln_gemm_model(*args, DM.faulty_keep("gt_for_ge", (M, 1024), P, seed), dt=dt, ft=F64)["y"], ref, b, f"M={M}")


def test_every_fault_has_a_test():
    assert set(DM.FAULTS) == {"ld_indexed", "fields_hi_lo", "other_seed", "word_ignored", "gt_for_ge", "no_scale", "scale_after_round",
                              "behind_residual", "bwd_shifted_group", "bott_masked", "bott_counted"}


def test_one_hash_per_group_equals_the_per_element_writing():
    for shape in ((4,), (1028,), (33, 1024), (3, 6, 256)):
        assert np.array_equal(DM.contiguous_fields(shape, 1234, WORD), DM.fields_of(DM.elements(shape), 1234, WORD))
