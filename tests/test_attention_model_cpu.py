"""CPU: pins tests/attention_model.py -- the float64 model against the oracle's attention and its autograd and against the float64
softmax of tests/test_attn_prefix_gpu.py, packed against padded, the all-masked sample -- and proves on the reference alone that
every one-tile probe of tests/test_attention_model_gpu.py can see: a kernel that loses the spotlighted tile misses the probe's
bound by a factor of two at least, whatever bf16 rounding does."""
import math

import pytest
import torch

from oracle import tri_mbt_oracle as O
from tests import attention_model as A
from tests import test_attn_prefix_gpu as PFX

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
ROUND_OFF = 1e-5        # err of an fp32 softmax attention and its autograd against float64 at these sizes stays below this


def _inputs(N, B, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, N, 768, generator=g), torch.randn(B, N, 256, generator=g), torch.randn(B, N, 256, generator=g))


@pytest.mark.parametrize("N,lens", [(54, None), (54, [54, 4, 30, 7]), (133, [133, 4, 5, 90]), (261, [261, 200, 4, 64]), (40, [0, 17, 40, 1])])
def test_model_matches_oracle_attention_and_autograd(N, lens):
    qkv, res, w = _inputs(N, 4, 7 + N)
    x = qkv.clone().requires_grad_()
    o_ref = O.attention_core(x, None if lens is None else torch.tensor(lens))
    (o_ref * w).sum().backward()
    m = A.attention_model(qkv, lens, w, res, dt=F32, ft=F64)
    assert A.err(m["o"], o_ref) <= ROUND_OFF
    assert A.err(m["o_res"], o_ref.detach().double() + res.double()) <= ROUND_OFF
    for i, nm in enumerate(("dq", "dk", "dv")):
        e = A.err(m[nm], x.grad[..., 256 * i:256 * (i + 1)])
        assert e <= ROUND_OFF, (nm, e)
    # lse: log2 of the sum of exp2 of the scaled scores = logsumexp(q.k / 8) / ln 2, on the live keys
    q, k = (qkv[..., 256 * i:256 * (i + 1)].double().view(4, N, 4, 64).transpose(1, 2) for i in range(2))
    s = q @ k.transpose(-1, -2) / 8.0
    if lens is not None:
        kv = torch.tensor([n if n > 0 else N for n in lens])
        s = s.masked_fill((torch.arange(N)[None, :] >= kv[:, None])[:, None, None, :], -math.inf)
        s[torch.tensor(lens) <= 0] = 0.0
    assert A.err(m["lse"], torch.logsumexp(s, -1) / math.log(2.0)) <= 1e-12


@pytest.mark.parametrize("N,lens,mname", PFX.CASES[:3])
def test_model_matches_the_prefix_reference(N, lens, mname):
    assert torch.equal(A.MASKS[mname], PFX.MASKS[mname]) and A.mask_words(A.MASKS[mname]) == PFX.words(PFX.MASKS[mname])
    qkv, res, w = PFX.inputs(N, 3, F32, 11 + N)
    o_ref, g_ref = PFX.reference(qkv, None if lens is None else torch.tensor(lens), PFX.MASKS[mname], w)
    m = A.attention_model(qkv, lens, w, dt=F32, ft=F64, mask=A.MASKS[mname])
    assert A.err(m["o"], o_ref) <= ROUND_OFF
    for i, nm in enumerate(("dq", "dk", "dv")):
        assert A.err(m[nm], g_ref[..., 256 * i:256 * (i + 1)]) <= ROUND_OFF, nm


def test_packed_model_is_the_padded_model_on_each_samples_rows():
    N, lens = 150, [150, 1, 64, 65, 7]
    qkv, res, w = _inputs(N, len(lens), 3)
    live = torch.arange(N)[None, :] < torch.tensor(lens)[:, None]
    w = w * live[..., None]                                      # (pad queries are live in the padded layout: give them no gradient)
    pad = A.attention_model(qkv, lens, w, res, dt=F32, ft=F64)
    pkd = A.attention_model(qkv, lens, w, res, dt=F32, ft=F64, packed=True)
    assert torch.equal(pkd["qrows"], live) and torch.equal(pkd["krows"], live) and bool(pad["qrows"].all())
    for nm in ("o", "o_res", "dq", "dk", "dv"):
        assert A.err(pkd[nm][live], pad[nm][live]) <= 1e-13, nm          # (zero terms more in a sum: another summation order)
        assert float(pkd[nm][~live].abs().max()) == 0.0, nm
    assert torch.equal(pkd["lse"].transpose(1, 2)[live], pad["lse"].transpose(1, 2)[live])


@pytest.mark.parametrize("ft", [F64, F32])
def test_all_keys_masked_is_the_uniform_average(ft):
    N = 70
    qkv, res, w = _inputs(N, 2, 5)
    m = A.attention_model(qkv, [0, 33], w, res, dt=F32, ft=ft)
    tol = 1e-13 if ft == F64 else 1e-5
    assert torch.allclose(m["o"][0], qkv[0, :, 512:].to(ft).mean(0).expand(N, 256), rtol=0, atol=tol)
    assert torch.allclose(m["dv"][0], w[0].to(ft).mean(0).expand(N, 256), rtol=0, atol=tol)
    assert float(m["dq"][0].abs().max()) == 0.0 and float(m["dk"][0].abs().max()) == 0.0
    assert torch.allclose(m["lse"][0], torch.full((4, N), math.log2(N), dtype=ft), rtol=0, atol=tol)
    assert bool(m["krows"][0].all()) and int(m["krows"][1].sum()) == 33
    c = A.attn_cls_model(qkv, res, [0, 33], w[:, 0], 4, dt=F32, ft=ft)
    assert torch.allclose(c["o"][0], qkv[0, :, 512:].to(ft).mean(0), rtol=0, atol=tol)
    assert float(c["dq"][0].abs().max()) == 0.0 and float(c["dk"][0].abs().max()) == 0.0
    assert torch.allclose(c["dv"][0], (w[0, 0].to(ft) / N).expand(N, 256), rtol=0, atol=tol)


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("cls_tok", [0, 4])
def test_cls_model_is_the_dense_models_cls_row(cls_tok, packed):
    """d_o that is zero outside the CLS row: the dense model's o / lse of that row and its dq / dk / dv"""
    N, lens = 90, [90, 5, 64, 33]
    qkv, res, w = _inputs(N, len(lens), 9)
    d = torch.zeros_like(w)
    d[:, cls_tok] = w[:, cls_tok]
    dense = A.attention_model(qkv, lens, d, res, dt=F32, ft=F64, packed=packed)
    c = A.attn_cls_model(qkv, res, lens, w[:, cls_tok], cls_tok, dt=F32, ft=F64, packed=packed)
    assert A.err(c["o"], dense["o"][:, cls_tok]) <= 1e-12 and A.err(c["r1"], dense["o_res"][:, cls_tok]) <= 1e-12
    assert A.err(c["lse"], dense["lse"][:, :, cls_tok]) <= 1e-12
    assert A.err(c["dq"], dense["dq"][:, cls_tok]) <= 1e-12
    assert A.err(c["dk"], dense["dk"]) <= 1e-12 and A.err(c["dv"], dense["dv"]) <= 1e-12
    rest = torch.ones(N, dtype=torch.bool)
    rest[cls_tok] = False
    assert float(dense["dq"][:, rest].abs().max()) == 0.0


def _probe_cases():
    for kind in A.PROBE_KINDS:
        for tile in A.PROBE_TILES:
            for N, packed, dts in A.PROBE_SHAPES:
                for dt in dts:
                    yield pytest.param(A.probe_case(kind, tile, N, packed), dt, id=f"{kind}-{tile}-{N}{'p' if packed else ''}-{A.dt_name(dt)}")


@pytest.mark.parametrize("c,dt", list(_probe_cases()))
def test_every_probe_can_see_its_tile(c, dt):
    """On the reference alone: bound <= 0.25, a reference with non-zero rms, and err >= 0.5 once the spotlighted tile's term is
    removed -- so a kernel that loses that tile fails by a factor of two at least."""
    ref, lost = A.reference(c, dt), A.dropped(c, dt)
    bodies = A.PROBE_BODIES[c.probe[0]]
    for name in A.PROBE_OUT[c.probe[0]]:
        rms = float(ref[name].pow(2).mean().sqrt())
        e_lost = A.err(lost[name], ref[name])
        for bounded in bodies:
            b = A.bound(A.e_chain(c, dt, bounded)[name], dt == BF16)
            print(f"{c.name}[N={c.N},{'packed' if c.packed else 'padded'},{A.dt_name(dt)},{'bounded' if bounded else 'online'}].{name}: "
                  f"bound {b:.3e} rms {rms:.3e} err without the tile {e_lost:.3f}")
            assert b <= 0.25, (name, b)
        assert rms > 0.0 and e_lost >= 0.5, (name, rms, e_lost)


def test_what_the_dense_long_stream_cases_see_of_a_lost_query_tile():
    """A figure, not a gate (it goes into profiles/attention_model.txt): how far the float64 dK / dV of the dense long-stream cases
    move when the last query tile is removed, next to the bound of that case.  Where the movement is below the bound the dense
    case alone would not catch that loss -- the one-tile probes are what does."""
    for row in A.long_stream_drop_figures():
        print("{case}.{name}: err without the last query tile {moved:.3e}, bound {bound:.3e}".format(**row))
        assert math.isfinite(row["moved"]) and row["moved"] > 0.0
