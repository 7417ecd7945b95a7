"""Pins tests/row_kernels_model.py -- the float64 references, the metric, the input generator and the tolerance's e_torch -- against
independent formulations, so that the references cannot be wrong together with the kernels.  Runs without a GPU."""
import math
import os

import numpy as np
import pytest
import torch

import filler
from oracle import tri_mbt_oracle as O
from tests import row_kernels_model as R

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIGHT = 1e-11            # two float64 formulations of one expression


# ------------------------------------------------------------------------------------------ the metric
def test_metric_is_element_wise():
    g = torch.Generator().manual_seed(1)
    ref = torch.randn(64, 256, generator=g, dtype=F64) * 100
    ref[5, 7] = 1e-3                                          # one small element inside a large tensor
    rms = float(ref.pow(2).mean().sqrt())
    assert R.err(ref.clone(), ref) == 0.0
    got = ref.clone()
    got[5, 7] += 0.02                                         # wrong by 20x its own size
    assert float((got - ref).abs().max() / ref.abs().max()) < 1e-4          # the max-norm check at 1e-4 lets it through
    assert R.err(got, ref) == pytest.approx(0.02 / (1e-3 + rms), rel=1e-9)
    assert R.err(got, ref) > 10 * R.bound(2.4e-6)                           # the element-wise bound does not, at any e_torch met here
    got = ref.clone()
    got[9, 9] *= 1 + 1e-3                                     # a large element wrong by 1e-3 of itself
    assert R.err(got, ref) == pytest.approx(1e-3 * abs(float(ref[9, 9])) / (abs(float(ref[9, 9])) + rms), rel=1e-6)


def test_metric_edges():
    z = torch.zeros(4, 4)
    assert R.err(z, z) == 0.0
    assert R.err(z + 1e-30, z) == math.inf                    # an all-zero reference admits no difference
    assert R.err(torch.full((3,), float("nan")), torch.ones(3)) == math.inf
    assert R.err(torch.zeros(0, 256), torch.zeros(0, 256)) == 0.0
    with pytest.raises(AssertionError):
        R.err(torch.zeros(3), torch.zeros(4))
    # one dropped row of M in a column sum shifts it by ~1/sqrt(M) of its scale: at 33 000 rows that is far above the bound and
    # still under the 1e-2 the max-norm checks allow a bf16 gradient
    g = torch.Generator().manual_seed(2)
    x = torch.randn(33000, 256, generator=g, dtype=F64)
    full, short = x.sum(0), x[:-1].sum(0)
    assert R.err(short, full) > 100 * R.bound(4e-7)
    assert float((short - full).abs().max() / full.abs().max()) < 1e-2


def test_bound():
    assert R.bound(0.0) == 16 * 2.0 ** -24
    assert R.bound(1e-6) == 8e-6
    assert R.bound(1e-6, bf16_out=True) == 8e-6 + 2.0 ** -8
    assert R.bound(1e-8) == R.FLOOR


# ------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("M", [1, 17, 300])
@pytest.mark.parametrize("res", [False, True])
def test_ln_model_vs_oracle_autograd(M, res):
    g = torch.Generator().manual_seed(3 + M)
    z = (torch.randn(M, 256, generator=g, dtype=F64) * 2 + 0.3).requires_grad_()
    gam = (1 + 0.1 * torch.randn(256, generator=g, dtype=F64)).requires_grad_()
    bet = torch.zeros(256, dtype=F64, requires_grad=True)
    dy = torch.randn(M, 256, generator=g, dtype=F64)
    dres = torch.randn(M, 256, generator=g, dtype=F64) if res else None
    (O.custom_layernorm(z, gam, bet) * dy).sum().backward()
    zd = z.detach()
    stats = torch.stack([zd.mean(-1), 1 / (zd.std(-1) + 1e-6)], 1)           # exact statistics: the two must agree to float64 round-off
    m = R.ln_bwd_model(zd, stats, gam.detach(), dy, dres, ft=F64)
    assert R.err(m["dz"], z.grad + (dres if res else 0)) < TIGHT
    assert R.err(m["dgamma"], gam.grad) < TIGHT and R.err(m["dbeta"], bet.grad) < TIGHT
    # with the fp32 statistics the kernel is given, the model moves by their rounding and no more
    m32 = R.ln_bwd_model(zd, R.ln_stats(zd), gam.detach(), dy, dres, ft=F64)
    assert R.err(m32["dz"], m["dz"]) < 2e-6 and R.err(m32["dgamma"], m["dgamma"]) < 2e-6


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("use_pe", [False, True])
def test_stream_input_model_vs_torch_chain(dt, use_pe):
    """the op chain of test_stream_input_vs_torch_chain (cat CLS -> F.layer_norm -> + sinusoid rows, bottleneck rows in front)"""
    g = torch.Generator().manual_seed(5 + int(use_pe))
    B, N, nb = 3, 37, 4
    x = torch.randn(B, N, 256, generator=g).to(dt)
    cls, gam, bet = torch.randn(1, 1, 256, generator=g), 1 + 0.1 * torch.randn(256, generator=g), 0.1 * torch.randn(256, generator=g)
    bott = torch.randn(1, nb, 256, generator=g)
    pe = O.sinusoid_table(2500, 256)[:N + 1] if use_pe else None
    w = torch.randn(B, nb + 1 + N, 256, generator=g)
    for ft, tol in ((F64, TIGHT), (F32, 1e-5)):
        xr, cr, gr, br, tr = (t.clone().to(ft).requires_grad_() for t in (x, cls, gam, bet, bott))
        c = cr + (cr.to(dt).to(ft) - cr).detach()        # (the cast's own backward would round the gradient to dt as well)
        xc = torch.cat([c.expand(B, -1, -1), xr], 1)
        y = torch.nn.functional.layer_norm(xc, (256,), gr, br, 1e-5)
        if use_pe:
            y = y + pe[None].to(ft)
        z_ref = torch.cat([tr.expand(B, -1, -1), y], 1)
        (z_ref * w.to(ft)).sum().backward()
        m = R.stream_input_model(x.float(), cls, gam, bet, pe, bott, w, dt=dt, ft=F64)
        for name, a in (("z", z_ref), ("dx", xr.grad), ("dcls", cr.grad.view(-1)), ("dgamma", gr.grad), ("dbeta", br.grad),
                        ("dbott", tr.grad.view(nb, 256))):
            assert R.err(a, m[name]) < tol, (name, ft)
    assert torch.equal(R.sinusoid_table(300), O.sinusoid_table(300, 256))


def test_stream_input_model_packed_counts_live_rows_only():
    B, N, nb, kv = R.STREAM_PACKED
    c = R.stream_case(B, N, nb, False, F32, kv)
    ref = c["ref"]
    assert ref["live"].sum() == sum(kv) and not ref["live"][1, 5:].any() and ref["live"][0].all()
    pad_tok = ~ref["live"][:, nb + 1:]
    assert float(ref["dx"][pad_tok].abs().sum()) == 0.0 and float(ref["dx"][~pad_tok].abs().min()) > 0.0
    # the same parameter gradients from the live rows alone, sample by sample
    tot = {k: 0 for k in ("dbott", "dgamma", "dbeta", "dcls")}
    for b, k in enumerate(kv):
        one = R.stream_input_model(c["x"][b:b + 1, :k - nb - 1], c["cls"], c["gamma"], c["beta"], None, c["bott"], c["w"][b:b + 1, :k],
                                   dt=F32, ft=F64)
        for name in tot:
            tot[name] = tot[name] + one[name]
    for name in tot:
        assert R.err(tot[name], ref[name]) < TIGHT, name


def _golden_tie():
    Gd = np.load(os.path.join(ROOT, "tests", "golden", "model_step.npz"), allow_pickle=False)
    names = ["ie_vslt.0.weight", "ie_vslt.0.bias", "ie_vslt.1.weight", "ie_vslt.1.bias", "ie_time.0.weight", "ie_time.0.bias",
             "ie_time.1.weight", "ie_time.1.bias", "ie_feat.weight"]
    shapes = [(256, 1), (256,), (256,), (256,), (256, 1), (256,), (256,), (256,), (20, 256)]
    prm = [filler.fill_tensor(k, torch.zeros(s)) for k, s in zip(names, shapes)]
    bt = filler.make_batch(int(Gd["seed"]), int(Gd["B"]), int(Gd["T"]))
    return Gd, prm, bt["x"].float().reshape(-1, 3)


def test_tie_model_vs_golden():
    """the golden vectors were written by the reference in fp32: agreement to its own round-off (the existing GPU test's 1e-4 max-norm
    is kept as the structural check, the element-wise figure is printed)"""
    Gd, prm, ev = _golden_tie()
    w = torch.from_numpy(Gd["tie_w"]).reshape(-1, 256)
    m = R.tie_model(ev, prm, w, ft=F64)
    for name, key, shape in (("out", "tie_emb", (-1, 256)), ("dWv", "tie_dWv", (256, 1)), ("dbt", "tie_dbt", (256,)),
                             ("dgv", "tie_dgv", (256,)), ("dF", "tie_dF", (20, 256))):
        ref = torch.from_numpy(Gd[key]).double().reshape(shape)
        e = float((m[name] - ref).abs().max() / ref.abs().max())
        print(f"tie model vs golden {name}: max-norm {e:.2e}, element-wise {R.err(ref, m[name]):.2e}")
        assert e < 1e-5, name
    o = O.tie_embedding({k: v.double() for k, v in zip(["ie_vslt.0.weight", "ie_vslt.0.bias", "ie_vslt.1.weight", "ie_vslt.1.bias",
                                                        "ie_time.0.weight", "ie_time.0.bias", "ie_time.1.weight", "ie_time.1.bias",
                                                        "ie_feat.weight"], prm)}, ev.double().unsqueeze(0))[0]
    assert R.err(m["out"], o) < TIGHT


def test_time_model_is_the_tie_model_without_the_value_chain():
    c = R.tie_case(5, F32, False)
    m = c["ref"]
    for k in ("dWv", "dbv", "dgv", "dhv"):
        assert float(m[k].abs().sum()) == 0.0
    P = [p.double() for p in c["prm"]]
    ev = c["ev"]
    tim = torch.relu(torch.nn.functional.layer_norm(ev[:, :1].double() * P[4].view(1, -1) + P[5], (256,), P[6], P[7], 1e-5))
    assert R.err(m["out"], tim + P[8][ev[:, 2].long()]) < TIGHT


@pytest.mark.parametrize("resbottle", [False, True])
def test_exchange_model_vs_oracle_expression(resbottle):
    """oracle.tri_mbt_oracle.mbt_encoder's exchange (mbt_encoder.py:764-779) for all four patterns, and its autograd"""
    g = torch.Generator().manual_seed(11)
    B = 8
    missing = torch.tensor([0, 1, 2, 3, 3, 2, 1, 0])
    b_out = [torch.randn(B, 4, 256, generator=g, dtype=F64).requires_grad_() for _ in range(3)]
    res = torch.randn(B, 4, 256, generator=g, dtype=F64).requires_grad_() if resbottle else None
    d_rows = [torch.randn(B, 4, 256, generator=g, dtype=F64) for _ in range(3)]
    d_prev = torch.randn(B, 4, 256, generator=g, dtype=F64)
    st = torch.stack(b_out)
    cand = torch.stack([st.mean(0), st[:2].mean(0), torch.stack([st[0], st[2]]).mean(0), st[0]])
    bott = cand[missing, torch.arange(B)]
    if resbottle:
        bott = torch.stack([bott, res]).mean(0)
    (bott * (sum(d_rows) + d_prev)).sum().backward()
    m = R.exchange_model([t.detach() for t in b_out], missing, None if res is None else res.detach(), d_rows, d_prev, ft=F64)
    assert R.err(m["new"], bott) < TIGHT
    for k in range(3):
        assert R.err(m[f"d{k}"], b_out[k].grad) < TIGHT
    if resbottle:
        assert R.err(m["d_prev"], res.grad) < TIGHT
    # two streams (mbt_encoder.py:629-632): candidates (mean of both, stream 0) = rows 1 and 3 of the table
    two = torch.stack([st[:2].mean(0), st[0]])[torch.tensor([0, 1, 1, 0, 0, 1, 0, 1]), torch.arange(B)].detach()
    m2 = R.exchange_model([t.detach() for t in b_out[:2]], torch.tensor([1, 3, 3, 1, 1, 3, 1, 3]), None, d_rows[:2], None, ft=F64)
    assert R.err(m2["new"], two) < TIGHT


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adamw_model_vs_torch_optim(wd):
    g = torch.Generator().manual_seed(13)
    p = torch.nn.Parameter(torch.randn(1000, generator=g, dtype=F64))
    opt = torch.optim.AdamW([p], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    q, m, v = p.detach().clone(), torch.zeros(1000, dtype=F64), torch.zeros(1000, dtype=F64)
    for step in range(1, 6):
        gr = torch.randn(1000, generator=g, dtype=F64)
        p.grad = gr.clone()
        opt.step()
        r = R.adamw_model(q, gr * 4, m, v, 1e-3, 0.9, 0.999, 1e-8, wd, step, 0.25, ft=F64)
        assert R.err(r["update"], r["param"] - q) < 1e-9               # (the difference loses digits to the parameter's size)
        q, m, v = r["param"], r["exp_avg"], r["exp_avg_sq"]
        assert R.err(q, p.detach()) < TIGHT
        assert R.err(m, opt.state[p]["exp_avg"]) < TIGHT and R.err(v, opt.state[p]["exp_avg_sq"]) < TIGHT
    assert R.f32_scalar(0.999) == float(np.float32(0.999)) != 0.999


def test_sum_models():
    g = torch.Generator().manual_seed(17)
    s = torch.randn(37, 12, generator=g)
    assert R.err(R.column_sum_model(s, ft=F64)["sum"], torch.stack([s[:, c].double().sum() for c in range(12)])) < TIGHT
    dx = torch.randn(15, 256, generator=g)
    ref = torch.stack([dx[0:5].double().sum(0), dx[5:10].double().sum(0), dx[10:15].double().sum(0)])
    assert R.err(R.token_sums_model(dx, 5, ft=F64)["sum"], ref) < TIGHT


# ------------------------------------------------------------------------------------------ the input generator
def test_tie_events_resampling():
    prm = R.tie_params(R.TIE_PARAM_SEED)
    ev, rounds = R.tie_events(8197, prm, 3000 + 8197)
    print("resampled per round at n = 8197:", rounds)
    assert rounds[-1] == 0 and rounds[0] <= R.RESAMPLE_CAP * 8197
    assert not R.tie_near_zero(ev, prm).any()                           # the property, on the final inputs
    P = [p.double() for p in prm]
    for chain in (0, 1):
        assert float(R._tie_pre(ev, P, chain).abs().min()) >= R.RELU_MARGIN
    ev2, rounds2 = R.tie_events(8197, prm, 3000 + 8197)
    assert torch.equal(ev, ev2) and rounds == rounds2                   # same seed, same events
    assert not torch.equal(ev, R.tie_events(8197, prm, 1)[0])
    idx = ev[:, 2].long()
    assert set(idx.tolist()) == set(range(20)) and int((idx == 5).sum()) == 1
    assert torch.equal(ev[:, :2], ev[:, :2].half().float()) and float(ev[:, 0].min()) >= -24 and float(ev[:, 0].max()) <= 0
    # parameters that put a whole chain on the ReLU edge trip the cap
    bad = [p.clone() for p in prm]
    bad[2][:] = 0
    bad[3][:] = 0
    with pytest.raises(AssertionError, match="inside the ReLU margin"):
        R.tie_events(64, bad, 1)


def test_every_tie_case_respects_the_relu_margin():
    cases = [R.tie_case(n, F32) for n in R.TIE_SIZES] + [R.tie_case(n, F32, False) for n in R.TIME_SIZES]
    cases += [R.tie_case(n, F32, True, n2) for n, n2, _ in R.TIE_TIME_CASES] + [R.tie_packed_case(F32)]
    for c in cases:
        value = float(c["ev"][:, 1].abs().sum()) > 0
        assert not R.tie_near_zero(c["ev"], c["prm"], value).any()
        assert c["rounds"][0] <= R.RESAMPLE_CAP * c["ev"].shape[0]
        if c.get("tev") is not None:
            assert not R.tie_near_zero(c["tev"], c["prm"], False).any()
            assert c["rounds_t"][0] <= R.RESAMPLE_CAP * c["tev"].shape[0]


# ------------------------------------------------------------------------------------------ e_torch of every case
def _all_cases():
    for dt in R.DTS:
        d = R.dt_name(dt)
        for M, v in R.LN_CASES:
            yield f"ln_bwd[{M},{v},{d}]", lambda M=M, v=v, dt=dt: R.ln_case(M, v, dt)
        for c in R.STREAM_CASES:
            yield f"stream_in[{c[0]}x{c[1]}+{c[2]},{d}]", lambda c=c, dt=dt: R.stream_case(*c, dt)
        B, N, nb, kv = R.STREAM_PACKED
        yield f"stream_in_packed[{d}]", lambda dt=dt: R.stream_case(B, N, nb, False, dt, kv)
        for n in R.TIE_SIZES:
            yield f"tie[{n},{d}]", lambda n=n, dt=dt: R.tie_case(n, dt)
        for n in R.TIME_SIZES:
            yield f"time[{n},{d}]", lambda n=n, dt=dt: R.tie_case(n, dt, False)
        for n, n2 in sorted({c[:2] for c in R.TIE_TIME_CASES}):
            yield f"tie_time[{n}+{n2},{d}]", lambda n=n, n2=n2, dt=dt: R.tie_case(n, dt, True, n2)
        yield f"tie_packed[{d}]", lambda dt=dt: R.tie_packed_case(dt)
        for L in R.TOKEN_L:
            yield f"token_sums[L={L},{d}]", lambda L=L, dt=dt: R.token_case(L, 3, dt)
        for nr in R.EXCHANGE_ROWS:
            for rb, pi, two in ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 0, 1)):
                yield f"exchange[{nr},res={rb},prev_in={pi},two={two},{d}]", lambda a=(nr, rb, pi, two), dt=dt: R.exchange_case(*a, dt)
    for rows in R.REDUCE_ROWS:
        for ld in (512, 770, 1792):
            yield f"reduce[{rows}x{ld}]", lambda rows=rows, ld=ld: R.reduce_case(rows, ld)
    yield "reduce[256 x wide]", lambda: R.reduce_case(256, R.REDUCE_WIDE_COLS)
    for n in R.ADAMW_N:
        for step, wd, gs, _ in R.ADAMW_RUNS:
            yield f"adamw[{n},step={step},wd={wd},gs={gs}]", lambda a=(n, step, wd, gs): R.adamw_case(*a)


def test_e_torch_of_every_case_is_finite_and_small():
    worst = 0.0
    print()
    for name, make in _all_cases():
        et = make()["e_torch"]
        et = et if isinstance(et, dict) else {"sum": et}
        print(f"{name:48s} " + " ".join(f"{k}={v:.1e}" for k, v in et.items()))
        for k, v in et.items():
            assert math.isfinite(v) and v < 1e-5, (name, k, v)
            worst = max(worst, v)
    print(f"largest e_torch {worst:.2e} -> largest fp32 bound {R.bound(worst):.2e}")
