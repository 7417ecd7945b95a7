"""-m gpu: the three-row LayerNorm head kernels (csrc/head3.hip: ops.TriHeadFn, ops.CandidateMeanFn, ops.BceMaskedMean) against
the torch module chain in float64 on the CPU.

Bounds: outputs, d cls_m and every parameter gradient 1e-4 relative to the tensor's scale (the project's fp32 bound, _rel below).
With bf16 CLS rows the reference is fed the same bf16 values upcast, and d cls_m -- which the kernels hand back IN bf16 -- is held to
1e-4 of the scale plus half a bf16 ulp of the element (at most 2^-8 |ref|, bf16 keeping 8 significant bits: the rounding to the output type, which no fp32 computation
avoids; the value in front of the rounding is what the 1e-4 is about).
Candidate mean: 1 ulp of the fp32 result of the reference's stack / mean / gather form.  Masked BCE: loss 1e-5 absolute (the bound
the step goldens use), dlogit 1e-6 relative and exactly 0 outside the sets.

ReLU gates: a pre-activation that rounds to the other side of 0 in fp32 would fail a gradient without a bug, so every case asserts --
on the CPU, from the float64 reference alone -- that no pre-activation of either ReLU lies within 1e-4 of zero.  The LayerNorm
weights / biases in front of the two ReLUs are drawn as |g| in [0.1, 0.3], |b| in [0.75, 1.2] (a gate flips where the normalised
value passes 2.5 .. 12: some gates depend on the sample, few values come near zero), and SEEDS below names, per batch size, the first
seed for which the margin holds for every variant of the case (found by tests/test_tri_head_gpu.py::find_seeds on the CPU).
"""
import functools
import math

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BATCHES = [1, 2, 3, 4, 5, 63, 64, 65, 128, 129, 256]
SEEDS = {1: 0, 2: 0, 3: 0, 4: 0, 5: 0, 63: 0, 64: 0, 65: 0, 128: 0, 129: 0, 256: 0}
GATE_MARGIN = 1e-4
SHARED_NAMES = ["demo.0.weight", "demo.0.bias", "demo.1.weight", "demo.1.bias", "ln.weight", "ln.bias"]
SET_NAMES = ["0.weight", "0.bias", "1.weight", "1.bias", "3.weight", "3.bias"]


def _rel(a, b):
    """max |a-b| / (max|b| + tiny): error relative to the tensor's scale (tests/test_gpu_parity.py)"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _gated(gen, n):
    """LayerNorm weight / bias in front of a ReLU: see the module docstring"""
    sign = lambda: (torch.randint(0, 2, (n,), generator=gen) * 2 - 1).double()
    g = (0.1 + 0.2 * torch.rand(n, generator=gen, dtype=torch.float64)) * sign()
    b = (0.75 + 0.45 * torch.rand(n, generator=gen, dtype=torch.float64)) * sign()
    return g, b


def _modules(gen, n_sets):
    """(ie_demo, layer_norms_after_concat, [fc_list] * n_sets) in float64 with seeded weights"""
    R = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    demo = nn.Sequential(nn.Linear(2, 256), nn.LayerNorm(256), nn.ReLU()).double()
    ln = nn.LayerNorm(256).double()
    heads = [nn.Sequential(nn.Linear(512, 256), nn.LayerNorm(256), nn.ReLU(), nn.Linear(256, 1)).double() for _ in range(n_sets)]
    with torch.no_grad():
        demo[0].weight.copy_(R(256, 2)), demo[0].bias.copy_(0.5 * R(256))
        g, b = _gated(gen, 256)
        demo[1].weight.copy_(g), demo[1].bias.copy_(b)
        ln.weight.copy_(1 + 0.2 * R(256)), ln.bias.copy_(0.2 * R(256))
        for fc in heads:
            fc[0].weight.copy_(R(256, 512) / math.sqrt(512.0)), fc[0].bias.copy_(0.1 * R(256))
            g, b = _gated(gen, 256)
            fc[1].weight.copy_(g), fc[1].bias.copy_(b)
            fc[3].weight.copy_(R(1, 256) / 16.0), fc[3].bias.copy_(R(1))
    return demo, ln, heads


def _param_list(demo, ln, heads):
    prm = [demo[0].weight, demo[0].bias, demo[1].weight, demo[1].bias, ln.weight, ln.bias]
    for fc in heads:
        prm += [fc[0].weight, fc[0].bias, fc[1].weight, fc[1].bias, fc[3].weight, fc[3].bias]
    return prm


def _inputs(gen, B, dt):
    cls = 1.5 * torch.randn(3, B, 256, generator=gen) + 0.3
    cls = cls.to(dt).float()                                        # bf16 cases: the same rounded values on both sides
    age, gender = torch.rand(B, generator=gen), torch.randint(0, 2, (B,), generator=gen).float()
    w = torch.randn(3, B, generator=gen)
    return cls, age, gender, w


@functools.lru_cache(maxsize=None)
def reference(B, dt, n_sets, seed=None):
    """The float64 torch chain of one case, computed once and shared: inputs, parameters, logits, d cls, parameter gradients and the
    smallest |pre-activation| of the two ReLUs."""
    gen = torch.Generator().manual_seed(1000 * B + (SEEDS[B] if seed is None else seed))
    demo, ln, heads = _modules(gen, n_sets)
    cls, age, gender, w = _inputs(gen, B, dt)
    c64 = cls.double().requires_grad_()
    demo_pre = demo[:2](torch.stack([age, gender], 1).double())
    x = torch.cat([ln(c64), demo[2](demo_pre).unsqueeze(0).expand(3, -1, -1)], dim=2)
    pres = [heads[m % n_sets][:2](x[m]) for m in range(3)]
    o = torch.stack([heads[m % n_sets][3](heads[m % n_sets][2](pres[m])).squeeze(-1) for m in range(3)])
    prm = _param_list(demo, ln, heads)
    grads = torch.autograd.grad((o * w.double()).sum(), [c64] + prm)
    margin = min(float(demo_pre.detach().abs().min()), min(float(p.detach().abs().min()) for p in pres))
    return dict(cls=cls, age=age, gender=gender, w=w, params=[p.detach() for p in prm], o=o.detach(), dcls=grads[0],
                grads=list(grads[1:]), margin=margin)


def find_seeds(limit=200):
    """(CPU, not a test) the first seed per batch size whose margin holds for fp32 and bf16 CLS rows, shared and separate heads"""
    out = {}
    for B in BATCHES:
        out[B] = next(s for s in range(limit) if all(reference(B, dt, n, s)["margin"] > GATE_MARGIN
                                                     for dt in (torch.float32, torch.bfloat16) for n in (1, 3)))
    return out


def _device_case(ref, dt, N):
    """CLS rows as strided views of [B, N, 256] tensors in the stack's type, parameters as fp32 leaves on the device"""
    B = ref["cls"].shape[1]
    g = torch.Generator().manual_seed(5)
    full = [torch.randn(B, N, 256, generator=g).to(dt).to(DEV) for _ in range(3)]
    for m in range(3):
        full[m][:, 0, :] = ref["cls"][m].to(dt).to(DEV)
        full[m].requires_grad_()
    prm = [nn.Parameter(p.float().to(DEV)) for p in ref["params"]]
    return full, ref["age"].to(DEV), ref["gender"].to(DEV), ref["w"].to(DEV), prm


def _run(ops, full, age, gender, w, prm):
    o = ops.TriHeadFn.apply(full[0][:, 0, :], full[1][:, 0, :], full[2][:, 0, :], age, gender, *prm)
    got = torch.autograd.grad((o * w).sum(), full + prm, allow_unused=True)
    return o.detach(), [g[:, 0, :] for g in got[:3]], [got[i][:, 1:, :] for i in range(3)], list(got[3:])


@pytest.fixture(scope="module")
def ops():
    from medical_tri_modal_pilot_amd import ops as _ops
    return _ops


@pytest.mark.parametrize("N", [1, 7])
@pytest.mark.parametrize("n_sets", [1, 3], ids=["shared", "three"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B", BATCHES)
def test_head_against_float64_chain(ops, B, dt, n_sets, N):
    from medical_tri_modal_pilot_amd.optim import FlatParams
    ref = reference(B, dt, n_sets)
    assert ref["margin"] > GATE_MARGIN, f"a ReLU pre-activation lies {ref['margin']:.2e} from zero: pick another seed (find_seeds)"
    full, age, gender, w, prm = _device_case(ref, dt, N)
    o, dcls, drest, grads = _run(ops, full, age, gender, w, prm)                    # plain autograd: fresh gradient tensors
    print(f"B={B} {dt} sets={n_sets} N={N}: o {_rel(o, ref['o']):.2e}")
    assert _rel(o, ref["o"]) <= 1e-4
    names = SHARED_NAMES + [f"fc{m}.{n}" for m in range(n_sets) for n in SET_NAMES]
    for m in range(3):
        assert dcls[m].dtype == dt and (N == 1 or float(drest[m].abs().max()) == 0.0)
        r = ref["dcls"][m]
        err = (dcls[m].double().cpu() - r).abs()
        bound = 1e-4 * r.abs().max() + (0.0 if dt == torch.float32 else 2.0 ** -8 * r.abs())
        print(f"  dcls{m} {float(err.max() / r.abs().max()):.2e}")
        assert bool((err <= bound).all()), (m, float((err - bound).max()))
    for n, g, r in zip(names, grads, ref["grads"]):
        print(f"  {n} {_rel(g, r):.2e}")
        assert g.shape == r.shape and _rel(g, r) <= 1e-4, (n, _rel(g, r))
    # the same through a FlatParams sink: the kernels write the slices of the flat gradient buffer, autograd sees None
    full2, _, _, _, prm2 = _device_case(ref, dt, N)
    flat = FlatParams([(n, p) for n, p in zip(names, prm2)])
    flat.zero_grad()
    o2, dcls2, _, g2 = _run(ops, full2, age, gender, w, prm2)
    assert all(g is None for g in g2) and flat.written == set(range(len(prm2)))
    assert torch.equal(o2, o) and all(torch.equal(a, b) for a, b in zip(dcls2, dcls))
    for n, p, g in zip(names, prm2, grads):
        assert torch.equal(p.grad, g), n                                             # same kernels, same bits, other destination


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B", [5, 129])
def test_shared_head_equals_three_equal_heads(ops, B, dt):
    """one shared parameter set == three sets loaded with the same weights: logits and d cls bit for bit, the shared set's gradient
    the three sets' gradients summed in the order m = 0, 1, 2"""
    ref = reference(B, dt, 1)
    full, age, gender, w, prm = _device_case(ref, dt, 7)
    o1, dcls1, _, g1 = _run(ops, full, age, gender, w, prm)
    prm3 = prm[:6] + [nn.Parameter(p.detach().clone()) for _ in range(3) for p in prm[6:]]
    o3, dcls3, _, g3 = _run(ops, full, age, gender, w, prm3)
    assert torch.equal(o1, o3) and all(torch.equal(a, b) for a, b in zip(dcls1, dcls3))
    for i in range(6):
        assert torch.equal(g1[i], g3[i]), SHARED_NAMES[i]
        assert torch.equal(g1[6 + i], (g3[6 + i] + g3[12 + i]) + g3[18 + i]), SET_NAMES[i]


def _mixed_ids(B, lo=0, hi=4, seed=3):
    ids = torch.randint(lo, hi, (B,), generator=torch.Generator().manual_seed(seed))
    ids[: min(B, hi - lo)] = torch.arange(lo, lo + min(B, hi - lo))
    return ids


@pytest.mark.parametrize("B", [8, 300])
def test_candidate_mean(ops, B):
    """every pattern id, and ids 4 .. 7 for bounds safety (read as id & 3), against the reference's stack / mean / gather in fp32"""
    g = torch.Generator().manual_seed(B)
    o = torch.randn(3, B, generator=g)
    w = torch.randn(B, generator=g)
    ids = _mixed_ids(B, 0, 8)
    assert set(ids.tolist()) == set(range(8))
    oc = o.clone().requires_grad_()
    ref = ops.candidate_mean(oc, ids & 3)                                     # (CPU tensors: the torch form)
    (dref,) = torch.autograd.grad((ref * w).sum(), oc)
    od = o.to(DEV).requires_grad_()
    out = ops.CandidateMeanFn.apply(od, ids.to(DEV))
    (dgot,) = torch.autograd.grad((out * w.to(DEV)).sum(), od)
    ulp = lambda t: (torch.nextafter(t.abs(), torch.full_like(t, math.inf)) - t.abs())
    assert bool(((out.cpu() - ref.detach()).abs() <= ulp(ref.detach())).all())
    assert bool(((dgot.cpu() - dref).abs() <= ulp(dref)).all())
    present = torch.stack([torch.ones(B, dtype=torch.bool), (ids & 3) < 2, (ids & 1) == 0])
    assert bool((dgot.cpu()[~present] == 0).all()) and bool((dgot.cpu()[present] != 0).all())


@pytest.mark.parametrize("ids_kind", ["every_set", "all_full", "all_vslt_only"])
@pytest.mark.parametrize("B", [7, 300])
def test_masked_bce(ops, B, ids_kind):
    g = torch.Generator().manual_seed(B + 1)
    o = 2.0 * torch.randn(3, B, generator=g)
    y = torch.randint(0, 2, (B,), generator=g).float()
    ids = {"every_set": _mixed_ids(B), "all_full": torch.zeros(B, dtype=torch.long), "all_vslt_only": torch.full((B,), 3)}[ids_kind]
    mask = torch.stack([torch.ones(B, dtype=torch.bool), ids < 2, (ids & 1) == 0])
    o64 = o.double().requires_grad_()
    ref = nn.BCEWithLogitsLoss()(o64[mask], y.double().unsqueeze(0).expand(3, -1)[mask])
    (dref,) = torch.autograd.grad(ref, o64)
    od = o.to(DEV).requires_grad_()
    loss = ops.bce_masked_mean(nn.BCEWithLogitsLoss(), od, y.to(DEV), ids.to(DEV))
    assert loss.grad_fn is not None and type(loss.grad_fn).__name__.startswith("BceMaskedMean")
    (dgot,) = torch.autograd.grad(loss, od, ops.unit_grad(loss))
    print(f"B={B} {ids_kind}: loss err {abs(float(loss.detach()) - float(ref.detach())):.2e}, dlogit {_rel(dgot, dref):.2e}")
    assert abs(float(loss) - float(ref)) <= 1e-5
    assert _rel(dgot, dref) <= 1e-6
    assert bool((dgot.cpu()[~mask] == 0).all())
    # a scaled incoming gradient takes the multiplying branch; the CPU / other-criterion form is the boolean-index one
    (d2,) = torch.autograd.grad(ops.bce_masked_mean(nn.BCEWithLogitsLoss(), od, y.to(DEV), ids.to(DEV)) * 3.0, od)
    assert _rel(d2, 3.0 * dref) <= 1e-6
    cpu = ops.bce_masked_mean(nn.BCEWithLogitsLoss(), o, y, ids)
    assert abs(float(cpu) - float(ref)) <= 1e-5
    summed = ops.bce_masked_mean(nn.BCEWithLogitsLoss(reduction="sum"), od, y.to(DEV), ids.to(DEV))
    assert abs(float(summed) / int(mask.sum()) - float(ref)) <= 1e-5


def _chain(ops, full, age, gender, y, ids, prm):
    """forward + masked BCE + backward of the three functions (the candidate mean's upstream gradient: its own output)"""
    o = ops.TriHeadFn.apply(full[0][:, 0, :], full[1][:, 0, :], full[2][:, 0, :], age, gender, *prm)
    loss = ops.bce_masked_mean(nn.BCEWithLogitsLoss(), o, y, ids)
    mean = ops.CandidateMeanFn.apply(o, ids)
    g_loss = torch.autograd.grad(loss, full + prm, ops.unit_grad(loss), retain_graph=True)
    (g_mean,) = torch.autograd.grad(mean, o, mean.detach())
    return [o.detach(), loss.detach(), mean.detach(), g_mean] + list(g_loss)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_two_runs_are_bit_identical(ops, dt):
    ref = reference(65, dt, 3)
    full, age, gender, _, prm = _device_case(ref, dt, 7)
    y, ids = (ref["w"][0] > 0).float().to(DEV), _mixed_ids(65).to(DEV)
    a = _chain(ops, full, age, gender, y, ids, prm)
    b = _chain(ops, full, age, gender, y, ids, prm)
    assert all(torch.equal(s, t) for s, t in zip(a, b))


def test_chain_replays_from_a_captured_graph(ops):
    """forward + masked BCE + backward of the three functions recorded with torch.cuda.graph on static buffers (one stream: one
    chain of launches, nothing forks), replayed twice with other inputs copied in: bit-equal to the eager chain on those inputs."""
    B, dt = 65, torch.bfloat16
    cases = [reference(65, dt, 3), reference(65, dt, 3, seed=SEEDS[65] + 1000)]
    full, age, gender, _, prm = _device_case(cases[0], dt, 7)
    y, ids = (cases[0]["w"][0] > 0).float().to(DEV), _mixed_ids(B).to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _chain(ops, full, age, gender, y, ids, prm)                                  # warm-up: unit_grad and the allocator's pool
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = _chain(ops, full, age, gender, y, ids, prm)
    for k, c in enumerate(cases[::-1] + cases[:1]):
        f2, a2, g2, _, _ = _device_case(c, dt, 7)
        y2, i2 = (c["w"][0] > 0).float().to(DEV), _mixed_ids(B, seed=10 + k).to(DEV)
        with torch.no_grad():
            for m in range(3):
                full[m].copy_(f2[m])
            age.copy_(a2), gender.copy_(g2), y.copy_(y2), ids.copy_(i2)
        graph.replay()
        eager = _chain(ops, f2, a2, g2, y2, i2, prm)
        torch.cuda.synchronize()
        for s, e in zip(static_out, eager):
            assert torch.equal(s, e)
