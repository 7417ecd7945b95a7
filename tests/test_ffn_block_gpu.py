"""-m gpu: the fused FFN block (csrc/ffn_infer.hip) against the float64 model of tests/ffn_block_model.py, element by element,
through ops.ffn_block / ops.ffn_block_grouped.  Metric and bound: see ffn_block_model.py -- `out` meets max(8 e_chain, 16 * 2^-24)
(+ 2^-8 for bf16) on EVERY element; nothing is fitted to what the kernel returns.  Operands are rounded to the compute type on both
sides; the models run on the device.

Shapes, from the kernel: a wave owns 32 rows, a workgroup 128 -> M = 1, 31, 32, 33, 127, 128, 129, 257; 210 (the image stream's
rows at B 4); 33 000 = 258 workgroups, more than the 256 CUs (one workgroup per CU: a second round).  The hidden index is walked in
32 groups through a ring of 4 (bf16) / 2 (fp32) weight buffers: the probes take the groups at both ends and one per ring stage."""
import ctypes

import pytest
import torch

from tests import ffn_block_model as Fm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
SENTINEL = 768.0                       # exact in bf16
ROWS = (1, 31, 32, 33, 127, 128, 129, 210, 257, 33000)


@pytest.fixture(scope="module")
def ops():
    from medical_tri_modal_pilot_amd import ops as _ops
    return _ops


def put(p, dt):
    """the models' CPU inputs -> the device: x, w1, w2 in the compute type (a column window of a wider buffer stays one), the rest fp32"""
    out = {}
    for k, t in p.items():
        cdt = dt if k in ("x", "w1", "w2") else F32
        if t.dim() == 2 and t._base is not None and not t.is_contiguous():
            off = t.storage_offset()
            out[k] = t._base.to(DEV, cdt)[:, off:off + t.shape[1]]
        else:
            out[k] = t.to(DEV, cdt)
    return out


def as_model(d):
    return {k: t.float() for k, t in d.items()}


def run(ops, d):
    return ops.ffn_block(d["x"], d["gamma"], d["beta"], d["w1"], d["c1"], d["w2"], d["c2"])


def check(tag, got, d, dt, **kw):
    """every element of `got` against the float64 model of the device operands d"""
    ref, e_chain = Fm.e_chain_of(as_model(d), dt, **kw)
    assert bool(torch.isfinite(got).all()), f"{tag}: not finite"
    e, b = Fm.err(got.double(), ref), Fm.bound(e_chain, dt == BF16)
    print(f"{tag}: err {e:.3e} e_chain {e_chain:.3e} bound {b:.3e} ratio {e / b:.3f}")
    assert e <= b, f"{tag}: err {e:.3e} > bound {b:.3e} (e_chain {e_chain:.3e})"
    return b


@pytest.mark.parametrize("dt", Fm.DTS, ids=Fm.dt_name)
@pytest.mark.parametrize("M", ROWS)
def test_rows(ops, M, dt):
    d = put(Fm.ffn_inputs(M, dt, seed=1), dt)
    got = run(ops, d)
    assert got.shape == (M, 256) and got.dtype == dt
    check(f"rows.{Fm.dt_name(dt)}.M{M}", got, d, dt)


@pytest.mark.parametrize("dt", Fm.DTS, ids=Fm.dt_name)
def test_strided_x(ops, dt):
    """x = the column window [8:264] of an [M, 320] buffer"""
    d = put(Fm.ffn_inputs(210, dt, seed=2, ldx=320), dt)
    assert d["x"].stride(0) == 320 and d["x"].storage_offset() == 8
    check(f"strided.{Fm.dt_name(dt)}", run(ops, d), d, dt)


def test_grouped_equals_singles(ops):
    """one grid over three streams = three single calls, bit for bit"""
    ds = [put(Fm.ffn_inputs(M, BF16, seed=3 + i), BF16) for i, M in enumerate((210, 1, 129))]
    singles = [run(ops, d) for d in ds]
    grouped = ops.ffn_block_grouped(*[[d[k] for d in ds] for k in ("x", "gamma", "beta", "w1", "c1", "w2", "c2")])
    for i, (s, g) in enumerate(zip(singles, grouped)):
        assert torch.equal(s, g), f"stream {i}"
    check("grouped.s0", grouped[0], ds[0], BF16)


@pytest.mark.parametrize("dt", Fm.DTS, ids=Fm.dt_name)
def test_deterministic(ops, dt):
    d = put(Fm.ffn_inputs(257, dt, seed=6), dt)
    assert torch.equal(run(ops, d), run(ops, d))


def test_rows_live(ops):
    """buffers of 300 rows, 130 live: NaN behind the live rows on the way in, the sentinel bit for bit on the way out"""
    from medical_tri_modal_pilot_amd import _lib
    d = put(Fm.ffn_inputs(300, BF16, seed=7), BF16)
    want = run(ops, {**d, "x": d["x"][:130]})
    x = d["x"].clone()
    x[130:] = float("nan")
    out = torch.full((300, 256), SENTINEL, dtype=BF16, device=DEV)
    pack = torch.tensor([0, 130, 0], dtype=torch.int32, device=DEV)           # row_starts() of one sample: pack[B] = rows in use
    ptr = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())
    ints = lambda v: (ctypes.c_int * 1)(v)
    _lib.call("mtmp_ffn_block_grouped", _lib.BF16, 1, ptr(x), ints(256), ptr(d["gamma"]), ptr(d["beta"]), ptr(d["w1"]), ptr(d["c1"]),
              ptr(d["w2"]), ptr(d["c2"]), ptr(out), ints(256), ints(300), ops.LN_EPS,
              (ctypes.c_void_p * 1)(pack.data_ptr() + 4), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(out[:130], want)
    assert bool((out[130:] == SENTINEL).all()), "rows at and behind the live count were written"
    # and through the wrapper, which takes the row_starts() tensor
    got = ops.ffn_block_grouped([x], [d["gamma"]], [d["beta"]], [d["w1"]], [d["c1"]], [d["w2"]], [d["c2"]], packs=[pack])[0]
    assert torch.equal(got[:130], want)


@pytest.mark.parametrize("dt", Fm.DTS, ids=Fm.dt_name)
@pytest.mark.parametrize("group", Fm.PROBE_GROUPS)
def test_one_group_probe(ops, group, dt):
    """the probed group carries most of the output: a kernel that loses it (or reads it from the wrong ring stage) cannot pass"""
    d = put(Fm.probe_inputs(dt, group), dt)
    m = as_model(d)
    ref = Fm.ffn_block_model(**m, dt=dt, ft=F64)["out"]
    lost = Fm.err(Fm.ffn_block_model(**m, dt=dt, ft=F64, without=group)["out"], ref)
    b = check(f"probe.{Fm.dt_name(dt)}.g{group}", run(ops, d), d, dt)
    print(f"probe g{group}: bound {b:.3e}, err without the group {lost:.3f}")
    assert b <= Fm.PROBE_BOUND and lost >= Fm.PROBE_LOSS
