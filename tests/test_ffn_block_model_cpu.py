"""CPU-only: the model of the fused FFN block (tests/ffn_block_model.py) on its own -- the working-precision chain stays close to the
float64 formula, and the one-group probes can tell a kernel that loses the probed group from a right one."""
import pytest
import torch

from tests import ffn_block_model as Fm

F64 = torch.float64


@pytest.mark.parametrize("dt", Fm.DTS, ids=Fm.dt_name)
def test_chain_against_float64(dt):
    p = Fm.ffn_inputs(210, dt, seed=1)
    ref, e_chain = Fm.e_chain_of(p, dt)
    print(f"{Fm.dt_name(dt)}: e_chain {e_chain:.3e} bound {Fm.bound(e_chain, dt == Fm.BF16):.3e}")
    assert ref.shape == (210, 256) and bool(torch.isfinite(ref).all())
    assert Fm.bound(e_chain, dt == Fm.BF16) < 0.25


@pytest.mark.parametrize("dt", Fm.DTS, ids=Fm.dt_name)
@pytest.mark.parametrize("group", Fm.PROBE_GROUPS)
def test_probe_conditions(group, dt):
    p = Fm.probe_inputs(dt, group)
    ref, e_chain = Fm.e_chain_of(p, dt)
    lost = Fm.err(Fm.ffn_block_model(**p, dt=dt, ft=F64, without=group)["out"], ref)
    b = Fm.bound(e_chain, dt == Fm.BF16)
    print(f"{Fm.dt_name(dt)} g{group}: bound {b:.3e} lost {lost:.3f}")
    assert b <= Fm.PROBE_BOUND and lost >= Fm.PROBE_LOSS


def test_without_removes_one_group_only():
    p = Fm.ffn_inputs(33, Fm.F32, seed=2)
    full = Fm.ffn_block_model(**p, dt=Fm.F32, ft=F64)["out"]
    w2 = p["w2"].clone()
    w2[:, 64:96] = 0
    assert torch.allclose(Fm.ffn_block_model(**p, dt=Fm.F32, ft=F64, without=2)["out"],
                          Fm.ffn_block_model(**dict(p, w2=w2), dt=Fm.F32, ft=F64)["out"], rtol=0, atol=1e-12)
    assert not torch.allclose(full, Fm.ffn_block_model(**p, dt=Fm.F32, ft=F64, without=2)["out"])
