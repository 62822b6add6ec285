"""CPU: the emulation of the "f16x2" precision mode (tests/tail_split_emulation.py; contract: csrc/srbh_ptail_split.hip).

What is pinned here, from CPU values alone: with both splits off the emulation IS the default one; the full split leaves only the trunk's own
error at the final map (within 5 % of an exact tail behind the same trunk, >= 10 x below the default mode); and the 2^11 scale of the low parts
makes that independent of how a matrix core treats fp16 subnormals (every subnormal operand flushed: still <= 1.5e-4).

Measured: (1337,init,1337) default 7.166e-4, tail exact 4.929e-5, f16x2 4.930e-5 (14.5 x); (3,stress,77) 6.413e-4, 5.736e-5, 5.736e-5 (11.2 x);
flushed: 1.263e-4 / 1.164e-4 with scaled low parts, 6.012e-4 / 5.086e-4 with unscaled ones."""
import pytest
import torch

from oracle import srbh_oracle as O
from oracle import synth
from oracle.rrdbnet_emulation import rrdbnet_emulated
from tests import tail_split_emulation as E

DRAWS = [(1337, "init", 1337), (3, "stress", 77)]
_cache = {}


def draw(wseed, mode, xseed):
    """23 blocks, one 64x64 tile (tile 0 of the bench batch for seed 1337): state dict, tile, emulated bf16 trunk, exact network"""
    key = (wseed, mode, xseed)
    if key not in _cache:
        sd = synth.rrdbnet_state_dict(seed=wseed, mode=mode)
        x = synth.tiles(1, 8, 64, seed=xseed)[:, :3].contiguous()
        _cache[key] = (sd, x, E.trunk_and_feat(sd, x, "bf16"), rrdbnet_emulated(sd, x, None))
    return _cache[key]


@pytest.mark.parametrize("nb,hw", [(2, 24), (0, 16)])
def test_both_splits_off_is_the_default_emulation(nb, hw):
    sd = synth.rrdbnet_state_dict(num_block=nb, seed=12, mode="stress")
    x = synth.tiles(2, 3, hw, seed=13)
    for acc in (torch.float64, torch.float32):
        got = E.rrdbnet_emulated_f16x2(sd, x, "bf16", acc=acc, split_w=False, split_a=False)
        assert torch.equal(got, rrdbnet_emulated(sd, x, "bf16", acc=acc))
    assert not torch.equal(E.rrdbnet_emulated_f16x2(sd, x, "bf16"), rrdbnet_emulated(sd, x, "bf16"))


def test_split_is_exact_on_fp32_values():
    """hi + lo' * 2^-11 carries 22 bits of an fp32 value (|v| >= 2^-13): |v - (hi + lo' 2^-11)| <= 2^-22 |v|; |lo'| <= |v|; and a lo' that is an
    fp16 subnormal stands for a residual below 2^-25 (a quarter of the smallest ulp in that range): flushing it costs nothing that matters"""
    g = torch.Generator().manual_seed(5)
    v = (torch.randn(1 << 16, generator=g) * torch.exp2(torch.randint(-13, 14, (1 << 16,), generator=g).float())).float()
    v = v[v.abs() >= 2.0 ** -13]
    hi, lo = E.split16(v)
    assert ((v - (hi.double() + lo.double() / 2048)).abs() <= v.abs().double() * 2.0 ** -22).all()
    assert (lo.abs() <= v.abs()).all()
    sub = lo.abs() < E.F16_MIN_NORMAL
    assert ((v - hi).abs()[sub] < 2.0 ** -25).all()


@pytest.mark.parametrize("wseed,mode,xseed", DRAWS)
def test_full_split_reaches_the_trunk_floor(wseed, mode, xseed):
    sd, x, (feat, xrr, planes), exact = draw(wseed, mode, xseed)
    d_default = O.rel_l2(rrdbnet_emulated(sd, x, "bf16").double(), exact)
    d_exact_tail = O.rel_l2(E.rrdbnet_tail_exact(sd, x, "bf16"), exact)
    d_split = O.rel_l2(E.tail_split(sd, feat, xrr, planes).double(), exact)
    print(f"[tail split cpu] ({wseed},{mode},{xseed}): default {d_default:.3e}  tail exact {d_exact_tail:.3e}  f16x2 {d_split:.3e}  "
          f"({d_default / d_split:.1f} x)")
    assert abs(d_split - d_exact_tail) <= 0.05 * d_exact_tail, (d_split, d_exact_tail)
    assert d_split * 10 <= d_default, (d_split, d_default)


@pytest.mark.parametrize("wseed,mode,xseed", DRAWS)
def test_scaled_low_parts_survive_a_subnormal_flush(wseed, mode, xseed):
    sd, x, (feat, xrr, planes), exact = draw(wseed, mode, xseed)
    d_flush = O.rel_l2(E.tail_split(sd, feat, xrr, planes, flush=True).double(), exact)
    d_unscaled = O.rel_l2(E.tail_split(sd, feat, xrr, planes, flush=True, lo_scale=1.0).double(), exact)
    print(f"[tail split cpu] ({wseed},{mode},{xseed}) every fp16-subnormal operand flushed: scaled low parts {d_flush:.3e}, unscaled {d_unscaled:.3e}")
    assert d_flush <= 1.5e-4, d_flush
    assert d_unscaled >= 2 * d_flush       # (what the 2^11 scale buys)
