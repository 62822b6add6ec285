"""CPU: the rounding-exact emulation of the inference RRDBNet (oracle/rrdbnet_emulation.py) against the plain oracle and against
what the hardware was measured to do."""
import pytest
import torch

from oracle import srbh_oracle as O
from oracle import synth
from oracle.rrdbnet_emulation import rrdbnet_emulated


@pytest.mark.parametrize("scale,hw", [(4, 24), (2, 32), (1, 32)])
def test_without_rounding_it_is_the_oracle(scale, hw):
    """trunk=None rounds nothing: the same network as srbh_oracle.rrdbnet_forward_feature -- in float64 to float64 rounding, and the fp32
    oracle sits at fp32 rounding from it; the trunk output equals the oracle's RRDB chain"""
    sd = synth.rrdbnet_state_dict(num_block=2, scale=scale, seed=12, mode="stress")
    x = synth.tiles(2, 3, hw, seed=13)
    sdd = {k: v.double() for k, v in sd.items()}
    want64 = O.rrdbnet_forward_feature(sdd, x.double(), scale=scale)
    xrr, got = rrdbnet_emulated(sd, x, trunk=None, stop="both", scale=scale)
    assert got.dtype == torch.float64 and got.shape == want64.shape
    assert O.rel_l2(got, want64) <= 1e-14
    assert O.rel_l2(O.rrdbnet_forward_feature(sd, x, scale=scale), got) <= 2e-6          # fp32 vs float64 arithmetic, ~40 convs deep
    xin = x.double() if scale == 4 else O.pixel_unshuffle(x.double(), 4 // scale)
    body = O._conv3(sdd, "conv_first", xin)
    for i in range(2):
        body = O.rrdb(sdd, f"body.{i}.", body)
    assert O.rel_l2(xrr, body) <= 1e-14
    assert torch.equal(rrdbnet_emulated(sd, x, trunk=None, stop="trunk", scale=scale), xrr)
    got32 = rrdbnet_emulated(sd, x, trunk=None, acc=torch.float32, scale=scale)
    assert got32.dtype == torch.float32 and O.rel_l2(got32, want64) <= 2e-6


def test_rounding_points_small():
    """a net without dense blocks has only the tail's roundings, whatever trunk is asked for; with blocks the three settings differ, bf16 the most"""
    sd0 = synth.rrdbnet_state_dict(num_block=0, seed=3, mode="stress")
    x = synth.tiles(1, 3, 16, seed=4)
    assert torch.equal(rrdbnet_emulated(sd0, x, "bf16"), rrdbnet_emulated(sd0, x, "fp16"))
    sd = synth.rrdbnet_state_dict(num_block=1, seed=3, mode="stress")
    exact = rrdbnet_emulated(sd, x, None, stop="trunk")
    eb = O.rel_l2(rrdbnet_emulated(sd, x, "bf16", stop="trunk"), exact)
    eh = O.rel_l2(rrdbnet_emulated(sd, x, "fp16", stop="trunk"), exact)
    assert 0 < eh < eb < 1e-3 and eb > 4 * eh        # (3 more mantissa bits: 8 x in rounding error per element)
    with pytest.raises(ValueError):
        rrdbnet_emulated(sd, x, "fp32")


def test_emulation_reproduces_the_figures_measured_on_the_gpu():
    """the configuration of DESIGN.md section 4 (seed 1337, init weights, tile 0 of the benchmark batch, 23 blocks): the final map's distance from the
    fp32 oracle with either trunk, and of the two trunks from each other, as recorded on an MI355X: 7.168e-4, 7.102e-4 (2 %) and 4.8e-4 (3 %: two
    digits recorded).  A rounding point in the wrong place moves these.  Measured here: 0.03 %, 0.06 %, 0.2 %."""
    sd = synth.rrdbnet_state_dict(seed=1337, mode="init")
    x = synth.tiles(1, 8, 64, seed=1337)[:, :3].contiguous()
    want = O.rrdbnet_forward_feature(sd, x)
    eb, eh = rrdbnet_emulated(sd, x, "bf16"), rrdbnet_emulated(sd, x, "fp16")
    got = O.rel_l2(eb, want), O.rel_l2(eh, want), O.rel_l2(eb, eh)
    print("emulated: bf16 vs oracle %.4e, fp16 vs oracle %.4e, bf16 vs fp16 %.4e" % got)
    for g, rec, tol in zip(got, (7.168e-4, 7.102e-4, 4.8e-4), (0.02, 0.02, 0.03)):
        assert abs(g - rec) <= tol * rec, (g, rec)
