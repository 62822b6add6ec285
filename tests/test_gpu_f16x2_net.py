"""The "f16x2" precision mode (net.precision = "f16x2": bf16 trunk untouched, the four tail convs on split fp16 operands) on the whole
network, and that selecting it moves nothing else.

Parity (23 blocks, one 64x64 tile per draw): forward_feature against the fp32 oracle must come within 2 x the distance an EXACT tail behind the
emulated bf16 trunk leaves on the same draw (tests/tail_split_emulation.py: the trunk's own error, nothing the tail could remove), and never
above 1.5e-4.  The default path sits at 5.6e-4 .. 7.2e-4 on these draws, so on a build that ignores the attribute this test fails.  The same
forward also has to agree with the float64 emulation of the mode as tests/test_gpu_trunk_parity.py asks of the final map: the two distances
from the oracle within 3 % of each other.

Measured on an MI355X, 12 draws: gpu vs oracle 4.87e-5 .. 5.74e-5; gpu / tail exact 1.000 on every draw; gpu vs emulated mode, distances from the
oracle within 0.00 .. 0.02 % (the two maps themselves 1.2e-6 .. 1.4e-6 apart: the trunk's floor).  predict_tiles: 0.061 % of the height pixels
differ from the default mode's mosaic, by 1 LSB."""
import pytest
import torch

from oracle import srbh_oracle as O
from oracle import synth
from oracle.mosaic_oracle import synthetic_city
from oracle.rrdbnet_emulation import rrdbnet_emulated
from srbh_amd import _lib
from tests import tail_split_emulation as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def build(sd, **kw):
    from srbh_amd.rrdbnet import RRDBNet
    net = RRDBNet(3, 3, **kw)
    net.load_state_dict(sd, strict=True)
    return net.to(DEV).eval()


def feature(net, x, precision=None, **kw):
    if precision is None:
        net.__dict__.pop("precision", None)
    else:
        net.precision = precision
    with torch.no_grad():
        y = net.forward_feature(x, **kw)
    torch.cuda.synchronize()
    net.check_status()
    return y


@pytest.mark.parametrize("xseed", [1337, 77])
@pytest.mark.parametrize("mode", ["init", "stress"])
@pytest.mark.parametrize("wseed", [1337, 3, 21])
def test_forward_feature_reaches_the_trunk_floor(wseed, mode, xseed):
    sd = synth.rrdbnet_state_dict(seed=wseed, mode=mode)
    x = synth.tiles(1, 8, 64, seed=xseed)[:, :3].contiguous()
    net = build(sd)
    got = feature(net, x.to(DEV), "f16x2").cpu()
    want = O.rrdbnet_forward_feature(sd, x)
    exact = rrdbnet_emulated(sd, x, None)
    feat, xrr, planes = E.trunk_and_feat(sd, x, "bf16")
    d_exact_tail = O.rel_l2(E.rrdbnet_tail_exact(sd, x, "bf16"), exact)
    emu = E.tail_split(sd, feat, xrr, planes)
    d_gpu, d_emu = O.rel_l2(got, want), O.rel_l2(emu, want)
    print(f"[f16x2 net] ({wseed},{mode},{xseed}): gpu vs oracle {d_gpu:.4e}  emulation vs oracle {d_emu:.4e} ({100 * abs(d_gpu - d_emu) / d_emu:.2f} %)  "
          f"tail exact {d_exact_tail:.4e}  gpu / tail exact {d_gpu / d_exact_tail:.3f}  gpu vs emulation {O.rel_l2(got, emu):.3e}")
    assert d_gpu <= 2 * d_exact_tail, (d_gpu, d_exact_tail)
    assert d_gpu <= 1.5e-4, d_gpu
    assert abs(d_gpu - d_emu) <= 0.03 * d_emu, (d_gpu, d_emu)


@pytest.mark.parametrize("persistent", ["1", "0"])
def test_switching_the_mode_moves_nothing_else(persistent, monkeypatch):
    """default, f16x2, default again on ONE net: first and third equal bit for bit, fp32 and fp16 hand-off; the mode's fp16 hand-off is rne16
    of its fp32 output; the mode does something; also with the environment selector and a caller-owned output"""
    monkeypatch.setenv("SRBH_PERSISTENT", persistent)
    monkeypatch.delenv("SRBH_TRUNK_PRECISION", raising=False)
    sd = synth.rrdbnet_state_dict(num_block=3, seed=21, mode="stress")
    net = build(sd, num_block=3)
    for B, hw in [(3, 64), (2, 40)]:
        x = synth.tiles(B, 3, hw, seed=22).to(DEV)
        a32, a16 = feature(net, x).clone(), feature(net, x, out_dtype=torch.float16).clone()
        s32, s16 = feature(net, x, "f16x2").clone(), feature(net, x, "f16x2", out_dtype=torch.float16).clone()
        b32, b16 = feature(net, x), feature(net, x, out_dtype=torch.float16)
        assert torch.equal(a32, b32) and torch.equal(a16, b16)
        assert torch.equal(feature(net, x, "f16"), a32)
        assert torch.equal(s16, s32.half()) and torch.equal(a16, a32.half())
        assert not torch.equal(s32, a32)
        want = O.rrdbnet_forward_feature(sd, x.cpu())
        assert O.rel_l2(s32.cpu(), want) < 0.5 * O.rel_l2(a32.cpu(), want)
        out = torch.empty_like(s32)
        assert feature(net, x, "f16x2", out=out) is out and torch.equal(out, s32)
        monkeypatch.setenv("SRBH_TRUNK_PRECISION", "f16x2")
        assert torch.equal(feature(net, x), s32)
        monkeypatch.delenv("SRBH_TRUNK_PRECISION")
        assert torch.equal(feature(net, x), a32)
        # the trunk is untouched: its fp32 output stream, read back from either mode's workspace, is the same
        outs = []
        for prec, key in (("f16x2", (B, hw, hw, 0, x.device, "f16x2")), (None, (B, hw, hw, 0, x.device))):
            feature(net, x, prec)
            ws = net._workspaces[key]
            t = torch.empty((B, hw, hw, 64), dtype=torch.float32, device=DEV)
            _lib.check(_lib.lib().srbh_rrdbnet_trunk_out(ws.data_ptr(), ws.numel(), 3, B, hw, hw, 0, t.data_ptr(), _lib.stream_ptr()), "trunk_out")
            torch.cuda.synchronize()
            outs.append(t)
        assert torch.equal(outs[0], outs[1])
    net.precision = "f16x2"
    with pytest.raises(NotImplementedError, match="f16x2"):
        net(synth.tiles(1, 3, 16, seed=1).to(DEV))


def test_weight_update_reaches_the_lo_packs():
    """the lo' packs are rewritten by the same pack launch as everything else"""
    sd = synth.rrdbnet_state_dict(num_block=1, seed=5, mode="stress")
    net = build(sd, num_block=1)
    x = synth.tiles(1, 3, 32, seed=6).to(DEV)
    y0 = feature(net, x, "f16x2").clone()
    with torch.no_grad():
        net.conv_hr.weight.mul_(1.0 + 2.0 ** -14)       # below fp16 resolution: only the lo' pack can see it
    y1 = feature(net, x, "f16x2")
    sd2 = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    assert not torch.equal(y0, y1)
    assert O.rel_l2(y1.cpu(), O.rrdbnet_forward_feature(sd2, x.cpu())) < 1e-4


def test_predict_tiles_runs_in_the_mode():
    """harness.predict_tiles (captured graphs, fp16 hand-off to the head) with a net in the mode, on the window layout of the mosaic fixtures'
    synthetic city: the height mosaic differs from the default mode's by at most 1 LSB; the share of differing pixels is printed"""
    from srbh_amd import harness
    from srbh_amd.mosaic import Mosaic
    from tests.test_gpu_model import make_model
    _, _, pos, lr_w, lr_h = synthetic_city(lr_w=160, lr_h=144, tile=64, n_extra=3)
    pos = [[int(v) for v in p] for p in pos]
    sd = synth.rrdbnet_state_dict(num_block=2, seed=4, mode="stress")
    net_hr = build(sd, num_block=2)
    model = make_model(seed=12, isaggre=False).to(DEV).eval()
    tiles = synth.tiles(len(pos), 8, 64, seed=23, kind="grid").to(DEV)

    def run(precision):
        if precision is None:
            net_hr.__dict__.pop("precision", None)
        else:
            net_hr.precision = precision
        m = Mosaic(4 * lr_h, 4 * lr_w, 7, DEV)
        assert harness.predict_tiles(net_hr, model, tiles, pos, m, batch=4) == len(pos)
        net_hr.check_status()
        return m.finalize()

    (h0, c0), (h1, c1), (h2, c2) = run(None), run("f16x2"), run(None)
    dh = (h0.int() - h1.int()).abs()
    print(f"[f16x2 predict] height pixels differing from the default mode: {100 * float((dh > 0).float().mean()):.3f} % (max {int(dh.max())} LSB); "
          f"classes differing {100 * float((c0 != c1).float().mean()):.3f} %")
    assert int(dh.max()) <= 1
    d02 = (h0.int() - h2.int()).abs()
    assert int(d02.max()) <= 1 and float((d02 > 0).float().mean()) < 1e-3      # (run to run: atomics in the head's pooled reductions)
