"""The persistent trunk kernel's two RDB forms (csrc/srbh_ptrunk3_kernel.h, `rdb_body`: the loop form of every RDB but the last -- halo
rows only, the trunk's operand format, weight prefetch and seam as compile-time properties -- and the peeled last-RDB form behind the
loop: no seam, whole output planes, fp16 in the bf16 form) and its TRAIN template parameter, against the per-layer launch sequence
(SRBH_PERSISTENT=0, read per call), bit for bit.
  * num_block 1: the peeled RDB is the third of three, i.e. at once the FIRST RRDB closing (`r2_pixel`: the RRDB-level stream still in
    conv_first's pixel order) and the last RDB; the loop runs twice.  num_block 2: the first closing is inside the loop, which runs five times.
  * H 8 / 16 / 24 at W 64, B 2: one, two, three tiles per image (no neighbour, one, both), an image boundary between tiles.
  * both operand formats (SRBH_TRUNK_BF16), and the three things that follow the trunk: fp32 features, the fp16 hand-off, the full forward.
The SR-stage training path (TRAIN = 1: forward, and BW = 1: backward) runs at num_block 1 on 16 x 64 tiles as tests/test_sr_stage.py runs
it at 64 x 64: forward and saved planes bit-identical to the per-layer sequence; the backward's per-layer sequence applies 0.2 to the
stream where the launch applies it to conv5's sum, which moves a bf16 rounding here and there, so input and parameter gradients are held
to that file's bound (2e-3 rel-L2, measured there ~1e-4)."""
import numpy as np
import pytest
import torch

from oracle import srbh_oracle as O
from oracle import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, W = 2, 64


@pytest.fixture(scope="module", params=[1, 2])
def net(request):
    from srbh_amd.rrdbnet import RRDBNet
    nb = request.param
    n = RRDBNet(3, 3, num_block=nb)
    n.load_state_dict(synth.rrdbnet_state_dict(num_block=nb, seed=41 + nb, mode="stress"), strict=True)
    return n.to(DEV).eval()


def tiles(H):
    return synth.tiles(B, 3, W, seed=52 + H)[:, :, :H, :].contiguous().to(DEV)


def run(net, x, want_forward):
    if want_forward == 1:
        return net.forward(x)
    return net.forward_feature(x, out_dtype=torch.float16 if want_forward == 2 else None)


def persistent(net, x, want_forward, monkeypatch):
    from srbh_amd import _lib
    monkeypatch.setenv("SRBH_PERSISTENT", "1")
    y = run(net, x, want_forward)
    assert _lib.lib().srbh_trunk_kernel_name() == b"ptrunk3_kernel"     # (the kernel under test, not a fall-back form)
    return y


@pytest.mark.parametrize("want_forward", [0, 2, 1])
@pytest.mark.parametrize("bf16", ["0", "1"])
@pytest.mark.parametrize("H", [8, 16, 24])
def test_both_rdb_forms_equal_the_per_layer_sequence(net, H, bf16, want_forward, monkeypatch):
    monkeypatch.setenv("SRBH_TRUNK_BF16", bf16)
    x = tiles(H)
    with torch.no_grad():
        y1 = persistent(net, x, want_forward, monkeypatch)
        net.check_status()
        monkeypatch.setenv("SRBH_PERSISTENT", "0")
        y0 = run(net, x, want_forward)
        net.check_status()
    assert y1.shape == (B, 3 if want_forward == 1 else 64, 4 * H, 4 * W) and y1.dtype == (torch.float16 if want_forward == 2 else torch.float32)
    assert bool(torch.isfinite(y1).all()) and float(y1.abs().max()) > 0
    assert torch.equal(y0, y1), (H, bf16, want_forward)


@pytest.mark.parametrize("bf16", ["0", "1"])
def test_two_forwards_back_to_back_repeat_themselves(net, bf16, monkeypatch):
    """no synchronisation in between: the second launch starts on the LDS stages, progress counters and dense buffers the peeled last
    RDB of the first left behind (it publishes, but nobody waits; it prefetches weights nobody reads)"""
    monkeypatch.setenv("SRBH_TRUNK_BF16", bf16)
    x = tiles(24)
    with torch.no_grad():
        ya = persistent(net, x, 0, monkeypatch).clone()
        yb = persistent(net, x, 0, monkeypatch)
        net.check_status()
        monkeypatch.setenv("SRBH_PERSISTENT", "0")
        y0 = net.forward_feature(x)
        net.check_status()
    assert torch.equal(ya, yb) and torch.equal(y0, yb), bf16


def test_training_forms_equal_the_per_layer_path():
    from srbh_amd import rrdbnet_autograd as RA
    from srbh_amd.rrdbnet import RRDBNet
    blocks, Hh = 1, 16
    net = RRDBNet(3, 3, num_block=blocks)
    net.load_state_dict(synth.rrdbnet_state_dict(num_block=blocks, seed=5, mode="stress"))
    net = net.to(DEV)

    def rand(shape, seed):
        return torch.from_numpy(np.random.default_rng(seed).uniform(-1.0, 1.0, size=shape).astype(np.float32))

    feat = rand((B, Hh, W, 64), 31).to(DEV).contiguous()          # (B, H, W, 64) fp32 NHWC
    g = rand((B, Hh, W, 64), 32).to(DEV).contiguous()
    old = RA.BWD_PERSISTENT
    fwd, bwd = [], []
    try:
        for pers in (True, False):      # the forward: one launch (TRAIN = 1) against the per-layer sequence
            RA.BWD_PERSISTENT = True
            RA._FAST_WS.clear()
            n0 = dict(RA.TRUNK_FWD_PATHS)
            ws = RA._fast_buffers(B, Hh, W, blocks * 3, feat.device)
            assert ws["aux"] is not None, "this geometry must take the persistent kernel"
            if not pers:
                ws["aux"] = None
            xr, lease = RA._trunk_fast_forward(net, feat)
            torch.cuda.synchronize()
            key = "persistent" if pers else "per_layer"
            assert RA.TRUNK_FWD_PATHS[key] == n0[key] + 1
            fwd.append((xr.clone(), lease.ws["D"].clone()))
            lease.release()
        for pers in (True, False):      # the backward (BW = 1) behind a persistent forward, on the same saved planes
            RA.BWD_PERSISTENT = True
            RA._FAST_WS.clear()
            xr, lease = RA._trunk_fast_forward(net, feat)
            RA.BWD_PERSISTENT = pers
            n0 = dict(RA.TRUNK_BWD_PATHS)
            grads = {}
            gin = RA._trunk_fast_backward(net, lease, g.clone(), grads)
            torch.cuda.synchronize()
            key = "persistent" if pers else "per_layer"
            assert RA.TRUNK_BWD_PATHS[key] == n0[key] + 1
            lease.release()
            bwd.append((gin.clone(), {n_: grads[id(p)].clone() for n_, p in net.named_parameters() if id(p) in grads}))
    finally:
        RA.BWD_PERSISTENT = old
        RA._FAST_WS.clear()
    assert bool(torch.isfinite(fwd[0][0]).all()) and float(fwd[0][0].abs().max()) > 0
    assert torch.equal(fwd[0][0], fwd[1][0])
    assert torch.equal(fwd[0][1], fwd[1][1])
    (g0, w0), (g1, w1) = bwd
    assert bool(torch.isfinite(g0).all()) and len(w0) == blocks * 3 * 10 and w0.keys() == w1.keys()
    e_in = O.rel_l2(g0.cpu(), g1.cpu())
    worst = max(O.rel_l2(w0[k].cpu(), w1[k].cpu()) for k in w0)
    print(f"input gradient rel-L2 {e_in:.3e}, worst parameter gradient rel-L2 {worst:.3e}")
    assert e_in <= 2e-3 and worst <= 2e-3, (e_in, worst)
