"""The persistent trunk kernel's paired order of the dense block's cout-32 layers (P3_PAIR, csrc/srbh_ptrunk3_kernel.h: conv2 leaves x's
second chunk and X1 staged for conv3 and conv4, which share one pass over their common planes) against the per-layer launch sequence,
bit for bit, at the tile counts where the halo exchange differs: one tile per image (both halo rows are borders), two (every tile has
exactly one neighbour), three (a middle tile with two), with an image boundary between tiles.  Two RRDBs are six dense blocks: both
kinds of RRDB closing and the last dense block's fp16 output."""
import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NUM_BLOCK, B, W = 2, 2, 64


@pytest.fixture(scope="module")
def net():
    from srbh_amd.rrdbnet import RRDBNet
    n = RRDBNet(3, 3, num_block=NUM_BLOCK)
    n.load_state_dict(synth.rrdbnet_state_dict(num_block=NUM_BLOCK, seed=31, mode="stress"), strict=True)
    return n.to(DEV).eval()


def tiles(H):
    return synth.tiles(B, 3, W, seed=32 + H)[:, :, :H, :].contiguous().to(DEV)


def persistent(net, x, monkeypatch):
    from srbh_amd import _lib
    monkeypatch.setenv("SRBH_PERSISTENT", "1")
    y = net.forward_feature(x)
    assert _lib.lib().srbh_trunk_kernel_name() == b"ptrunk3_kernel"     # (the kernel under test, not a fall-back form)
    return y


@pytest.mark.parametrize("bf16", ["1", "0"])
@pytest.mark.parametrize("H", [8, 16, 24])
def test_paired_order_equals_the_per_layer_sequence(net, H, bf16, monkeypatch):
    monkeypatch.setenv("SRBH_TRUNK_BF16", bf16)
    x = tiles(H)
    with torch.no_grad():
        y1 = persistent(net, x, monkeypatch)
        net.check_status()
        monkeypatch.setenv("SRBH_PERSISTENT", "0")
        y0 = net.forward_feature(x)
        net.check_status()
    assert y1.shape == (B, 64, 4 * H, 4 * W) and float(y1.abs().max()) > 0
    assert torch.equal(y0, y1), (H, bf16)


@pytest.mark.parametrize("bf16", ["1", "0"])
def test_back_to_back_launches_repeat_themselves(net, bf16, monkeypatch):
    """two launches with no synchronisation in between: a stale LDS stage or progress counter of the first would show in the second"""
    monkeypatch.setenv("SRBH_TRUNK_BF16", bf16)
    x = tiles(24)
    with torch.no_grad():
        ya = persistent(net, x, monkeypatch).clone()
        yb = persistent(net, x, monkeypatch)
        net.check_status()
        monkeypatch.setenv("SRBH_PERSISTENT", "0")
        y0 = net.forward_feature(x)
        net.check_status()
    assert torch.equal(ya, yb) and torch.equal(y0, yb), bf16
