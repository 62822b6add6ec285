"""The inference trunk on bf16 operands (srbh_rrdbnet_desc.rdb_b16, SRBH_TRUNK_BF16): the persistent kernel's bf16 form against the
per-layer bf16 sequence bit for bit, its distance from the fp16 trunk, and the A/B switch restoring the fp16 trunk exactly."""
import ctypes as C

import pytest
import torch

from oracle import srbh_oracle as O
from oracle import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def build(sd, **kw):
    from srbh_amd.rrdbnet import RRDBNet
    net = RRDBNet(3, 3, **kw)
    net.load_state_dict(sd, strict=True)
    return net.to(DEV).eval()


def test_bf16_persistent_and_per_layer_paths_agree(monkeypatch):
    """the shapes of test_persistent_and_per_layer_paths_agree, with the bf16 trunk selected explicitly"""
    monkeypatch.setenv("SRBH_TRUNK_BF16", "1")
    sd = synth.rrdbnet_state_dict(num_block=3, seed=21, mode="stress")
    net = build(sd, num_block=3)
    for B, hw in ((3, 64), (40, 64), (2, 40)):
        x = synth.tiles(B, 3, hw, seed=22).to(DEV)
        with torch.no_grad():
            monkeypatch.setenv("SRBH_PERSISTENT", "1")
            y1 = net.forward_feature(x)
            net.check_status()
            monkeypatch.setenv("SRBH_PERSISTENT", "0")
            y0 = net.forward_feature(x)
        assert torch.equal(y0, y1), (B, hw)


def test_bf16_trunk_stays_close_to_the_fp16_trunk(monkeypatch):
    """the full 23-block network at B=32: bf16 trunk operands move forward_feature by ~5e-4 (rel-L2) from the fp16 trunk, and its distance
    from the fp32 oracle by ~1 % (measured 7.17e-4 against 7.10e-4 on tile 0): the tail convs, not the trunk, set the error"""
    sd = synth.rrdbnet_state_dict(seed=1337, mode="init")
    net = build(sd)
    x = synth.tiles(32, 8, 64, seed=1337)[:, :3].contiguous().to(DEV)
    with torch.no_grad():
        monkeypatch.setenv("SRBH_TRUNK_BF16", "1")
        yb = net.forward_feature(x)
        net.check_status()
        monkeypatch.setenv("SRBH_TRUNK_BF16", "0")
        yh = net.forward_feature(x)
        net.check_status()
    e = O.rel_l2(yb.cpu(), yh.cpu())
    want = O.rrdbnet_forward_feature(sd, x[:1].cpu())
    eb, eh = O.rel_l2(yb[:1].cpu(), want), O.rel_l2(yh[:1].cpu(), want)
    print(f"bf16 vs fp16 trunk rel-L2 {e:.3e}; vs fp32 oracle (tile 0): bf16 {eb:.3e}, fp16 {eh:.3e}")
    assert e <= 7.5e-4
    assert eb <= 1e-3 and eh <= 1e-3
    assert eb <= 1.05 * eh


def test_switch_off_is_the_fp16_trunk(monkeypatch):
    """SRBH_TRUNK_BF16=0 computes what a descriptor without bf16 packs computes (the fp16 trunk), in both launch forms"""
    sd = synth.rrdbnet_state_dict(num_block=3, seed=21, mode="stress")
    net = build(sd, num_block=3)
    x = synth.tiles(3, 3, 64, seed=22).to(DEV)
    with torch.no_grad():
        for persistent in ("1", "0"):
            monkeypatch.setenv("SRBH_PERSISTENT", persistent)
            monkeypatch.setenv("SRBH_TRUNK_BF16", "0")
            y_off = net.forward_feature(x)
            monkeypatch.delenv("SRBH_TRUNK_BF16")
            y_on = net.forward_feature(x)
            desc = net._packed[2]
            ptr_t = type(desc.rdb_b16)
            saved = C.cast(desc.rdb_b16, C.c_void_p).value       # (an address: the field object itself aliases the struct's storage)
            desc.rdb_b16 = ptr_t()
            try:
                y_fp16 = net.forward_feature(x)
            finally:
                desc.rdb_b16 = C.cast(C.c_void_p(saved), ptr_t)
            net.check_status()
            assert torch.equal(y_off, y_fp16), persistent
            assert not torch.equal(y_on, y_fp16), persistent     # (the default is the bf16 trunk)
