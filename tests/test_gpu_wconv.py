"""srbh_wconv3x3, the wide form of the trunk-family 3x3 conv (64..512 channels, one launch per conv, workgroup = (8 x 64 tile, 64-channel output
slice)), ONE LAYER AT A TIME through the C ABI, fp16 and bf16 operands:

* the fp32 output against a float64 conv (gpu_util.ref_conv64) of the SAME rounded operands, <= 5e-6 (the TIGHT of tests/test_gpu_conv_b16.py:
  products of two 16-bit numbers are exact in fp32, only the order of the additions is left);
* the 16-bit planes BIT FOR BIT equal to torch's RNE conversion of the fp32 output of the same call; borders still zero;
* every epilogue: ReLU on the stored values, the ReLU mask from a saved fp16 plane (against where(saved > 0, g, 0)), addend planes, mask and
  addend together (addend behind the mask), and the gradient form 64 -> 32 with an fp32 NHWC output of 3 channels (nothing written outside it)."""
import pytest
import torch

from oracle import srbh_oracle as O
from srbh_amd import _lib
from tests import gpu_util as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TIGHT = 5e-6
PLANE_T = {0: torch.float16, 1: torch.bfloat16}

SHAPES = [
    (32, 64, 1, 8, 64),        # one chunk in, one slice out, one full tile
    (64, 128, 2, 24, 20),      # ragged tile, two slices, two images
    (256, 512, 1, 6, 5),       # 8 input chunks, 8 slices
    (512, 512, 1, 3, 2),       # 16 input chunks, 8 output slices, a plane smaller than every fragment
    (128, 64, 1, 8, 200),      # several tiles along x, ragged last one
]


def rnd(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def rt(t, bf):
    return G.b16(t) if bf else G.h16(t)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16).cpu(), b.contiguous().view(torch.int16).cpu())


def pack(w, bf):
    return G.pack_w_b16(w.to(DEV)) if bf else G.pack_w(w.to(DEV))


def wconv(xin, cin, wp, bias, cout, B, H, W, bf, **kw):
    import ctypes as C
    a = _lib.WConvArgs()
    a.in_, a.in_chunks_total, a.in_chunk0, a.in_chunks = xin.data_ptr(), cin // 32, 0, cin // 32
    a.w, a.bias, a.cout = wp.data_ptr(), (None if bias is None else bias.data_ptr()), cout
    a.B, a.H, a.W, a.bf16 = B, H, W, bf
    for k, v in kw.items():
        setattr(a, k, v)
    _lib.check(_lib.lib().srbh_wconv3x3(C.byref(a), _lib.stream_ptr()), "wconv3x3")
    torch.cuda.synchronize()


def run_case(cin, cout, B, H, W, bf, relu=0, mask=False, add=False, seed=0):
    x, w, b = rnd((B, cin, H, W), seed + 1), rnd((cout, cin, 3, 3), seed + 2, -0.1, 0.1), rnd((cout,), seed + 3)
    xin = G.act16_from_nchw_x16(x.to(DEV), bf16=bf)
    wp, bd = pack(w, bf), b.to(DEV)
    nmb = cout // 32
    o16 = G.act16_alloc(B, nmb, H, W, DEV)
    o32 = torch.full((B, H, W, cout), 7.0, device=DEV)
    kw = dict(relu=relu, out16=o16.data_ptr(), out16_chunks_total=nmb, out16_chunk0=0, out32=o32.data_ptr(), out32_c=cout)
    want = G.ref_conv64(rt(x, bf), rt(w, bf), b)
    if mask:
        s = rnd((B, cout, H, W), seed + 4)
        sp = G.act16_from_nchw_x16(s.to(DEV), bf16=0)                 # the saved forward plane is fp16 in both operand forms
        kw.update(mask16=sp.data_ptr(), mask_chunks_total=nmb, mask_chunk0=0)
        want = torch.where(G.h16(s) > 0, want, torch.zeros_like(want))
    if add:
        ad = rnd((B, cout, H, W), seed + 5)
        ap = G.act16_from_nchw_x16(ad.to(DEV), bf16=bf)               # addend planes have the output's 16-bit format
        kw.update(add16=ap.data_ptr(), add_chunks_total=nmb, add_chunk0=0)
        want = want + rt(ad, bf).double()
    if relu:
        want = want.clamp_min(0)
    wconv(xin, cin, wp, bd, cout, B, H, W, bf, **kw)
    got32 = o32.permute(0, 3, 1, 2)
    e = O.rel_l2(got32.cpu(), want)
    print(f"wconv {cin}->{cout} {B}x{H}x{W} bf16={bf} relu={relu} mask={mask} add={add}: fp32 output vs float64 conv of the rounded operands {e:.2e}")
    assert e <= TIGHT
    assert same_bits(G.act16_planes(o16, B, nmb, H, W, PLANE_T[bf]), got32.to(PLANE_T[bf]))
    assert G.border_is_zero(o16, B, nmb, H, W)
    if relu:
        assert float(got32.min()) >= 0.0
    if mask:
        assert torch.equal((got32.cpu() == 0) | (G.h16(s) > 0) | add, torch.ones_like(s, dtype=torch.bool))


@pytest.mark.parametrize("bf", [0, 1])
@pytest.mark.parametrize("cin,cout,B,H,W", SHAPES)
def test_wconv_plain(cin, cout, B, H, W, bf):
    run_case(cin, cout, B, H, W, bf)


@pytest.mark.parametrize("bf", [0, 1])
@pytest.mark.parametrize("relu,mask,add", [(1, False, False), (0, True, False), (0, False, True), (0, True, True)])
@pytest.mark.parametrize("cin,cout,B,H,W", [SHAPES[1], SHAPES[3]])
def test_wconv_epilogues(cin, cout, B, H, W, relu, mask, add, bf):
    run_case(cin, cout, B, H, W, bf, relu=relu, mask=mask, add=add, seed=20)


@pytest.mark.parametrize("bf", [0, 1])
def test_wconv_gradient_form_with_fp32_output(bf):
    """64 -> 32 with out32_c = 3 (the last data-gradient conv of the VGG stack: 64 -> 3 channels, the weight's 3 output channels padded to 32 by
    the pack): fp32 NHWC (B, H, W, 3) only, 10 x 70 so that both tile edges are ragged and x has two tiles; NaN guards around the output"""
    B, H, W, cin = 2, 10, 70, 64
    x, w = rnd((B, cin, H, W), 31), rnd((3, cin, 3, 3), 32, -0.1, 0.1)
    b32 = torch.zeros(32)
    b32[:3] = rnd((3,), 33)
    xin = G.act16_from_nchw_x16(x.to(DEV), bf16=bf)
    wp = pack(w, bf)
    gb = G.GuardedBuffers()
    o32 = gb.out((B, H, W, 3))
    wconv(xin, cin, wp, b32.to(DEV), 32, B, H, W, bf, out32=o32.data_ptr(), out32_c=3)
    gb.verify()
    want = G.ref_conv64(rt(x, bf), rt(w, bf), b32[:3])
    e = O.rel_l2(o32.permute(0, 3, 1, 2).cpu(), want)
    print(f"wconv 64->32 (3 stored) bf16={bf}: {e:.2e}")
    assert e <= TIGHT
    # the same call with 16-bit planes as well: 32 channels, the 29 padded ones exactly zero
    o16 = G.act16_alloc(B, 1, H, W, DEV)
    o32b = torch.full((B, H, W, 3), 7.0, device=DEV)
    wconv(xin, cin, wp, None, 32, B, H, W, bf, out16=o16.data_ptr(), out16_chunks_total=1, out16_chunk0=0, out32=o32b.data_ptr(), out32_c=3)
    planes = G.act16_planes(o16, B, 1, H, W, PLANE_T[bf])
    assert same_bits(planes[:, :3], o32b.permute(0, 3, 1, 2).to(PLANE_T[bf]))
    assert not bool(planes[:, 3:].float().abs().max() > 0) and G.border_is_zero(o16, B, 1, H, W)


def test_wconv_refuses_what_it_cannot_run():
    xin = G.act16_alloc(1, 2, 8, 8, DEV)
    wp = torch.zeros(_lib.lib().srbh_wpack16_bytes(96, 64), dtype=torch.uint8, device=DEV)
    o16 = G.act16_alloc(1, 3, 8, 8, DEV)
    with pytest.raises(RuntimeError, match="cout must be 32 or a multiple of 64"):
        wconv(xin, 64, wp, None, 96, 1, 8, 8, 0, out16=o16.data_ptr(), out16_chunks_total=3, out16_chunk0=0)
    with pytest.raises(RuntimeError, match="no output requested"):
        wconv(xin, 64, wp, None, 64, 1, 8, 8, 0)
