"""The split-fp16 tail conv (srbh_conv3x3_f16x2, csrc/srbh_ptail_split.hip) layer by layer through the C ABI, against the float64 evaluation
of its contract (tests/tail_split_emulation.py) on the SAME split operands: the planes the kernel reads are read back from the device, so
only the kernel's arithmetic is under test -- the four tail convs (conv_body: + skip; conv_up1 / conv_up2: nearest-x2 read, LeakyReLU;
conv_hr: fp32 and fp16-NHWC ends), full and ragged tiles, one image and a batch with more tiles than CUs (several tiles per workgroup).

Bound.  The contract fixes every rounding but not the order of the additions inside the sums; the distance between the float32 and the float64
accumulation of the emulation on the case itself (`floor`) measures what that freedom is worth, and the kernel -- a third order -- may sit
K = 2 floors from the float64 result (the yardstick and K of tests/test_gpu_trunk_parity.py).  Plane outputs are compared as hi + lo' 2^-11 on
both sides.  One case scales weights and inputs so that UNSCALED low parts would all be fp16 subnormals, with the same bound: the result
does not hang on the matrix cores' subnormal handling.

Measured on an MI355X (all cases): ratio gpu-vs-float64 / floor 0.74 .. 0.81 for the plane and fp32 ends (floor 1.7e-7 .. 2.2e-7; 6.7e-8 in the
small-operand conv_body case), 0.92 .. 1.21 for the fp16-NHWC end (floor 6.6e-6 .. 1.0e-5: rounding flips).  K = 2 holds with a factor 1.65 to
spare.  The fp16 hand-off is bit for bit rne16 of the fp32 output of the same conv."""
import ctypes as C

import pytest
import torch

from oracle import srbh_oracle as O
from srbh_amd import _lib
from tests import gpu_util as G
from tests import tail_split_emulation as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = 2

CONVS = {  # name: (nearest-x2 read, skip, lrelu, end)
    "conv_body": (False, True, False, "planes"),
    "conv_up1": (True, False, True, "planes"),
    "conv_up2": (True, False, True, "planes"),
    "conv_hr": (False, False, False, "final"),
}
# OUTPUT geometries: full 8 x 64 tiles, ragged rows and columns; B = 1 and a batch with more than 256 tiles
GEOS = {"full-1": (1, 16, 128), "ragged-1": (1, 20, 72), "full-batch": (40, 32, 128), "ragged-batch": (48, 28, 88)}


def split_planes(v):
    """(B,64,H,W) fp32 cuda -> 4-plane ACT16 buffer: hi in planes 0..1 (srbh_nhwc32_to_act16), lo' in 2..3 (srbh_act16_split_lo)"""
    L = _lib.lib()
    B, _, H, W = v.shape
    buf = G.act16_alloc(B, 4, H, W, v.device)
    src = v.permute(0, 2, 3, 1).contiguous()
    _lib.check(L.srbh_nhwc32_to_act16(src.data_ptr(), buf.data_ptr(), B, 64, H, W, 4, 0, 1.0, 0, _lib.stream_ptr()), "nhwc32_to_act16")
    _lib.check(L.srbh_act16_split_lo(src.data_ptr(), 0, buf.data_ptr(), 4, 0, buf.data_ptr(), 4, 2, B, H, W, _lib.stream_ptr()), "act16_split_lo")
    torch.cuda.synchronize()
    return buf


def pack_lo(w):
    L = _lib.lib()
    buf = torch.zeros(L.srbh_wpack16_bytes(64, 64), dtype=torch.uint8, device=w.device)
    _lib.check(L.srbh_pack_conv3x3_f16lo(w.contiguous().data_ptr(), 64, 64, buf.data_ptr(), _lib.stream_ptr()), "pack_conv3x3_f16lo")
    return buf


def run_split(inbuf, w, bias, B, H, W, ups, skip, lrelu, end):
    """end: "planes" -> (B,128,H,W) fp16 [hi | lo'] read back, "f32" -> (B,64,H,W) fp32, "h16" -> (B,64,H,W) fp16"""
    wh, wl = G.pack_w(w), pack_lo(w)
    a = G.conv_args(**{"in": inbuf.data_ptr()}, in_chunks_total=4, in_chunk0=0, in_chunks=2, w=wh.data_ptr(), bias=bias.data_ptr(), cout=64,
                    B=B, H=H, W=W, upsample2x=int(ups), lrelu=int(lrelu), skip=None if skip is None else skip.data_ptr())
    s = _lib.ConvSplit(in_lo=inbuf.data_ptr(), in_lo_chunks_total=4, in_lo_chunk0=2, w_lo=wl.data_ptr())
    if end == "planes":
        out = G.act16_alloc(B, 4, H, W, DEV)
        a.out16, a.out16_chunks_total, a.out16_chunk0 = out.data_ptr(), 4, 0
        s.out16_lo, s.out16_lo_chunks_total, s.out16_lo_chunk0 = out.data_ptr(), 4, 2
    elif end == "f32":
        out = torch.full((B, H, W, 64), float("nan"), dtype=torch.float32, device=DEV)
        a.out32, a.out32_c = out.data_ptr(), 64
    else:
        out = torch.full((B, H, W, 64), float("nan"), dtype=torch.float16, device=DEV)
        a.out16, a.out16_chunks_total, a.out16_chunk0, a.out16_nhwc = out.data_ptr(), 2, 0, 1
    _lib.check(_lib.lib().srbh_conv3x3_f16x2(C.byref(a), C.byref(s), _lib.stream_ptr()), "conv3x3_f16x2")
    torch.cuda.synchronize()
    if end == "planes":
        assert G.border_is_zero(out, B, 4, H, W)
        return G.act16_planes(out, B, 4, H, W, torch.float16).cpu()
    return out.permute(0, 3, 1, 2).contiguous().cpu()


def emulate(planes_in, w, bias, ups, skip, lrelu, acc):
    """the contract on the operand planes read back from the device ((n,128,h,w) fp16: hi | lo'), fp32 values in `acc` dtype"""
    hi, lo = planes_in[:, :64].to(acc), planes_in[:, 64:].to(acc)
    if ups:
        hi, lo = O.nearest2x(hi), O.nearest2x(lo)
    y = E.split_conv(w, bias, hi, lo, acc)
    if skip is not None:
        y = E._f32(y + skip.to(acc))
    if lrelu:
        y = torch.where(y >= 0, y, E._f32(y * E._f32(torch.ones((), dtype=acc) * 0.2)))
    return y


def recon(planes):
    return planes[:, :64].double() + planes[:, 64:].double() / 2048


def as_planes(y):
    hi, lo = E.split16(y)
    return torch.cat([hi, lo], 1)


def case(name, geo, wscale=0.05, xscale=1.0, seed=0):
    ups, has_skip, lrelu, end = CONVS[name]
    B, H, W = GEOS[geo]
    g = torch.Generator().manual_seed(1000 + seed)
    ih, iw = (H // 2, W // 2) if ups else (H, W)
    v = (torch.randn(B, 64, ih, iw, generator=g) * xscale).to(DEV)
    w = (torch.randn(64, 64, 3, 3, generator=g) * wscale).to(DEV)
    bias = (torch.randn(64, generator=g) * wscale * xscale).to(DEV)
    skip = (torch.randn(B, H, W, 64, generator=g) * xscale).to(DEV) if has_skip else None
    inbuf = split_planes(v)
    planes_in = G.act16_planes(inbuf, B, 4, ih, iw, torch.float16).cpu()
    idx = sorted({0, B // 2, B - 1})
    sk = None if skip is None else skip.permute(0, 3, 1, 2).cpu()[idx]
    e64 = emulate(planes_in[idx], w.cpu(), bias.cpu(), ups, sk, lrelu, torch.float64)
    e32 = emulate(planes_in[idx], w.cpu(), bias.cpu(), ups, sk, lrelu, torch.float32)
    return (B, H, W, ups, lrelu, end), (inbuf, w, bias, skip), idx, e64, e32


def judge(tag, got, want64, want32):
    floor = O.rel_l2(want32.double(), want64.double())
    d = O.rel_l2(got.double(), want64.double())
    print(f"[tail split] {tag}: floor {floor:.3e}  gpu-vs-float64 {d:.3e}  ratio {d / floor:.2f}")
    assert floor > 0 and d <= K * floor, (d, floor)


@pytest.mark.parametrize("geo", list(GEOS))
@pytest.mark.parametrize("name", list(CONVS))
def test_conv_against_the_contract(name, geo):
    (B, H, W, ups, lrelu, end), (inbuf, w, bias, skip), idx, e64, e32 = case(name, geo)
    if end == "planes":
        got = run_split(inbuf, w, bias, B, H, W, ups, skip, lrelu, "planes")[idx]
        judge(f"{name} {geo} planes", recon(got), recon(as_planes(e64)), recon(as_planes(e32)))
        return
    y32 = run_split(inbuf, w, bias, B, H, W, ups, skip, lrelu, "f32")
    y16 = run_split(inbuf, w, bias, B, H, W, ups, skip, lrelu, "h16")
    assert torch.equal(y16, y32.half()), "the fp16 hand-off is not rne16 of the fp32 output"
    judge(f"{name} {geo} fp32", y32[idx], e64, e32)
    judge(f"{name} {geo} fp16-NHWC", y16[idx].float(), E.rne16(e64), E.rne16(e32))


@pytest.mark.parametrize("name", ["conv_body", "conv_up2", "conv_hr"])
def test_operands_whose_unscaled_low_parts_would_be_subnormal(name):
    """weights ~ 0.01, inputs ~ 0.02: every unscaled low part is below 2^-14 (|v| 2^-11 < 6.1e-5 for |v| < 0.125), the scaled ones are normal"""
    (B, H, W, ups, lrelu, end), (inbuf, w, bias, skip), idx, e64, e32 = case(name, "ragged-1", wscale=0.01, xscale=0.02, seed=7)
    ih, iw = (H // 2, W // 2) if ups else (H, W)
    planes_in = G.act16_planes(inbuf, B, 4, ih, iw, torch.float16).cpu()
    lo_unscaled = planes_in[:, 64:].float().abs() / 2048
    assert float(lo_unscaled.max()) < E.F16_MIN_NORMAL and float(w.abs().max()) < 0.125
    lo_scaled = planes_in[:, 64:].float().abs()
    # (a precondition on the inputs, not on the kernel: a scaled lo' is subnormal only where the residual v - hi is below 2^-25 -- residuals are
    #  uniform within half an ulp of hi, 2^-17 at |v| ~ 0.02, so a few per cent)
    assert float((lo_scaled[lo_scaled > 0] >= E.F16_MIN_NORMAL).float().mean()) >= 0.95
    if end == "planes":
        got = run_split(inbuf, w, bias, B, H, W, ups, skip, lrelu, "planes")[idx]
        judge(f"{name} subnormal-range planes", recon(got), recon(as_planes(e64)), recon(as_planes(e32)))
    else:
        judge(f"{name} subnormal-range fp32", run_split(inbuf, w, bias, B, H, W, ups, skip, lrelu, "f32")[idx], e64, e32)


def test_split_lo_kernel_and_lo_pack_are_the_contract():
    g = torch.Generator().manual_seed(3)
    v = torch.randn(2, 64, 12, 40, generator=g) * torch.exp2(torch.randint(-12, 6, (2, 64, 12, 40), generator=g).float())
    planes = G.act16_planes(split_planes(v.to(DEV)), 2, 4, 12, 40, torch.float16).cpu()
    hi, lo = E.split16(v)
    assert torch.equal(planes[:, :64].float(), hi) and torch.equal(planes[:, 64:].float(), lo)
    w = torch.randn(64, 64, 3, 3, generator=g) * 0.05
    _, w_lo = E.split16(w)
    raw = pack_lo(w.to(DEV)).view(torch.float16).cpu().float()      # WPACK16: [chunk][tap][ks][mb][lane][8]
    raw = raw.view(2, 9, 2, 2, 64, 8)
    for chunk, tap, ks, mb, lane, j in [(0, 0, 0, 0, 0, 0), (1, 4, 1, 1, 37, 5), (0, 8, 1, 0, 63, 7)]:
        oc, ic = mb * 32 + (lane & 31), chunk * 32 + ks * 16 + (lane >> 5) * 8 + j
        assert raw[chunk, tap, ks, mb, lane, j] == w_lo[oc, ic, tap // 3, tap % 3]


# (B, output H, W, nearest-x2 read + LeakyReLU, workgroup cap): a ragged single image with the plain and the nearest-x2 read; 12 full tiles walked
# by two workgroups, six each, so the resident weights and the next-tile prefetch of both kernels run
SHARED_PASS = {"ragged-1": (1, 20, 72, False, 0), "ragged-1-ups": (1, 20, 72, True, 0), "walk-6": (3, 16, 128, False, 2)}


@pytest.mark.parametrize("geo", list(SHARED_PASS))
def test_zero_low_parts_give_the_fp16_kernels_bits(geo):
    """lo' planes and the w_lo pack all zero, no skip: passes 0 and 1 leave every accumulator at +0, the 2^-11 rescale keeps it there and pass 2
    is the fp16 kernel's own accumulation (the same 288-MFMA pass in the same order) -- so srbh_conv3x3_f16x2 equals srbh_conv3x3_f16
    on the same hi planes, w_hi pack and bias bit for bit: the fp16 NHWC hand-off (which sends srbh_conv3x3_f16 to ptail_kernel at any size), the
    ACT16 hi planes and the fp32 NHWC output (against whichever form srbh_conv3x3_f16 selects; tests/test_gpu_conv.py ties the forms together)."""
    B, H, W, ups, cap = SHARED_PASS[geo]
    L = _lib.lib()
    g = torch.Generator().manual_seed(77)
    ih, iw = (H // 2, W // 2) if ups else (H, W)
    v = torch.randn(B, ih, iw, 64, generator=g).to(DEV)
    w = (torch.randn(64, 64, 3, 3, generator=g) * 0.05).to(DEV)
    bias = (torch.randn(64, generator=g) * 0.05).to(DEV)
    inbuf = G.act16_alloc(B, 4, ih, iw, DEV)                       # hi in planes 0..1; planes 2..3 (lo') stay zero
    _lib.check(L.srbh_nhwc32_to_act16(v.data_ptr(), inbuf.data_ptr(), B, 64, ih, iw, 4, 0, 1.0, 0, _lib.stream_ptr()), "nhwc32_to_act16")
    wh = G.pack_w(w)
    wl = torch.zeros_like(wh)

    def args(**out):
        return G.conv_args(**{"in": inbuf.data_ptr()}, in_chunks_total=4, in_chunk0=0, in_chunks=2, w=wh.data_ptr(), bias=bias.data_ptr(), cout=64,
                           B=B, H=H, W=W, upsample2x=int(ups), lrelu=int(ups), **out)

    def run(split):
        p16 = G.act16_alloc(B, 4 if split else 2, H, W, DEV)
        o32 = torch.full((B, H, W, 64), float("nan"), dtype=torch.float32, device=DEV)
        n16 = torch.full((B, H, W, 64), float("nan"), dtype=torch.float16, device=DEV)
        for a in (args(out16=p16.data_ptr(), out16_chunks_total=4 if split else 2, out16_chunk0=0, out32=o32.data_ptr(), out32_c=64),
                  args(out16=n16.data_ptr(), out16_chunks_total=2, out16_chunk0=0, out16_nhwc=1)):
            if split:
                s = _lib.ConvSplit(in_lo=inbuf.data_ptr(), in_lo_chunks_total=4, in_lo_chunk0=2, w_lo=wl.data_ptr(),
                                   out16_lo=p16.data_ptr(), out16_lo_chunks_total=4, out16_lo_chunk0=2)
                _lib.check(L.srbh_conv3x3_f16x2(C.byref(a), C.byref(s), _lib.stream_ptr()), "conv3x3_f16x2")
            else:
                G.run_conv(a)
        torch.cuda.synchronize()
        assert not bool(torch.isnan(o32).any() or torch.isnan(n16).any()) and G.border_is_zero(p16, B, 4 if split else 2, H, W)
        hi = G.act16_planes(p16, B, 4 if split else 2, H, W, torch.int16)[:, :64]
        return n16.view(torch.int16), hi, o32.view(torch.int32)

    prev = L.srbh_ptail_wgs_cap(cap)
    try:
        got, want = run(True), run(False)
    finally:
        L.srbh_ptail_wgs_cap(prev)
    for what, a, b in zip(("fp16 NHWC hand-off", "ACT16 hi planes", "fp32 NHWC"), got, want):
        assert bool(b.any()), what
        assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} elements differ"
