"""The compile-time epilogue forms of the persistent tail conv kernel (csrc/srbh_ptail.hip): every form gives the bits of the per-tile kernel.

A launch takes the persistent kernel from 512 tiles on, so the shapes are B = 4 with a 128 x 512 output (512 whole 8 x 64 tiles) and its ragged
twin 124 x 500 (also 512 tiles).  Whole tiles with ONE output run that conv's full-tile form; the ragged shape and planes + fp32 together run the
general form -- srbh_ptail_form_counts says which one ran.  Every case runs under srbh_ptail_wgs_cap(48) (47 workgroups of 11 tiles, the last
6: both parities of the double-buffered input areas, walks that cross tile column, tile row and image) and at the default grid (2 tiles per
workgroup or fewer).

Per case: torch.equal with the per-tile kernel (SRBH_PTAIL=0) on every output, rel-L2 <= TIGHT of tests/test_gpu_conv.py against the CPU conv of
the same fp16-rounded operands on image 0, and the form counter.  TIGHT (5e-6) is a bound for fp32 values: a 16-bit output carries the fp16
rounding itself (half an ulp: 2^-11 relative at most, 2.8e-4 rms), so it is (a) bit-identical to the fp32 output of the per-tile kernel rounded
once to fp16, and that fp32 output holds TIGHT; (b) within 3e-4, the bound of test_gpu_conv.py for 16-bit outputs, of the reference rounded to
fp16 (measured on an MI355X: fp32 1.3e-7, 16-bit 7.4e-6 .. 8.1e-6).  The NHWC16 output exists only in the persistent kernel: it is compared with
the per-tile kernel's ACT16 planes, which hold the same values in another layout."""
import pytest
import torch

from oracle import srbh_oracle as O
from srbh_amd import _lib
from tests import gpu_util as G
from tests.test_gpu_conv import TIGHT, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 4
FULL, RAGGED = (128, 512), (124, 500)
OUT16_BOUND = 3e-4      # tests/test_gpu_conv.py: "output itself is stored as fp16"


@pytest.fixture(scope="module")
def operands():
    """per (ups, shape): inputs, packed weights, bias and the CPU reference of image 0 (before LeakyReLU) -- computed once, never modified"""
    cache = {}

    def get(ups, shape, seed=0):
        key = (ups, shape, seed)
        if key not in cache:
            H, W = shape
            hin, win = (H // 2, W // 2) if ups else (H, W)
            x, w, b = rnd((B, 64, hin, win), 31 + seed), rnd((64, 64, 3, 3), 32, -0.1, 0.1), rnd((64,), 33)
            cache[key] = dict(xin=G.act16_from_nchw(x.to(DEV)), wp=G.pack_w(w.to(DEV)), bias=b.to(DEV), ref0=G.ref_conv(x[:1], w, b, ups=bool(ups)))
        return cache[key]
    return get


def run(op, ups, lrelu, shape, outs):
    """one srbh_conv3x3_f16 launch with the outputs named in `outs` ('planes', 'f32', 'nhwc16'); NaN / zero pre-fill; returns {name: tensor}"""
    H, W = shape
    kw, res = {}, {}
    if "planes" in outs:
        res["planes"] = G.act16_alloc(B, 2, H, W, DEV)
        kw.update(out16=res["planes"].data_ptr(), out16_chunks_total=2, out16_chunk0=0)
    if "nhwc16" in outs:
        res["nhwc16"] = torch.full((B, H, W, 64), float("nan"), dtype=torch.float16, device=DEV)
        kw.update(out16=res["nhwc16"].data_ptr(), out16_chunks_total=2, out16_chunk0=0, out16_nhwc=1)
    if "f32" in outs:
        res["f32"] = torch.full((B, H, W, 64), float("nan"), dtype=torch.float32, device=DEV)
        kw.update(out32=res["f32"].data_ptr(), out32_c=64)
    a = G.conv_args(**{"in": op["xin"].data_ptr()}, in_chunks_total=2, in_chunk0=0, in_chunks=2, w=op["wp"].data_ptr(), bias=op["bias"].data_ptr(),
                    cout=64, B=B, H=H, W=W, upsample2x=ups, lrelu=lrelu, **kw)
    G.run_conv(a)
    return res


_PER_TILE = {}


def per_tile(op, ups, lrelu, shape):
    """planes and fp32 of the per-tile kernel (SRBH_PTAIL=0) as raw bits, once per (operands, lrelu); its fp32 output holds TIGHT against the CPU
    reference, which ties every bit-identical output below to that bound"""
    key = (id(op), lrelu)
    if key not in _PER_TILE:
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("SRBH_PTAIL", "0")
            _lib.ptail_form_counts(reset=True)
            r = run(op, ups, lrelu, shape, ("planes", "f32"))
            torch.cuda.synchronize()
            assert not any(_lib.ptail_form_counts().values())
        H, W = shape
        assert G.border_is_zero(r["planes"], B, 2, H, W) and not bool(torch.isnan(r["f32"]).any())
        ref = torch.nn.functional.leaky_relu(op["ref0"], 0.2) if lrelu else op["ref0"]
        assert O.rel_l2(r["f32"][:1].permute(0, 3, 1, 2).cpu(), ref) <= TIGHT
        _PER_TILE[key] = {"planes": G.act16_planes(r["planes"], B, 2, H, W, torch.int16), "f32": r["f32"].view(torch.int32),
                          "f32_as_h16": r["f32"].half().view(torch.int16).permute(0, 3, 1, 2)}
    return _PER_TILE[key]


def check(got, want, op, lrelu, shape):
    """every output of `got` against the per-tile kernel's bits and against the CPU reference on image 0"""
    H, W = shape
    ref = torch.nn.functional.leaky_relu(op["ref0"], 0.2) if lrelu else op["ref0"]
    for name, t in got.items():
        if name == "f32":
            bits, val = t.view(torch.int32), t[:1].permute(0, 3, 1, 2).cpu()
            err, bound = O.rel_l2(val, ref), TIGHT
        else:
            if name == "planes":
                assert G.border_is_zero(t, B, 2, H, W)
                bits = G.act16_planes(t, B, 2, H, W, torch.int16)
                val = G.act16_planes(t, B, 2, H, W, torch.float16)[:1].float().cpu()
            else:
                bits, val = t.view(torch.int16).permute(0, 3, 1, 2), t[:1].permute(0, 3, 1, 2).float().cpu()
            err, bound = O.rel_l2(val, G.h16(ref)), OUT16_BOUND
        w = want["f32" if name == "f32" else "planes"]
        print(f"{name}: rel_l2 {err:.3e} (bound {bound:g}), {int((bits != w).sum())} of {bits.numel()} elements differ from the per-tile kernel")
        assert bool(w.any()), name
        assert torch.equal(bits, w), f"{name}: {int((bits != w).sum())} of {bits.numel()} elements differ from the per-tile kernel"
        if name != "f32":       # a 16-bit output is the fp32 value rounded once
            assert torch.equal(bits, want["f32_as_h16"]), name
        assert err <= bound, (name, err)


def form_name(ups, lrelu, outs, shape):
    if shape != FULL or len(outs) != 1:
        return "general"
    return f"full_ups{ups}_lrelu{lrelu}_{'out32' if outs == ('f32',) else 'out16'}"


def launch_counted(op, ups, lrelu, shape, outs):
    _lib.ptail_form_counts(reset=True)
    got = run(op, ups, lrelu, shape, outs)
    torch.cuda.synchronize()
    counts = _lib.ptail_form_counts(reset=True)
    assert counts == {k: int(k == form_name(ups, lrelu, outs, shape)) for k in _lib.PTAIL_FORMS}, counts
    return got


CASES = [(u, l, FULL, o) for u in (0, 1) for l in (0, 1) for o in (("planes",), ("f32",), ("nhwc16",), ("planes", "f32"))]
CASES += [(1, 1, RAGGED, ("planes",)), (0, 0, RAGGED, ("f32",))]      # conv_up* and conv_hr argument sets on ragged edges


@pytest.mark.parametrize("cap", [48, 0])
@pytest.mark.parametrize("ups,lrelu,shape,outs", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_every_form_gives_the_bits_of_the_per_tile_kernel(ups, lrelu, shape, outs, cap, operands):
    op = operands(ups, shape)
    want = per_tile(op, ups, lrelu, shape)
    L = _lib.lib()
    prev = L.srbh_ptail_wgs_cap(cap)
    try:
        got = launch_counted(op, ups, lrelu, shape, outs)
    finally:
        L.srbh_ptail_wgs_cap(prev)
    check(got, want, op, lrelu, shape)


@pytest.mark.parametrize("ups,lrelu,outs", [(1, 1, ("planes",)), (0, 0, ("f32",))])
def test_second_launch_on_the_same_stream_is_clean(ups, lrelu, outs, operands):
    """two walks back to back on one stream with different inputs: a store or an input request left in flight by the first would show in the
    second result"""
    first, second = operands(ups, FULL), operands(ups, FULL, seed=100)
    want = per_tile(second, ups, lrelu, FULL)
    L = _lib.lib()
    prev = L.srbh_ptail_wgs_cap(48)
    try:
        run(first, ups, lrelu, FULL, outs)
        got = run(second, ups, lrelu, FULL, outs)
        torch.cuda.synchronize()
    finally:
        L.srbh_ptail_wgs_cap(prev)
    check(got, want, second, lrelu, FULL)


@pytest.mark.parametrize("batch", [1, 4])
def test_whole_forward_feature_is_bit_identical(batch, monkeypatch):
    """forward_feature through RRDBNet (3 blocks, 64 x 64): SRBH_PTAIL=1 against SRBH_PTAIL=0, fp32 and out_dtype=float16.  The dense fp16
    hand-off exists only in the persistent kernel, so its twin is the per-tile fp32 result rounded once to fp16 -- what that output is defined
    as.  At batch 1 only the fp16 conv_hr is a persistent launch (128 tiles); batch 4 brings conv_up2 and the fp32 conv_hr to 512 tiles."""
    from srbh_amd import synth
    from srbh_amd.rrdbnet import RRDBNet
    sd = synth.rrdbnet_state_dict(num_block=3, seed=11, mode="stress")
    net = RRDBNet(3, 3, num_block=3)
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV).eval()
    x = synth.tiles(batch, 8, 64, seed=11)[:, :3].contiguous().to(DEV)

    def fwd(mode, dtype):
        monkeypatch.setenv("SRBH_PTAIL", mode)
        _lib.ptail_form_counts(reset=True)
        with torch.no_grad():
            y = net.forward_feature(x, out_dtype=dtype).clone()
        torch.cuda.synchronize()
        net.check_status()
        return y, _lib.ptail_form_counts(reset=True)

    base, c0 = fwd("0", torch.float32)
    assert not any(c0.values()), c0
    y32, c32 = fwd("1", torch.float32)
    y16, c16 = fwd("1", torch.float16)
    up2, hr = int(batch == 4), int(batch == 4)
    assert c32 == {k: {"full_ups1_lrelu1_out16": up2, "full_ups0_lrelu0_out32": hr}.get(k, 0) for k in _lib.PTAIL_FORMS}, c32
    assert c16 == {k: {"full_ups1_lrelu1_out16": up2, "full_ups0_lrelu0_out16": 1}.get(k, 0) for k in _lib.PTAIL_FORMS}, c16
    assert y32.shape == (batch, 64, 256, 256) and bool(base.any())
    assert torch.equal(y32, base), f"fp32: {int((y32 != base).sum())} elements differ"
    assert y16.dtype == torch.float16 and torch.equal(y16, base.half()), f"fp16: {int((y16 != base.half()).sum())} elements differ"
