"""The bf16 forms of the fused 3x3 convolution, their packs and their plane conversion, ONE LAYER AT A TIME through the C ABI.

The whole-network tests reach these forms only through chains with tolerances of 1e-3, and the two launch forms of the bf16 trunk are
compared with each other, not with a reference: a wrong weight slice, a truncation instead of round-to-nearest-even or a swapped half of a
pack would be shared by both.  Here every form meets an independent reference:

* srbh_conv3x3_x16(bf16 = 1 | 2): the fp32 result against a float64 conv of the SAME bf16-rounded operands, <= 5e-6 (a product of two
  bf16 numbers has 16 significant bits and is exact in fp32, so as for fp16 only the order of the additions is left); the 16-bit planes
  BIT FOR BIT equal to torch's RNE conversion of the fp32 result of the same call (both come from the same accumulators);
* the rounding itself at its edges (ties to even in both directions, binade carry, overflow to infinity, infinities, NaN, -0.0);
* the packs against torch's RNE conversion in the element order the fp16 pack defines; the plane conversion against torch's product."""
import numpy as np
import pytest
import torch

from oracle import srbh_oracle as O
from srbh_amd import _lib
from tests import gpu_util as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TIGHT = 5e-6
OUT_T = {1: torch.bfloat16, 2: torch.float16}

TRUNK_SHAPES = [(64, 32), (96, 32), (128, 32), (160, 32), (192, 64)]      # (cin, cout) of conv1 .. conv5 of a dense block


def rnd(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def bits(t):
    return t.contiguous().view(torch.int16)


def same_bits(a, b):
    return torch.equal(bits(a.cpu()), bits(b.cpu()))


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("lrelu", [0, 1])
@pytest.mark.parametrize("B,cin,cout,H,W", [
    (2, 64, 32, 64, 64),      # conv1
    (1, 96, 32, 64, 64),      # conv2
    (1, 128, 32, 64, 64),     # conv3
    (1, 160, 32, 16, 64),     # conv4, short image
    (2, 192, 64, 64, 64),     # conv5 shape (plain epilogue)
    (1, 64, 64, 24, 40),      # ragged: H, W not multiples of the 8 x 64 tile
    (3, 32, 32, 7, 5),        # tiny, one chunk
    (1, 64, 64, 8, 200),      # several tiles along x, ragged last one
])
def test_conv_b16_plain(B, cin, cout, H, W, lrelu, form):
    x, w, b = rnd((B, cin, H, W), 1), rnd((cout, cin, 3, 3), 2, -0.1, 0.1), rnd((cout,), 3)
    xin = G.act16_from_nchw_x16(x.to(DEV))
    assert same_bits(G.act16_planes(xin, B, cin // 32, H, W), x.to(torch.bfloat16))      # the operand planes are what the reference rounds
    wp, bd = G.pack_w_b16(w.to(DEV)), b.to(DEV)
    o16 = G.act16_alloc(B, cout // 32, H, W, DEV)
    o32 = torch.full((B, H, W, cout), 7.0, device=DEV)
    a = G.conv_args(**{"in": xin.data_ptr()}, in_chunks_total=cin // 32, in_chunk0=0, in_chunks=cin // 32, w=wp.data_ptr(), bias=bd.data_ptr(),
                    cout=cout, B=B, H=H, W=W, lrelu=lrelu, out16=o16.data_ptr(), out16_chunks_total=cout // 32, out16_chunk0=0,
                    out32=o32.data_ptr(), out32_c=cout)
    G.run_conv_x16(a, form)
    torch.cuda.synchronize()
    want = G.ref_conv64(G.b16(x), G.b16(w), b)
    if lrelu:
        want = torch.where(want >= 0, want, want * float(np.float32(0.2)))
    got32 = o32.permute(0, 3, 1, 2)
    e = O.rel_l2(got32.cpu(), want)
    print(f"conv_b16 form {form} {cin}->{cout} {B}x{H}x{W} lrelu={lrelu}: fp32 result vs float64 conv of the bf16 operands {e:.2e}")
    assert e <= TIGHT
    assert same_bits(G.act16_planes(o16, B, cout // 32, H, W, OUT_T[form]), got32.to(OUT_T[form]))
    assert G.border_is_zero(o16, B, cout // 32, H, W)


@pytest.mark.parametrize("form", [1, 2])
def test_conv_b16_residual_epilogues_and_chunk_offsets(form):
    """conv5's calls: x5 * 0.2 + x into res1 in place; closing an RRDB also (..) * 0.2 + res2, both streams updated; the 16-bit copy into another
    buffer's planes 0..1.  Then a conv3-style call that reads planes 1..2 of a 6-plane buffer and writes plane 4 of the SAME buffer."""
    B, H, W = 2, 16, 64
    x = rnd((B, 192, H, W), 10)
    w, b = rnd((64, 192, 3, 3), 11, -0.05, 0.05), rnd((64,), 12)
    r1, r2 = rnd((B, 64, H, W), 13), rnd((B, 64, H, W), 14)
    S = float(np.float32(0.2))
    xin = G.act16_from_nchw_x16(x.to(DEV))
    wp, bd = G.pack_w_b16(w.to(DEV)), b.to(DEV)
    conv = G.ref_conv64(G.b16(x), G.b16(w), b)
    for closing in (0, 1):
        nxt = G.act16_alloc(B, 6, H, W, DEV)
        res1 = r1.permute(0, 2, 3, 1).contiguous().to(DEV)
        res2 = r2.permute(0, 2, 3, 1).contiguous().to(DEV)
        o32 = torch.zeros((B, H, W, 64), device=DEV)
        kw = dict(res2_scale=0.2, res2=res2.data_ptr(), res2_update=1) if closing else {}
        a = G.conv_args(**{"in": xin.data_ptr()}, in_chunks_total=6, in_chunk0=0, in_chunks=6, w=wp.data_ptr(), bias=bd.data_ptr(), cout=64,
                        B=B, H=H, W=W, res_scale=0.2, res1=res1.data_ptr(), res1_update=1, out16=nxt.data_ptr(), out16_chunks_total=6,
                        out16_chunk0=0, out32=o32.data_ptr(), out32_c=64, **kw)
        G.run_conv_x16(a, form)
        torch.cuda.synchronize()
        want = conv * S + r1.double()
        if closing:
            want = want * S + r2.double()
        got = o32.permute(0, 3, 1, 2)
        e = O.rel_l2(got.cpu(), want)
        print(f"conv5 form {form} closing={closing}: {e:.2e}")
        assert e <= TIGHT
        assert torch.equal(res1, o32)                                   # the stream holds the very values the planes were rounded from
        assert torch.equal(res2, o32) if closing else torch.equal(res2.cpu(), r2.permute(0, 2, 3, 1))
        planes = G.act16_planes(nxt, B, 6, H, W, OUT_T[form])
        assert same_bits(planes[:, :64], got.to(OUT_T[form]))
        assert not bits(planes[:, 64:].cpu()).any() and G.border_is_zero(nxt, B, 6, H, W)
    # in_chunk0 / out16_chunk0 inside one buffer
    w3, b3 = rnd((32, 64, 3, 3), 15, -0.1, 0.1), rnd((32,), 16)
    before = G.act16_planes(xin, B, 6, H, W).cpu().clone()
    o32 = torch.zeros((B, H, W, 32), device=DEV)
    a = G.conv_args(**{"in": xin.data_ptr()}, in_chunks_total=6, in_chunk0=1, in_chunks=2, w=G.pack_w_b16(w3.to(DEV)).data_ptr(),
                    bias=b3.to(DEV).data_ptr(), cout=32, B=B, H=H, W=W, lrelu=1, out16=xin.data_ptr(), out16_chunks_total=6, out16_chunk0=4,
                    out32=o32.data_ptr(), out32_c=32)
    G.run_conv_x16(a, 1)
    torch.cuda.synchronize()
    want = G.ref_conv64(G.b16(x[:, 32:96]), G.b16(w3), b3)
    want = torch.where(want >= 0, want, want * S)
    got = o32.permute(0, 3, 1, 2)
    assert O.rel_l2(got.cpu(), want) <= TIGHT
    after = G.act16_planes(xin, B, 6, H, W).cpu()
    assert same_bits(after[:, 128:160], got.to(torch.bfloat16))
    keep = [c for c in range(192) if not 128 <= c < 160]
    assert same_bits(after[:, keep], before[:, keep]) and G.border_is_zero(xin, B, 6, H, W)


def _edge_cases(form):
    """(x, bias, expected 16-bit pattern or None): the accumulator is x (exact in bf16, through the identity filter) + bias, exact in fp32"""
    inf, nan = float("inf"), float("nan")
    if form == 1:       # bf16: 8 significant bits, one ulp at 1.0 = 2^-7
        u = 2.0 ** -7
        return [(1.0, u / 2, 0x3F80), (1.0, u + u / 2, 0x3F82), (-1.0, -u / 2, 0xBF80), (-1.0, -(u + u / 2), 0xBF82),      # ties -> even: down, up
                (1.0, u / 2 + 2.0 ** -23, 0x3F81), (1.0, u / 2 - 2.0 ** -23, 0x3F80), (1.0, u + u / 2 - 2.0 ** -23, 0x3F81),   # next to a tie
                (1.0, 1.0 - 2.0 ** -9, 0x4000), (-1.0, -(1.0 - 2.0 ** -9), 0xC000),     # 2 - 2^-9: the carry runs into the next binade
                (0.0, 3.4028234663852886e38, 0x7F80), (0.0, -3.4028234663852886e38, 0xFF80),       # FLT_MAX rounds to infinity
                (0.0, 3.3895313892515355e38, 0x7F7F),                                  # the largest bf16 stays
                (0.0, inf, 0x7F80), (0.0, -inf, 0xFF80), (0.0, nan, None), (0.0, 0.0, 0x0000), (3.0, -3.0, 0x0000)]
    u = 2.0 ** -10      # fp16: 11 significant bits
    return [(1.0, u / 2, 0x3C00), (1.0, u + u / 2, 0x3C02), (-1.0, -u / 2, 0xBC00), (-1.0, -(u + u / 2), 0xBC02),
            (1.0, u / 2 + 2.0 ** -23, 0x3C01), (1.0, u / 2 - 2.0 ** -23, 0x3C00), (1.0, u + u / 2 - 2.0 ** -23, 0x3C01),
            (1.0, 1.0 - 2.0 ** -12, 0x4000), (-1.0, -(1.0 - 2.0 ** -12), 0xC000),
            (65280.0, 240.0, 0x7C00), (-65280.0, -240.0, 0xFC00), (65280.0, 239.0, 0x7BFF),        # 65520 = the tie between 65504 and 2^16 -> inf
            (0.0, 1e30, 0x7C00),
            (0.0, inf, 0x7C00), (0.0, -inf, 0xFC00), (0.0, nan, None), (0.0, 0.0, 0x0000), (3.0, -3.0, 0x0000)]


@pytest.mark.parametrize("form", [1, 2])
def test_conv_b16_rounding_edges_bit_exact(form):
    """identity centre-tap filter, fp32 bias: the accumulator of channel c is x_c + bias_c exactly, and its 16-bit store must be the RNE rounding
    of it.  Truncation fails the ties that go up, round-half-up the ties that go down.  NaN / inf are ordinary data here.  A second call with
    LeakyReLU makes -0.0 (the smallest negative fp32 number times 0.2f) and checks its sign survives."""
    cases = _edge_cases(form)
    B, H, W = 1, 8, 8
    x = torch.zeros(B, 32, H, W)
    bias = torch.zeros(32)
    for c, (xv, bv, _) in enumerate(cases):
        x[:, c], bias[c] = xv, bv
    assert same_bits(x.to(torch.bfloat16).float(), x)
    w = torch.zeros(32, 32, 3, 3)
    w[torch.arange(32), torch.arange(32), 1, 1] = 1.0
    xin = G.act16_from_nchw_x16(x.to(DEV))
    wp = G.pack_w_b16(w.to(DEV))
    for lrelu in (0, 1):
        bd = bias.clone()
        if lrelu:       # (positive cases pass through unchanged; the negative ones are replaced by the -0.0 probe)
            bd[[c for c, (xv, bv, _) in enumerate(cases) if xv < 0 or bv < 0]] = 0.0
            x_neg = [c for c, (xv, _, _) in enumerate(cases) if xv < 0]
            bd[x_neg] = 1.0                                             # x = -1: accumulator 0.0
            bd[len(cases)] = -1.401298464324817e-45                     # -2^-149; * 0.2f rounds to -0.0
        bdev = bd.to(DEV)
        o16 = G.act16_alloc(B, 1, H, W, DEV)
        o32 = torch.full((B, H, W, 32), 7.0, device=DEV)
        a = G.conv_args(**{"in": xin.data_ptr()}, in_chunks_total=1, in_chunk0=0, in_chunks=1, w=wp.data_ptr(), bias=bdev.data_ptr(), cout=32,
                        B=B, H=H, W=W, lrelu=lrelu, out16=o16.data_ptr(), out16_chunks_total=1, out16_chunk0=0, out32=o32.data_ptr(), out32_c=32)
        G.run_conv_x16(a, form)
        torch.cuda.synchronize()
        got32 = o32.permute(0, 3, 1, 2).cpu()
        got16 = G.act16_planes(o16, B, 1, H, W, OUT_T[form]).cpu()
        acc = (x + bd.view(1, -1, 1, 1))                                # fp32, exact by construction
        finite = ~torch.isnan(acc)
        if lrelu:
            acc = torch.where(acc >= 0, acc, acc * torch.tensor(0.2, dtype=torch.float32))
        assert torch.equal(got32[finite], acc[finite]) and torch.isnan(got32[~finite]).all()
        want16 = acc.to(OUT_T[form])
        assert torch.equal(bits(got16)[finite], bits(want16)[finite])
        assert torch.isnan(got16.float()[~finite]).all()
        if not lrelu:
            for c, (_, _, pattern) in enumerate(cases):
                if pattern is not None:
                    assert (bits(got16)[:, c].to(torch.int32) & 0xFFFF == pattern).all(), (c, cases[c], hex(int(bits(got16)[0, c, 0, 0]) & 0xFFFF))
        else:
            c = len(cases)
            assert (bits(got16)[:, c].to(torch.int32) & 0xFFFF == 0x8000).all() and (bits(got32.to(OUT_T[form]))[:, c].to(torch.int32) & 0xFFFF == 0x8000).all()
        assert G.border_is_zero(o16, B, 1, H, W)


@pytest.mark.parametrize("cout,cin,mask_chunk0", [(32, 64, 0), (32, 96, 3), (64, 192, 1)])
def test_conv_b16_lrelu_derivative_mask(cout, cin, mask_chunk0):
    """the gradient convs: the output times the LeakyReLU derivative taken from SAVED fp16 planes -- 1 where the saved value is > 0, 0.2 everywhere
    else: negative values, +0 and -0 (torch's leaky_relu backward)"""
    B, H, W = 2, 16, 40
    x, w = rnd((B, cin, H, W), 31), rnd((cout, cin, 3, 3), 32, -0.1, 0.1)
    mask_planes = 6
    m = rnd((B, 32 * mask_planes, H, W), 33)
    sel = torch.randint(0, 4, m.shape, generator=torch.Generator().manual_seed(34))
    m = torch.where(sel == 0, torch.zeros_like(m), torch.where(sel == 1, -torch.zeros_like(m), m))      # a quarter +0, a quarter -0
    mbuf = G.act16_from_nchw_x16(m.to(DEV), bf16=0)
    saved = G.act16_planes(mbuf, B, mask_planes, H, W, torch.float16).cpu()
    assert same_bits(saved, m.half())
    neg0 = bits(saved) == -32768
    assert neg0.any() and (saved == 0).sum() > neg0.sum() and (saved > 0).any() and (saved < 0).any()
    xin = G.act16_from_nchw_x16(x.to(DEV))
    o16 = G.act16_alloc(B, cout // 32, H, W, DEV)
    o32 = torch.zeros((B, H, W, cout), device=DEV)
    a = G.conv_args(**{"in": xin.data_ptr()}, in_chunks_total=cin // 32, in_chunk0=0, in_chunks=cin // 32, w=G.pack_w_b16(w.to(DEV)).data_ptr(),
                    bias=None, cout=cout, B=B, H=H, W=W, out16=o16.data_ptr(), out16_chunks_total=cout // 32, out16_chunk0=0,
                    out32=o32.data_ptr(), out32_c=cout)
    G.run_conv_x16(a, 1, mbuf, mask_planes, mask_chunk0)
    torch.cuda.synchronize()
    mm = saved[:, 32 * mask_chunk0: 32 * mask_chunk0 + cout].double()
    slope = torch.where(mm > 0, torch.ones_like(mm), torch.full_like(mm, float(np.float32(0.2))))
    want = G.ref_conv64(G.b16(x), G.b16(w), None) * slope
    got = o32.permute(0, 3, 1, 2)
    assert O.rel_l2(got.cpu(), want) <= TIGHT
    # ... and element by element: which slope was applied (the two candidates differ by a factor 5)
    plain = G.ref_conv64(G.b16(x), G.b16(w), None)
    big = plain.abs() > 1e-3
    ratio = (got.cpu().double() / plain)[big]
    assert torch.allclose(ratio, slope[big], rtol=1e-3, atol=0)
    assert same_bits(G.act16_planes(o16, B, cout // 32, H, W), got.to(torch.bfloat16))
    assert G.border_is_zero(o16, B, cout // 32, H, W)


def _pack_order(cout, cin):
    """for every 16-bit slot of the WPACK16 image of a (cout, cin) conv: 1 + the flat OIHW index of the weight it holds, 0 for padding -- read
    off srbh_pack_conv3x3_f16 with index-coded weights (integers up to 2048 are exact in fp16: two passes, radix 2048)"""
    n = cout * cin * 9
    code = torch.arange(1, n + 1, dtype=torch.int64)
    order = None
    for digit in (code % 2048, code // 2048):
        pk = G.pack_w(digit.float().view(cout, cin, 3, 3).to(DEV)).view(torch.float16).cpu().to(torch.int64)
        order = pk if order is None else order + 2048 * pk
    real = order[order > 0]
    assert real.numel() == n and torch.equal(real.sort().values, code)      # every weight exactly once
    return order


def _with_ties(t, seed):
    """half of the elements replaced by exact ties between two bf16 neighbours (bit 15 set, bits 14..0 clear)"""
    t = t.to(torch.bfloat16).float()
    tie = torch.rand(t.shape, generator=torch.Generator().manual_seed(seed)) < 0.5
    return torch.where(tie, (t.contiguous().view(torch.int32) | 0x8000).view(torch.float32), t)


def _tie_weights(cout, cin, seed):
    return _with_ties(rnd((cout, cin, 3, 3), seed, -0.1, 0.1), seed + 1)


@pytest.mark.parametrize("cin,cout", TRUNK_SHAPES + [(64, 3)])
def test_packs_b16_are_rne_in_the_fp16_packs_order(cin, cout):
    L = _lib.lib()
    order = _pack_order(cout, cin)
    w = _tie_weights(cout, cin, 40 + cin + cout)
    wd = w.to(DEV)
    nbytes = L.srbh_wpack16_bytes(cout, cin)
    assert order.numel() * 2 == nbytes
    want = torch.zeros(order.numel(), dtype=torch.int16)
    wb = bits(w.to(torch.bfloat16)).flatten()
    want[order > 0] = wb[order[order > 0] - 1]
    one = G.pack_w_b16(wd)
    torch.cuda.synchronize()
    assert torch.equal(one.view(torch.int16).cpu(), want)
    truncated = (w.view(torch.int32) >> 16).to(torch.int16).flatten()
    assert not torch.equal(truncated, wb)                                   # (the data can tell truncation from RNE)
    # the same through the many-packs launch: a bf16 row and an fp16 row of the same weight, bias copied by the fp16 row
    b = rnd((cout,), 5)
    bsrc = b.to(DEV)
    bdst = torch.zeros((cout + 31) // 32 * 32, device=DEV)
    many = torch.zeros(2, nbytes, dtype=torch.uint8, device=DEV)
    desc_t = np.dtype([("w", np.uint64), ("packed", np.uint64), ("bias_src", np.uint64), ("bias_dst", np.uint64), ("cout", np.int32),
                       ("cin", np.int32), ("bf16", np.int32), ("pad", np.int32)])
    tab = np.zeros(2, dtype=desc_t)
    tab[0] = (wd.data_ptr(), many[0].data_ptr(), bsrc.data_ptr(), bdst.data_ptr(), cout, cin, 0, 0)
    tab[1] = (wd.data_ptr(), many[1].data_ptr(), 0, 0, cout, cin, 1, 0)
    table = torch.from_numpy(tab.view(np.uint8).copy()).to(DEV)
    _lib.check(L.srbh_pack_conv3x3_many(table.data_ptr(), 2, nbytes // 2, _lib.stream_ptr()), "pack_conv3x3_many")
    torch.cuda.synchronize()
    assert torch.equal(many[1], one)
    assert torch.equal(many[0], G.pack_w(wd))
    assert torch.equal(bdst[:cout].cpu(), b) and not bdst[cout:].any()
    want_h = torch.zeros(order.numel(), dtype=torch.int16)
    want_h[order > 0] = bits(w.half()).flatten()[order[order > 0] - 1]
    assert torch.equal(many[0].view(torch.int16).cpu(), want_h)


@pytest.mark.parametrize("bf16", [1, 0])
@pytest.mark.parametrize("scale", [1.0, 0.2, 0.04])
def test_nhwc32_to_act16_rounds_the_fp32_product(scale, bf16):
    """the values the code converts with: 1 (planes), 0.2 and 0.04 (gradient streams): bits == (x * scale) formed in fp32, then RNE"""
    B, Cc, H, W, total, chunk0 = 2, 64, 9, 21, 5, 2
    dt = torch.bfloat16 if bf16 else torch.float16
    x = rnd((B, Cc, H, W), 50, -4.0, 4.0)
    x[:, :32] = _with_ties(x[:, :32], 51)          # exact bf16 ties at scale 1
    buf = G.act16_alloc(B, total, H, W, DEV)
    G.act16_from_nchw_x16(x.to(DEV), bf16=bf16, chunks_total=total, chunk0=chunk0, scale=scale, buf=buf)
    want = (x * torch.tensor(scale, dtype=torch.float32)).to(dt)
    planes = G.act16_planes(buf, B, total, H, W, dt).cpu()
    assert same_bits(planes[:, 32 * chunk0: 32 * chunk0 + Cc], want)
    if bf16 and scale == 1.0:
        assert not same_bits((x.view(torch.int32) >> 16).to(torch.int16).view(torch.bfloat16), want)      # (truncation would differ)
    rest = [c for c in range(32 * total) if not 32 * chunk0 <= c < 32 * chunk0 + Cc]
    assert not bits(planes[:, rest]).any() and G.border_is_zero(buf, B, total, H, W)
