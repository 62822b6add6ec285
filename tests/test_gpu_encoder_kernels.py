"""The inference BatchNorm, affine + activation and squeeze-and-excitation kernels of csrc/srbh_enc_eval.hip (and srbh_bn_eval_scale_shift),
each entry point on its own through the C ABI against the float64 functions of tests/encoder_kernels_oracle.py, at the shapes where
their dispatch changes form: the float4 and the scalar affine pass (plane sizes that are no multiple of 4, pointers that are only
4-byte aligned, y aliasing x, more work items than one grid stride), the wave-per-plane and the small-plane pooling kernels with ragged
plane counts, every loop of the hidden-layer dot product, both sides of the gate kernel's SQ <= 128 switch with a ragged last image
chunk, the quad and the wave-per-plane gate + scale kernels.

Every output (and the in-place y) lives inside a larger NaN-filled device buffer with 64 floats of slack on either side: after the call
the slack is still NaN, the output holds no NaN, and every input is bit-identical to its clone.

Bounds: relative L2 against the oracle, 2e-6 for the affine / pooling / hidden-layer / BatchNorm-folding kernels (the figure
srbh_dwconv_eval_fwd holds in tests/test_gpu_dwconv.py with two __expf SiLUs in it), 3e-6 for the two gate kernels (the figure of
srbh_pwconv_fwd_epi); pooled means: max abs error <= 1e-5 * max |y|.  Each test prints its error next to the error of the stock fp32 op
chain on the same device against the same oracle.

Measured on an MI355X, largest error over the cases of each entry point (bound; the stock fp32 chain's largest error beside it):
  srbh_affine_act_nchw        6.8e-8   (2e-6; stock 7.2e-8)
  srbh_affine_act_add_nchw    6.3e-8   (2e-6; stock 1.4e-7)
  srbh_affine_act_pool_nchw   y 6.6e-8 (2e-6; stock 7.4e-8), pooled 6.6e-8 of max |y| (1e-5; stock 7.4e-8)
  srbh_se_hidden              9.1e-7   (2e-6; stock 3.4e-6) -- B = 1, C = 448, SQ = 1: a single output whose 448 terms largely cancel
  srbh_se_gate                5.6e-8   (3e-6; stock 9.0e-8), gates between 0.008 and 0.992
  srbh_se_gate_scale          6.5e-8   (3e-6; stock 7.9e-8)
  srbh_bn_eval_scale_shift    scale 1.0e-7, shift 1.2e-7 (2e-6; stock 7.3e-8, 6.2e-8)
No case needed a bound other than its starting figure."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import encoder_kernels_oracle as O
from tests.gpu_util import GuardedBuffers as Buffers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INFER, GATE = 2e-6, 3e-6


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _act32(u, act):
    return F.silu(u) if act == 1 else (F.relu(u) if act == 2 else u)


def _affine_inputs(B, C, HW, g, with_res):
    x = torch.randn((B, C, HW), generator=g) * 1.5 + 0.4
    scale, shift = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    res = torch.randn((B, C, HW), generator=g) if with_res else None
    return x, scale, shift, res


def _affine_call(L, x, scale, shift, res, y, B, C, HW, act):
    from srbh_amd import _lib
    if res is None:
        _lib.check(L.srbh_affine_act_nchw(x.data_ptr(), scale.data_ptr(), shift.data_ptr(), y.data_ptr(), B, C, HW, act, _lib.stream_ptr()), "affine_act_nchw")
    else:
        _lib.check(L.srbh_affine_act_add_nchw(x.data_ptr(), scale.data_ptr(), shift.data_ptr(), res.data_ptr(), y.data_ptr(), B, C, HW, act,
                                              _lib.stream_ptr()), "affine_act_add_nchw")


def _affine_stock(x, scale, shift, res, act):
    u = _act32(x * scale.view(1, -1, 1) + shift.view(1, -1, 1), act)
    return u if res is None else u + res


def _run_affine(B, C, HW, act, with_res, offsets=(0, 0, 0), alias=False, seed=0):
    """one call of srbh_affine_act_nchw / _add_nchw; offsets: floats past 16-byte alignment of (x, y, res).  Returns (y, error)"""
    from srbh_amd import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(seed + B * 1000 + C * 10 + act)
    x, scale, shift, res = _affine_inputs(B, C, HW, g, with_res)
    bufs = Buffers()
    sc, sh = bufs.inp(scale), bufs.inp(shift)
    rs = bufs.inp(res, offsets[2]) if with_res else None
    if alias:
        xd = yd = bufs.out(x.shape, offsets[1], fill=x)
    else:
        xd, yd = bufs.inp(x, offsets[0]), bufs.out(x.shape, offsets[1])
    stock = _affine_stock(x.to(DEV), sc, sh, rs, act)
    _affine_call(L, xd, sc, sh, rs, yd, B, C, HW, act)
    bufs.verify()
    want = O.affine_act(x, scale, shift, act, res)
    e, es = rel(yd, want), rel(stock, want)
    print(f"affine_act{'_add' if with_res else ''} B={B} C={C} HW={HW} act={act} offsets={offsets} alias={alias}: err {e:.3e} (stock fp32 chain {es:.3e})")
    return yd, e


AFFINE_SHAPES = [(1, 1, 1), (3, 5, 9), (2, 7, 4), (5, 37, 64), (2, 3, 1024)]


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("B,C,HW", AFFINE_SHAPES)
def test_affine_act_matches_the_oracle(B, C, HW, act, with_res):
    """float4 form (HW % 4 == 0) and scalar form, C = 1, a channel index that wraps across images; each activation, with and without the
    skip connection"""
    _, e = _run_affine(B, C, HW, act, with_res)
    assert e <= INFER


@pytest.mark.parametrize("which", ["x", "y", "res"])
def test_affine_act_takes_pointers_that_are_only_4_byte_aligned(which):
    """the documented scalar fallback: any of x, y, res one float past a 16-byte boundary; the call succeeds and gives the values of the
    aligned call, bit for bit (the two forms do the same arithmetic per element)"""
    offsets = tuple(int(which == n) for n in ("x", "y", "res"))
    aligned, e0 = _run_affine(2, 7, 4, 1, True)
    got, e = _run_affine(2, 7, 4, 1, True, offsets=offsets)
    assert e0 <= INFER and e <= INFER
    assert torch.equal(got, aligned)


@pytest.mark.parametrize("B,C,HW", [(5, 37, 64), (3, 5, 9)])
def test_affine_act_in_place(B, C, HW):
    """include/srbh.h: "y may alias x" -- the float4 and the scalar form"""
    sep, e0 = _run_affine(B, C, HW, 1, True)
    got, e = _run_affine(B, C, HW, 1, True, alias=True)
    assert e0 <= INFER and e <= INFER
    assert torch.equal(got, sep)


@pytest.mark.parametrize("B,C,HW,with_res", [(5, 7, 245760, True), (3, 7, 104859, False)])
def test_affine_act_beyond_one_grid_stride(B, C, HW, with_res):
    """more than 8192 * 256 work items, so that the workgroups of the capped grid take a second stride: the float4 form (5 * 7 * 245760 / 4
    items) and the scalar form (HW odd)"""
    items = B * C * (HW // 4 if HW % 4 == 0 else HW)
    assert items > O.GRID_CAP_ITEMS
    _, e = _run_affine(B, C, HW, 1, with_res)
    assert e <= INFER


POOL_EXTRA = [(9, 1, 7, 0), (32, 1, 7, 2), (64, 5, 37, 2), (2, 5, 37, 0)]


@pytest.mark.parametrize("HW,B,C,act", [(hw, b, c, 1) for hw in (1, 2, 32, 9, 36, 64, 81, 1024) for b, c in ((1, 1), (1, 7), (5, 37))] + POOL_EXTRA)
def test_affine_act_pool_matches_the_oracle(HW, B, C, act):
    """HW in {1, 2, 32}: the small-plane kernel (64 / HW planes per wave; with 7 or 185 planes the last wave is partly empty, and
    planes * HW is no multiple of 64); the other sizes: a wave per plane with planes % 4 != 0, plane sizes that are no power of two.
    y and the per-plane means; the same bits on a second run (fixed reduction tree)"""
    from srbh_amd import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(HW * 7 + B * C + act)
    x, scale, shift, _ = _affine_inputs(B, C, HW, g, False)
    assert (B * C) % 4 != 0 and (HW not in (1, 2, 32) or B * C == 1 or (B * C * HW) % 64 != 0)
    runs = []
    for _ in range(2):
        bufs = Buffers()
        xd, sc, sh = bufs.inp(x), bufs.inp(scale), bufs.inp(shift)
        yd, pd = bufs.out(x.shape), bufs.out((B, C))
        _lib.check(L.srbh_affine_act_pool_nchw(xd.data_ptr(), sc.data_ptr(), sh.data_ptr(), yd.data_ptr(), pd.data_ptr(), B, C, HW, act,
                                               _lib.stream_ptr()), "affine_act_pool_nchw")
        bufs.verify()
        runs.append((yd, pd))
    (yd, pd), (y2, p2) = runs
    stock = _affine_stock(xd, sc, sh, None, act)
    want, want_p = O.affine_act_pool(x, scale, shift, act)
    e, es = rel(yd, want), rel(stock, want)
    ep = float((pd.double().cpu() - want_p).abs().max()) / float(want.abs().max())
    eps_ = float((stock.mean(2).double().cpu() - want_p).abs().max()) / float(want.abs().max())
    print(f"affine_act_pool B={B} C={C} HW={HW} act={act}: y err {e:.3e} (stock {es:.3e}), pooled max abs / max|y| {ep:.3e} (stock {eps_:.3e})")
    assert e <= INFER
    assert ep <= 1e-5
    assert torch.equal(yd, y2) and torch.equal(pd, p2)


def _se_weights(rows, cols, g):
    """nn.Conv2d(cols, rows, 1)'s default initialisation with the weight times 3, as tests/test_gpu_mbconv.py scales it: gates spread over (0, 1)"""
    bound = 1.0 / math.sqrt(cols)
    w = (torch.rand((rows, cols), generator=g) * 2 - 1) * bound * 3.0
    b = (torch.rand(rows, generator=g) * 2 - 1) * bound
    return w, b


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("SQ", [1, 3, 6, 28, 112])
@pytest.mark.parametrize("C", [8, 64, 200, 257, 448, 2688])
def test_se_hidden_matches_the_oracle(C, SQ, B):
    """one wave per (b, j) dot product: C below one wave, the four-way unrolled loop, its tail, and both in one wave (C = 200: lanes 0 .. 7
    take the unrolled step, the others the tail); SQ % 4 != 0 leaves waves of the last workgroup without a row"""
    from srbh_amd import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(C * 31 + SQ * 7 + B)
    pooled = torch.randn((B, C), generator=g) * 0.5 + 0.3
    w1, b1 = _se_weights(SQ, C, g)
    bufs = Buffers()
    pd, wd, bd = bufs.inp(pooled), bufs.inp(w1), bufs.inp(b1)
    hd = bufs.out((B, SQ))
    _lib.check(L.srbh_se_hidden(pd.data_ptr(), wd.data_ptr(), bd.data_ptr(), hd.data_ptr(), B, C, SQ, _lib.stream_ptr()), "se_hidden")
    bufs.verify()
    want = O.se_hidden(pooled, w1, b1)
    e, es = rel(hd, want), rel(F.silu(F.linear(pd, wd, bd)), want)
    print(f"se_hidden B={B} C={C} SQ={SQ}: err {e:.3e} (stock fp32 chain {es:.3e})")
    assert e <= INFER


@pytest.mark.parametrize("B,C,SQ", [(1, 5, 1), (8, 16, 6), (9, 19, 16), (70, 144, 17), (1, 144, 112), (9, 5, 128), (8, 19, 129), (70, 16, 200)])
def test_se_gate_matches_the_oracle(B, C, SQ):
    """both sides of the SQ <= 128 switch (register-held row vs the strided loop) and the `sub + 16 u < SQ` edges (SQ = 16, 17, 128);
    C % 16 != 0 leaves channel slots of the last workgroup empty; B = 9 and 70 end on a ragged chunk of SE_GATE_IB = 8 images"""
    from srbh_amd import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(B * 977 + C * 13 + SQ)
    hidden = F.silu(torch.randn((B, SQ), generator=g))
    w2, b2 = _se_weights(C, SQ, g)
    bufs = Buffers()
    hd, wd, bd = bufs.inp(hidden), bufs.inp(w2), bufs.inp(b2)
    gd = bufs.out((B, C))
    _lib.check(L.srbh_se_gate(hd.data_ptr(), wd.data_ptr(), bd.data_ptr(), gd.data_ptr(), B, C, SQ, _lib.stream_ptr()), "se_gate")
    bufs.verify()
    want = O.se_gate(hidden, w2, b2)
    e, es = rel(gd, want), rel(torch.sigmoid(F.linear(hd, wd, bd)), want)
    print(f"se_gate B={B} C={C} SQ={SQ}: err {e:.3e} (stock fp32 chain {es:.3e}); gates in [{float(want.min()):.3f}, {float(want.max()):.3f}]")
    assert e <= GATE


def _run_gate_scale(B, C, SQ, HW, offset):
    from srbh_amd import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(B * 977 + C * 13 + SQ * 3 + HW)
    y = F.silu(torch.randn((B, C, HW), generator=g) * 1.5 + 0.4)
    hidden = F.silu(torch.randn((B, SQ), generator=g))
    w2, b2 = _se_weights(C, SQ, g)
    bufs = Buffers()
    hd, wd, bd = bufs.inp(hidden), bufs.inp(w2), bufs.inp(b2)
    yd = bufs.out(y.shape, offset, fill=y)
    stock = y.to(DEV) * torch.sigmoid(F.linear(hd, wd, bd)).unsqueeze(2)
    _lib.check(L.srbh_se_gate_scale(yd.data_ptr(), hd.data_ptr(), wd.data_ptr(), bd.data_ptr(), B, C, SQ, HW, _lib.stream_ptr()), "se_gate_scale")
    bufs.verify()
    want = O.se_gate_scale(y, hidden, w2, b2)
    e, es = rel(yd, want), rel(stock, want)
    print(f"se_gate_scale B={B} C={C} SQ={SQ} HW={HW} y offset {offset}: err {e:.3e} (stock fp32 chain {es:.3e})")
    return yd, e


@pytest.mark.parametrize("HW,SQ", [(4, 1), (4, 6), (16, 28), (64, 112), (256, 1), (256, 6), (256, 28), (256, 112), (256, 200)])
def test_se_gate_scale_quad_planes(HW, SQ):
    """planes of 4 / 16 / 64 / 256 elements: the float4 kernel whose HW / 4 threads per plane share the gate (planes * HW is no multiple of
    its 1024-element workgroups; at HW = 256, G = 64: SQ = 200 runs the unrolled loop in lanes 0 .. 7 and the tail loop, 28 leaves lanes
    without a term), and with y one float past a 16-byte boundary the wave-per-plane kernel: the same result from both"""
    B, C = 3, 5
    assert (B * C * HW) % 1024 != 0
    a, ea = _run_gate_scale(B, C, SQ, HW, 0)
    b, eb = _run_gate_scale(B, C, SQ, HW, 1)
    assert ea <= GATE and eb <= GATE
    assert rel(a, b) <= GATE


@pytest.mark.parametrize("B,C,SQ,HW", [(3, 5, 6, 1), (3, 5, 28, 9), (3, 5, 200, 1024), (5, 37, 112, 9), (5, 37, 1, 64)])
def test_se_gate_scale_other_planes(B, C, SQ, HW):
    """the wave-per-plane kernel on plane sizes the quad kernel does not take (and one it does, at 185 planes)"""
    _, e = _run_gate_scale(B, C, SQ, HW, 0)
    assert e <= GATE


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("eps", [1e-3, 1e-5])
@pytest.mark.parametrize("C", [1, 7, 448])
def test_bn_eval_scale_shift_matches_the_oracle(C, eps, affine):
    """running variances of 0 and 1e-8 among ordinary ones; with and without gamma / beta (null pointers: 1 and 0)"""
    from srbh_amd import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(C + int(eps * 1e6))
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    mean, var = torch.randn(C, generator=g) * 0.4, torch.rand(C, generator=g) + 0.1
    var[0] = 0.0 if (C > 1 or eps == 1e-3) else 1e-8
    if C > 1:
        var[1] = 1e-8
    bufs = Buffers()
    gd, bd = (bufs.inp(gamma), bufs.inp(beta)) if affine else (None, None)
    md, vd = bufs.inp(mean), bufs.inp(var)
    sc, sh = bufs.out((C,)), bufs.out((C,))
    _lib.check(L.srbh_bn_eval_scale_shift(C, gd.data_ptr() if affine else None, bd.data_ptr() if affine else None, md.data_ptr(), vd.data_ptr(),
                                          eps, sc.data_ptr(), sh.data_ptr(), _lib.stream_ptr()), "bn_eval_scale_shift")
    bufs.verify()
    want_s, want_h = O.bn_eval_scale_shift(gamma if affine else None, beta if affine else None, mean, var, eps)
    inv = torch.rsqrt(vd + eps)
    st_s = gd * inv if affine else inv
    st_h = (bd if affine else 0.0) - md * st_s
    es, eh = rel(sc, want_s), rel(sh, want_h)
    print(f"bn_eval_scale_shift C={C} eps={eps} affine={affine}: scale err {es:.3e} (stock {rel(st_s, want_s):.3e}), shift err {eh:.3e} (stock {rel(st_h, want_h):.3e})")
    assert es <= INFER and eh <= INFER
