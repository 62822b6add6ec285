"""GPU: every compiled form of the U-Net decoders' 3x3 convolutions (csrc/srbh_dconv.hip) against float64 references, through the C ABI.

dconv_kernel<LOGW, NPX, MB, BF16> has 5 plane sizes x 2 tile widths x 2 channel-block counts x 2 operand types = 40 forms with their own
staging geometry (whole images per tile, the whole plane, row strips with halo rows); dconv_wgrad_kernel<LOGW, MO> has 10.  The launchers
pick the form from the shape alone, so a test that wants a form has to bring a shape that selects it: every case here ASKS the library
(srbh_dconv_fwd_plan / srbh_dconv_wgrad_plan: the launchers' own rule) which form its shape runs, and the census at the end asserts that the
forms the production batches (B = 32, 64, 128) select are among the covered ones.

Checks per form: integer operands with an exact fp32 result (torch.equal with the float64 reference: the index map -- taps, halo rows and
columns, image boundaries inside multi-image tiles, ragged last tile, ragged channel block), randn operands with an ELEMENT-WISE bound
|got - ref| <= 2 n 2^-24 S (n terms, S = the same sum over absolute values: an fp32 sum of exact products in any order; the factor 2 covers
the undocumented rounding inside a matrix-core instruction's own 16-term reduction), and the memory contract of gpu_util.GuardedBuffers
(guards intact, inputs unchanged, every output element written).

Largest measured err / bound per form (MI355X, the shapes and seeds below; `pytest -s` prints them).  Forward / data gradient, n = 432:

     W   NPX  MB    fp16     bf16   |   W   NPX  MB    fp16     bf16
     4    64   1   0.0008   0.0005  |  16   256   1   0.0024   0.0020
     4    64   2   0.0020   0.0020  |  16   256   2   0.0023   0.0020
     4   256   1   0.0024   0.0024  |  32    64   1   0.0015   0.0012
     4   256   2   0.0027   0.0032  |  32    64   2   0.0021   0.0022
     8    64   1   0.0009   0.0009  |  32   256   1   0.0025   0.0021
     8    64   2   0.0024   0.0020  |  32   256   2   0.0021   0.0020
     8   256   1   0.0021   0.0024  |  64    64   1   0.0015   0.0021
     8   256   2   0.0020   0.0026  |  64    64   2   0.0019   0.0020
    16    64   1   0.0011   0.0010  |  64   256   1   0.0025   0.0017
    16    64   2   0.0019   0.0019  |  64   256   2   0.0026   0.0030

(norm-wise 0.8e-7 ... 1.3e-7 everywhere: the worst-case bound is ~400x what random rounding errors reach, yet any slip of the index map moves
an element by O(S), 400x the bound.)  Weight gradient (W, MO, nsplit: err / bound, n = B W W): (4,1,1) 0.034, (4,2,2) 1.6e-4, (8,1,1) 8.3e-4,
(8,2,7) 3e-5, (16,1,1) 2.5e-4, (16,2,3) 1.1e-4, (32,1,4) 5e-5, (32,2,6) 3e-5, (64,1,512) < 1e-5, (64,2,16) 1e-5; norm-wise 1.7e-8 ... 1.8e-7.
At n = 262 144 the element-wise bound is wider than the gradient itself, which is why the norm bound stays beside it.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests.gpu_util import GuardedBuffers

gpu = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24

# the ten convolutions of one decoder (tests/test_gpu_dconv.py SHAPES): (Cin, Cout, W)
DECODER = [(608, 256, 4), (256, 256, 4), (312, 128, 8), (128, 128, 8), (160, 64, 16), (64, 64, 16), (112, 32, 32), (32, 32, 32), (32, 16, 64),
           (16, 16, 64)]
PRODUCTION_B = (32, 64, 128)

# ---- (a) one shape per forward form: (W, NPX, MB) -> (B, Cout); Cin = 40 = two full 16-channel chunks + a half-full one (the two-stage
# pipeline wraps), Cout ragged where the form allows it (MB = 2 needs an even block count: 24 -> 2 blocks, the second half full),
# B no multiple of the images per tile where a tile holds several whole images, one MB = 1 case with three channel blocks (Cout = 40)
CIN = 40
FWD_FORMS = {
    (4, 64, 1): (1, 8), (4, 64, 2): (1021, 24), (4, 256, 1): (1009, 56), (4, 256, 2): (1009, 120),
    (8, 64, 1): (1, 8), (8, 64, 2): (256, 24), (8, 256, 1): (1021, 8), (8, 256, 2): (1021, 24),
    (16, 64, 1): (1, 8), (16, 64, 2): (64, 24), (16, 256, 1): (86, 40), (16, 256, 2): (256, 24),
    (32, 64, 1): (1, 8), (32, 64, 2): (16, 24), (32, 256, 1): (64, 8), (32, 256, 2): (64, 24),
    (64, 64, 1): (1, 8), (64, 64, 2): (4, 24), (64, 256, 1): (16, 8), (64, 256, 2): (16, 24),
}
ALL_FWD_FORMS = {(W, npx, mb) for W in (4, 8, 16, 32, 64) for npx in (64, 256) for mb in (1, 2)}
assert set(FWD_FORMS) == ALL_FWD_FORMS and len(ALL_FWD_FORMS) == 20
for (_W, _npx, _mb), (_B, _Cout) in FWD_FORMS.items():
    if _W * _W < _npx and _npx // (_W * _W) > 1 and _B > 1:
        assert _B % (_npx // (_W * _W)) != 0, (_W, _npx, _mb)          # the last tile of whole images is ragged
assert any(mb == 1 and (co + 15) // 16 >= 3 and ((co + 15) // 16) % 2 == 1 for (_, _, mb), (_, co) in FWD_FORMS.items())
assert 9 * CIN * 16 < 2 ** 24           # integer operands from [-4, 4]: every partial sum is an integer below 2^24 -> fp32 is exact in any order

# ---- (d) one shape per weight-gradient form: (W, MO) -> (B, Cin, Cout, nsplit); MO = 2 iff Cout % 32 == 0; Cin ragged (but for the
# production shape that gives 512 splits); split counts 1 (B = 1 at 4x4: ONE 16-pixel step for four waves), 2, 7 (312 -> 128 at 8x8, B = 64:
# 256 steps over 28 waves), 512 (16 -> 16 at 64x64, B = 64: one dW block)
WGRAD_FORMS = {
    (4, 1): (1, 24, 24, 1), (4, 2): (70, 24, 32, 2),
    (8, 1): (5, 40, 24, None), (8, 2): (64, 312, 128, 7),
    (16, 1): (3, 24, 40, None), (16, 2): (6, 40, 64, None),
    (32, 1): (2, 24, 48, None), (32, 2): (3, 8, 32, None),
    (64, 1): (64, 16, 16, 512), (64, 2): (2, 24, 32, None),
}
ALL_WGRAD_FORMS = {(W, mo) for W in (4, 8, 16, 32, 64) for mo in (1, 2)}
assert set(WGRAD_FORMS) == ALL_WGRAD_FORMS and len(ALL_WGRAD_FORMS) == 10
assert {1, 2, 7, 512} <= {v[3] for v in WGRAD_FORMS.values()}
assert all(B * W * W * 9 < 2 ** 24 for (W, _), (B, _, _, _) in WGRAD_FORMS.items())     # integer operands from [-3, 3]: exact in fp32


def _L():
    from srbh_amd import _lib
    return _lib, _lib.lib()


def fwd_plan(B, Cout, W):
    _lib, L = _L()
    npx, mb = C.c_int(-1), C.c_int(-1)
    _lib.check(L.srbh_dconv_fwd_plan(B, Cout, W, C.byref(npx), C.byref(mb)), "dconv_fwd_plan")
    return npx.value, mb.value


def wgrad_plan(B, Cin, Cout, W):
    _lib, L = _L()
    mo, ns = C.c_int(-1), C.c_int(-1)
    _lib.check(L.srbh_dconv_wgrad_plan(B, Cin, Cout, W, C.byref(mo), C.byref(ns)), "dconv_wgrad_plan")
    return mo.value, ns.value


def r16(t, bf16):
    """the 16-bit operand the kernel multiplies (round to nearest even), as float64"""
    return (t.bfloat16() if bf16 else t.half()).double()


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _ints(shape, lim, gen):
    return torch.randint(-lim, lim + 1, shape, generator=gen).float()


def _pack(w, Cout, Cin, transpose_flip, bf16):
    """w: (Cout, Cin, 3, 3), or with transpose_flip the FORWARD weight (Cin, Cout, 3, 3) of which the kernel runs the data gradient"""
    _lib, L = _L()
    wd = w.to(DEV).contiguous()
    buf = torch.empty(L.srbh_hpack_h16_bytes(Cout, Cin, 3) // 2, dtype=torch.int16, device=DEV)
    _lib.check(L.srbh_hpack_conv_h16(wd.data_ptr(), Cout, Cin, 3, transpose_flip, bf16, buf.data_ptr(), _lib.stream_ptr()), "hpack_conv_h16")
    torch.cuda.synchronize()
    return buf.view(torch.uint8)


def run_fwd(x, w, Cout, bf16, transpose_flip, epi=None, refused=False):
    """one srbh_dconv_fwd / srbh_dconv_fwd_epi (epi = (scale | None, shift | None, act)) call on guarded buffers -> y on the host"""
    _lib, L = _L()
    B, Cin, W = x.shape[0], x.shape[1], x.shape[3]
    g = GuardedBuffers()
    xd = g.inp(x)
    pk = g.inp(_pack(w, Cout, Cin, transpose_flip, bf16), dtype=torch.uint8)
    y = g.out((B, Cout, W, W))
    if epi is None:
        rc = L.srbh_dconv_fwd(xd.data_ptr(), pk.data_ptr(), y.data_ptr(), B, Cin, Cout, W, W, bf16, _lib.stream_ptr())
    else:
        sc, sh, act = epi
        sc = None if sc is None else g.inp(sc).data_ptr()
        sh = None if sh is None else g.inp(sh).data_ptr()
        rc = L.srbh_dconv_fwd_epi(xd.data_ptr(), pk.data_ptr(), y.data_ptr(), B, Cin, Cout, W, W, bf16, sc, sh, act, _lib.stream_ptr())
    if refused:
        assert rc != 0, "the call should have been refused"
        g.verify(written=False)
        return None
    _lib.check(rc, "dconv_fwd")
    g.verify()
    return y.cpu()


def ref_fwd(x64, w64, transpose_flip):
    """float64 reference of what the kernel computes from these operands: the conv, or (transposed + flipped pack) the input gradient of
    the forward conv whose weight is w and whose output gradient is x"""
    if not transpose_flip:
        return F.conv2d(x64, w64, None, 1, 1)
    B, _, H, W = x64.shape
    return torch.nn.grad.conv2d_input((B, w64.shape[1], H, W), w64, x64, padding=1)


def _fwd_case(W, npx, mb, bf16, seed):
    """operands of one form: the fp16 cases run the forward conv, the bf16 cases the data gradient (transposed + flipped pack), as the
    autograd function does"""
    B, Cout = FWD_FORMS[(W, npx, mb)]
    assert fwd_plan(B, Cout, W) == (npx, mb), (fwd_plan(B, Cout, W), "the shape no longer selects the form it is here for")
    g = torch.Generator().manual_seed(seed + 1000 * W + 10 * npx + mb)
    wshape = (CIN, Cout, 3, 3) if bf16 else (Cout, CIN, 3, 3)
    return B, Cout, g, wshape


FWD_CASES = [pytest.param(W, npx, mb, bf16, id=f"W{W}-npx{npx}-mb{mb}-{'bf16' if bf16 else 'fp16'}")
             for (W, npx, mb) in sorted(FWD_FORMS) for bf16 in (0, 1)]
assert len(FWD_CASES) == 40


@gpu
@pytest.mark.parametrize("W,npx,mb,bf16", FWD_CASES)
def test_forward_form_integer_operands_exact(W, npx, mb, bf16):
    """the index map: integers from [-4, 4] are exact in fp16 and bf16, so is every product and (9 * Cin * 16 < 2^24) every partial sum:
    the fp32 result equals the float64 one bit for bit whatever the summation order"""
    B, Cout, g, wshape = _fwd_case(W, npx, mb, bf16, seed=1)
    x, w = _ints((B, CIN, W, W), 4, g), _ints(wshape, 4, g)
    got = run_fwd(x, w, Cout, bf16, transpose_flip=bf16)
    ref = ref_fwd(x.double(), w.double(), bf16)
    assert float(ref.abs().max()) < 2 ** 24
    bad = (got.double() != ref).nonzero()
    assert torch.equal(got.double(), ref), (len(bad), bad[:8].tolist())


@gpu
@pytest.mark.parametrize("W,npx,mb,bf16", FWD_CASES)
def test_forward_form_randn_elementwise_bound(W, npx, mb, bf16):
    """randn operands against the float64 conv of the same 16-bit-rounded operands, element by element: |got - ref| <= 2 n 2^-24 S with
    n = 9 * 16 * nchunk terms and S = the conv of the absolute rounded operands; and the module's norm-wise bound"""
    B, Cout, g, wshape = _fwd_case(W, npx, mb, bf16, seed=2)
    x, w = torch.randn((B, CIN, W, W), generator=g), torch.randn(wshape, generator=g)
    got = run_fwd(x, w, Cout, bf16, transpose_flip=bf16).double()
    x16, w16 = r16(x, bf16), r16(w, bf16)
    ref, S = ref_fwd(x16, w16, bf16), ref_fwd(x16.abs(), w16.abs(), bf16)
    n = 9 * 16 * ((CIN + 15) // 16)
    bound = 2 * n * EPS * S
    err = (got - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"\n[dconv form] W={W} NPX={npx} MB={mb} {'bf16' if bf16 else 'fp16'}: max err/bound = {ratio:.4f}, rel = {rel(got, ref):.3e}")
    assert bool((err <= bound).all()), ratio
    assert rel(got, ref) <= 2e-6


# ---- (b) rounding of the staged operands ----------------------------------------------------------------------------------------------
def _tie_inputs(bf16, n, gen):
    """n exact ties between neighbouring fp16 / bf16 values (both normal fp16 magnitudes, 2^-14 ... 2^15), random signs, and the value
    round-to-nearest-EVEN gives for each"""
    if bf16:
        k = torch.randint(0x3880, 0x4700, (n,), generator=gen, dtype=torch.int32)             # bf16 bit patterns of 2^-14 ... < 2^15
        lo, hi = (k << 16).view(torch.float32), ((k + 1) << 16).view(torch.float32)
        even = ((k + (k & 1)) << 16).view(torch.float32)
    else:
        k = torch.randint(0x0400, 0x7800, (n,), generator=gen, dtype=torch.int32)             # fp16 bit patterns of 2^-14 ... < 2^15
        lo, hi = k.to(torch.int16).view(torch.float16).float(), (k + 1).to(torch.int16).view(torch.float16).float()
        even = (k + (k & 1)).to(torch.int16).view(torch.float16).float()
    mid = (lo.double() + hi.double()) / 2
    assert torch.equal(mid.float().double(), mid)                     # the tie is an fp32 number
    sign = torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1
    return mid.float() * sign, even * sign


@gpu
@pytest.mark.parametrize("bf16", [0, 1])
def test_staged_operands_round_to_nearest_even(bf16):
    """a centre-tap identity weight copies the staged operand to the output: bit-equal to x.half() / x.bfloat16(), ties to even (fp16
    normal magnitudes only: an overflow would turn the zero taps into NaN, and fp16 subnormal handling is the hardware's)"""
    B, Cch, W = 3, 24, 8
    g = torch.Generator().manual_seed(5 + bf16)
    n = B * Cch * W * W
    ties, even = _tie_inputs(bf16, n // 2, g)
    rnd = torch.randn(n - n // 2, generator=g).clamp(-6, 6)
    rnd = torch.where(rnd.abs() < 2.0 ** -10, torch.full_like(rnd, 0.5), rnd)
    flat, want = torch.cat([ties, rnd]), torch.cat([even, r16(rnd, bf16).float()])
    perm = torch.randperm(n, generator=g)
    x, want = flat[perm].view(B, Cch, W, W), want[perm].view(B, Cch, W, W)
    assert torch.equal(r16(x, bf16).float(), want)                    # the framework's own rounding agrees on the ties
    w = torch.zeros(Cch, Cch, 3, 3)
    w[torch.arange(Cch), torch.arange(Cch), 1, 1] = 1.0
    got = run_fwd(x, w, Cch, bf16, transpose_flip=bf16)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# ---- (c) the epilogue against a reference -----------------------------------------------------------------------------------------------
EPI_FORMS = [(8, 256, 2), (16, 64, 2)]          # whole images per 256-pixel tile with a ragged batch; a 64-pixel form; both with Cout = 24


def _epi_ref(conv64, scale, shift, act):
    v = conv64 if scale is None else conv64 * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    return v.clamp_min(0.0) if act == 2 else v


@gpu
@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("W,npx,mb", EPI_FORMS)
def test_epilogue_against_float64(W, npx, mb, bf16):
    """y = act(fma(conv, scale[co], shift[co])) element-wise in float64: exact for integer operands with power-of-two scales; for randn
    operands the bound of the conv scaled by |scale| plus one fp32 rounding of the result.  scale has negative, zero and positive entries;
    act 0 and 2; and the allowed scale = shift = NULL with act = 2"""
    B, Cout = FWD_FORMS[(W, npx, mb)]
    assert fwd_plan(B, Cout, W) == (npx, mb) and Cout % 16 != 0
    g = torch.Generator().manual_seed(7 + W + bf16)
    co = torch.arange(Cout)
    # integer operands: |conv| <= 9 * 40 * 16 = 5760, scale a power of two in [1/4, 4], shift a multiple of 1/4: conv * scale + shift is a
    # multiple of 1/16 below 2^15 -- 19 bits, an fp32 number
    x, w = _ints((B, CIN, W, W), 4, g), _ints((Cout, CIN, 3, 3), 4, g)
    scale = torch.tensor([-2.0, 0.0, 0.5, 1.0, -0.25, 4.0])[co % 6]
    shift = torch.tensor([0.25, -3.0, 0.0, 1.5, 7.0])[co % 5]
    conv = ref_fwd(x.double(), w.double(), 0)
    for sc, sh, act in ((scale, shift, 0), (scale, shift, 2), (None, None, 2)):
        got = run_fwd(x, w, Cout, bf16, 0, epi=(sc, sh, act))
        assert torch.equal(got.double(), _epi_ref(conv, sc, sh, act)), (act, sc is None)
    # randn operands
    x, w = torch.randn((B, CIN, W, W), generator=g), torch.randn((Cout, CIN, 3, 3), generator=g)
    scale, shift = torch.randn(Cout, generator=g), torch.randn(Cout, generator=g)
    scale[1::5] = 0.0
    assert bool((scale < 0).any() and (scale == 0).any() and (scale > 0).any())
    x16, w16 = r16(x, bf16), r16(w, bf16)
    conv, S = ref_fwd(x16, w16, 0), ref_fwd(x16.abs(), w16.abs(), 0)
    E = 2 * 9 * 16 * ((CIN + 15) // 16) * EPS * S
    for sc, sh, act in ((scale, shift, 0), (scale, shift, 2), (None, None, 2)):
        got = run_fwd(x, w, Cout, bf16, 0, epi=(sc, sh, act)).double()
        ref = _epi_ref(conv, sc, sh, act)
        if sc is None:
            bound = E                                                 # (ReLU is 1-Lipschitz and exact)
        else:
            Es = E * sc.double().abs().view(1, -1, 1, 1)
            bound = Es + EPS * (_epi_ref(conv, sc, sh, 0).abs() + Es)   # the fma rounds ONCE: half an ulp of the value it holds
        err = (got - ref).abs()
        assert bool((err <= bound).all()), (act, sc is None, float((err / bound.clamp_min(1e-300)).max()))


@gpu
def test_epilogue_refused_combinations_write_nothing():
    """exactly one of scale / shift, and act = 1, are errors; a refused call leaves the output untouched"""
    B, Cout, W = 2, 24, 8
    g = torch.Generator().manual_seed(11)
    x, w = torch.randn((B, CIN, W, W), generator=g), torch.randn((Cout, CIN, 3, 3), generator=g)
    v = torch.ones(Cout)
    for epi in ((v, None, 2), (None, v, 2), (v, None, 0), (v, v, 1), (None, None, 1)):
        run_fwd(x, w, Cout, 0, 0, epi=epi, refused=True)


# ---- (d) weight gradient ------------------------------------------------------------------------------------------------------------------
def run_wgrad(x, dy):
    """one srbh_dconv_wgrad call on guarded buffers with a NaN-filled workspace -> dW on the host"""
    _lib, L = _L()
    B, Cin, W = x.shape[0], x.shape[1], x.shape[3]
    Cout = dy.shape[1]
    mo, nsplit = wgrad_plan(B, Cin, Cout, W)
    nws = L.srbh_dconv_wgrad_ws_floats(B, Cin, Cout, W, W)
    assert nws == nsplit * ((Cout + 16 * mo - 1) // (16 * mo)) * ((Cin + 15) // 16) * mo * 9 * 256
    g = GuardedBuffers()
    xd, dyd = g.inp(x), g.inp(dy)
    ws = g.out((nws,))                    # guard storage: NaN in every slot ("partials in fixed slots, nothing to zero")
    dw = g.out((Cout, Cin, 3, 3))
    assert bool(ws.isnan().all())
    _lib.check(L.srbh_dconv_wgrad(xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), ws.data_ptr(), B, Cin, Cout, W, W, _lib.stream_ptr()), "dconv_wgrad")
    g.verify()
    return dw.cpu()


def ref_wgrad(x64, dy64):
    return torch.nn.grad.conv2d_weight(x64, (dy64.shape[1], x64.shape[1], 3, 3), dy64, padding=1)


@gpu
@pytest.mark.parametrize("W,mo", sorted(WGRAD_FORMS))
def test_wgrad_form(W, mo):
    """every (plane size, MO) form: integer operands exact (B * W * W * 9 < 2^24), randn operands within 2 n 2^-24 S element by element
    (n = B * W * W, S = the weight gradient of the absolute bf16 operands) and within the module's norm bound; NaN in the workspace does not
    reach the result; a second call gives the same bits (fixed summation order)"""
    B, Cin, Cout, want_split = WGRAD_FORMS[(W, mo)]
    got_mo, nsplit = wgrad_plan(B, Cin, Cout, W)
    assert got_mo == mo and (want_split is None or nsplit == want_split), (got_mo, nsplit)
    steps = B * W * W // 16
    if want_split == 1:
        assert steps < 4                      # some of the four waves have an empty range
    if want_split == 7:
        assert steps % (4 * nsplit) != 0      # the last wave's range is short
    g = torch.Generator().manual_seed(13 + W + mo)
    x, dy = _ints((B, Cin, W, W), 3, g), _ints((B, Cout, W, W), 3, g)
    got = run_wgrad(x, dy)
    ref = ref_wgrad(x.double(), dy.double())
    assert float(ref.abs().max()) < 2 ** 24
    bad = (got.double() != ref).nonzero()
    assert torch.equal(got.double(), ref), (len(bad), bad[:8].tolist())
    x, dy = torch.randn((B, Cin, W, W), generator=g), torch.randn((B, Cout, W, W), generator=g)
    got = run_wgrad(x, dy)
    assert torch.equal(run_wgrad(x, dy).view(torch.int32), got.view(torch.int32))
    x16, dy16 = r16(x, 1), r16(dy, 1)
    ref, S = ref_wgrad(x16, dy16), ref_wgrad(x16.abs(), dy16.abs())
    bound = 2 * (B * W * W) * EPS * S
    err = (got.double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"\n[dconv wgrad form] W={W} MO={mo} nsplit={nsplit}: max err/bound = {ratio:.2e}, rel = {rel(got, ref):.3e}")
    assert bool((err <= bound).all()), ratio
    assert rel(got, ref) <= 5e-6


# ---- (e) production census (no kernel launch, no device) ----------------------------------------------------------------------------------
def test_production_shapes_select_covered_forms():
    """the ten decoder convolutions, forward and data gradient, at the batch sizes the project runs: every form the planning rule selects
    is one that the tables above compare with a reference -- a later change of the rule that moves production onto another form fails here"""
    from srbh_amd import _lib
    _lib.build()
    fwd, wg, splits = set(), set(), set()
    for B in PRODUCTION_B:
        for Cin, Cout, W in DECODER:
            fwd.add((W,) + fwd_plan(B, Cout, W))               # forward: fp16
            fwd.add((W,) + fwd_plan(B, Cin, W))                # data gradient: the same kernel, its Cout is the forward Cin
            mo, ns = wgrad_plan(B, Cin, Cout, W)
            wg.add((W, mo))
            splits.add(ns)
    assert fwd <= set(FWD_FORMS), fwd - set(FWD_FORMS)
    assert wg <= set(WGRAD_FORMS), wg - set(WGRAD_FORMS)
    assert any(npx == 256 for _, npx, _ in fwd) and max(splits) == 512      # (what the tables were built for is still what production runs)
    # the queries refuse what the convs refuse, and store nothing then
    L = _lib.lib()
    a, b = C.c_int(-7), C.c_int(-7)
    assert L.srbh_dconv_fwd_plan(4, 16, 12, C.byref(a), C.byref(b)) != 0 and L.srbh_dconv_fwd_plan(0, 16, 8, C.byref(a), C.byref(b)) != 0
    assert L.srbh_dconv_wgrad_plan(4, 16, 16, 128, C.byref(a), C.byref(b)) != 0 and L.srbh_dconv_fwd_plan(4, 16, 8, None, C.byref(b)) != 0
    assert (a.value, b.value) == (-7, -7)
