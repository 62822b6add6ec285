"""GPU: every kernel form behind the pointwise-convolution entry points (csrc/srbh_pwconv.hip, csrc/srbh_pwgemm_lds_kernel.h) against the
float64 oracle of tests/pwconv_oracle.py, element by element, through the C ABI on gpu_util.GuardedBuffers.

The launchers pick the form from the shape alone, so every case first ASKS the library (srbh_pwconv_gemm_plan / srbh_pwconv_wgrad_plan: the
launchers' own rule) which form its shape runs; tests/test_pwconv_oracle_cpu.py asserts that every form the EfficientNet-B4 encoder selects
at B = 32 ... 256 is a key of GEMM_FORMS / WGRAD_FORMS below.

Per case: integer operands from [-8, 8] with pairwise different images, channels and pixels, every partial sum below 2^24 -> torch.equal
with the oracle whatever the summation order (index map, ragged tiles, K remainders, stale workspace slots); Gaussian operands (w / sqrt(K))
within (K + F) 2^-23 sum|a||b| at EVERY element, F = the further roundings of the path: the kw-fold (kw), the nsplit reduce (nsplit), 1 for
the gate product, 1 each for the fmaf and the sum with res.  Outputs and the weight-gradient workspace are carved from NaN storage with
guards on either side; verify() after every call (guards intact, inputs unchanged, every output element written, none NaN).

SiLU (act = 1): the kernels compute v / (1 + __expf(-v)); its error has no derivation here, so it is measured: over all act = 1 cases the
largest |kernel - silu64(v)| / (2^-23 |silu64(v)|), v = the kernel's OWN fp32 pre-activation (the same call with act = 0, bit-reproducible),
so that the figure is the activation's alone.  C_SILU = the next power of two at or above twice that.  Integer operands with act = 1 cannot
be bit-equal; their pre-activation is exact and reaches thousands, and the bound there is (C_SILU + |v|) 2^-23 |silu| (pwconv_oracle.epi_bound).
Measured on an MI355X: see MEASURED below (4.19; the stock F.silu chain 1.31).

Determinism: every Gaussian case runs srbh_pwconv_fwd twice and the weight gradient twice: bit-equal.  srbh_pwconv_fwd, _fwd_wt and
_bwd_data of one case are asserted bit-equal to each other: the plan is a function of (M, K, HW, B) alone, so the three always run the same
form and kw and walk K in the same order; there is no case where the forms differ, hence none left unasserted.  (_fwd_epi and _bwd_data_res
run the EPI instantiation of the same form; without any epilogue part _fwd_epi is asserted bit-equal to _fwd as well.)

Not covered: the SRBH_PW_LDS / SRBH_PW_LDS_MINN overrides, SRBH_PW_UK other than 8, pointers that are not 16-byte aligned.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import pwconv_oracle as O
from tests.gpu_util import GuardedBuffers

gpu = pytest.mark.gpu
DEV = "cuda:0"
U = O.U

# MEASURED on an MI355X (the shapes and seeds below; `pytest -s` prints every figure).  Largest err / bound over the Gaussian cases:
#   srbh_pwconv_fwd, _fwd_wt, _bwd_data  0.342   (99, 5, 16, 440): K = 5, 1.7 units of 2^-23 S
#   srbh_pwconv_bwd_data_res             0.274
#   srbh_pwconv_fwd_epi                  0.342   (the empty epilogue, the same bits as _fwd); integer operands with SiLU: 0.136 of their bound
#   srbh_pwconv_bwd_weight               0.044   (19, 37, 3, 4): K = 12; 3e-6 at K = 20 000
# SiLU alone, in units of 2^-23 |silu|, worst over the 24 Gaussian act = 1 cases (|v| up to 11.6): kernel 4.19 at (448, 132, 4, 1536), the stock
# F.silu on the same pre-activations 1.31; integer operands (|v| up to 27 028): kernel 28.4, stock 0.84.  C_SILU = 16 >= 2 * 4.19.
C_SILU = 16.0
WORST = {}          # entry point -> largest err / bound this session (printed beside every figure)

# ---- forward / data gradient: (family, form, kw) -> [(M, K, HW, B)].  family 0: pw_gemm_kernel, form = tile 0 16x16 | 1 16x32 | 2 32x32;
# family 1: pw_gemm_lds_kernel, form 1 64x64 | 2 64x128 | 4 32x128
GEMM_FORMS = {
    (0, 0, 1): [(5, 3, 1, 1), (19, 7, 9, 3), (19, 64, 4, 9), (99, 261, 16, 250)],          # planes straddling a 16-column tile; a deep K on one wave
    (0, 0, 4): [(19, 69, 4, 9), (37, 256, 16, 2), (160, 960, 16, 128), (160, 128, 16, 64)],  # the last two: multiples of 4 the LDS plan declines
    (0, 0, 16): [(17, 261, 4, 3), (35, 320, 16, 1), (21, 2688, 4, 2), (21, 263, 9, 5)],    # one wave with 1 element of K and two with none; a ragged gate run
    (0, 1, 1): [(99, 5, 16, 440), (640, 128, 16, 148)],
    (0, 2, 1): [(99, 5, 16, 768), (1536, 8, 16, 63), (99, 7, 9, 1366)],
    (1, 4, 1): [(24, 4, 4, 257), (4, 8, 16, 65)],                                         # K below one K block; 9 tiles over 8 XCD runs
    (1, 1, 1): [(36, 20, 16, 65), (68, 56, 4, 300), (448, 132, 4, 1536)],                 # ragged last column tile; K no multiple of 16
    (1, 2, 1): [(2020, 8, 16, 250), (2020, 8, 4, 1000)],                                  # ragged M tile and ragged column tile
}
# ---- weight gradient: (vec, kw) -> [((Cout, Cin, B, HW), nsplit)]
WGRAD_FORMS = {
    (1, 4): [((19, 37, 3, 4), 1), ((512, 512, 64, 4), 2)],
    (1, 16): [((19, 37, 16, 4), 1), ((19, 37, 130, 4), 2), ((19, 37, 200, 4), 3), ((16, 16, 4096, 4), 64), ((16, 16, 5000, 4), 64)],
    (4, 4): [((37, 19, 5, 16), 1), ((37, 19, 9, 64), 2), ((144, 24, 5, 256), 5), ((24, 48, 4, 1024), 16)],
    (4, 16): [((33, 17, 70, 16), 1), ((17, 33, 129, 16), 2)],
}
COVERED_GEMM, COVERED_WGRAD = frozenset(GEMM_FORMS), frozenset(WGRAD_FORMS)
assert all(8 * 8 * 8 * K * 8 + 8 < 2 ** 24 for v in GEMM_FORMS.values() for (_, K, _, _) in v)        # gated product times scale plus shift: exact
assert all(64 * B * HW < 2 ** 24 for v in WGRAD_FORMS.values() for ((_, _, B, HW), _) in v)
# (gate, scale / shift, res, act): the five combinations of tests/test_gpu_dwconv.py
EPI_COMBOS = ((1, 1, 1, 0), (1, 1, 0, 0), (0, 1, 0, 1), (0, 0, 0, 0), (1, 0, 1, 2))


def _L():
    from srbh_amd import _lib
    return _lib, _lib.lib()


def gemm_plan(M, K, HW, B):
    """(family, form, kw) of the forward (M = Cout, K = Cin) or the data gradient (M = Cin, K = Cout); host only"""
    _lib, L = _L()
    a, b, c = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    _lib.check(L.srbh_pwconv_gemm_plan(B, M, K, HW, C.byref(a), C.byref(b), C.byref(c)), "pwconv_gemm_plan")
    return a.value, b.value, c.value


def wgrad_plan(Cout, Cin, B, HW):
    """(vec, kw, nsplit) of the weight gradient; host only"""
    _lib, L = _L()
    a, b, c = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    _lib.check(L.srbh_pwconv_wgrad_plan(B, Cin, Cout, HW, C.byref(a), C.byref(b), C.byref(c)), "pwconv_wgrad_plan")
    return a.value, b.value, c.value


def _ptr(t):
    return None if t is None else t.data_ptr()


class _Case:
    """the device operands of one (shape, kind), uploaded once and shared by every call; each call gets fresh NaN-carved outputs"""

    def __init__(self, ops):
        self.base = GuardedBuffers()
        self.h = ops
        self.d = {k: self.base.inp(v) for k, v in ops.items()}

    def call(self, fn, out_shape, refused=False):
        """fn(out) -> rc.  Returns the output (on the device) after verify()"""
        _lib, _ = _L()
        g = GuardedBuffers()
        g.inputs = self.base.inputs
        y = g.out(out_shape)
        rc = fn(y)
        if refused:
            assert rc != 0, "the call should have been refused"
            g.verify(written=False)
            return None
        _lib.check(rc, "pwconv")
        g.verify()
        return y


def _compare(name, shape, got, ref, bound):
    """every element within its bound (float64, on the device); prints the largest err / bound"""
    ref, bound = ref.to(DEV), bound.to(DEV)
    err = (got.double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    entry = name.split("(")[0].split(" ")[0]
    WORST[entry] = max(WORST.get(entry, 0.0), ratio)
    print(f"[pwconv forms] {name} {shape}: max err/bound = {ratio:.3e} (srbh_pwconv_{entry} so far: {WORST[entry]:.3e})")
    assert bool((err <= bound).all()), (name, shape, ratio)
    return ratio


def _exact(name, shape, got, ref):
    ref = ref.to(DEV)
    assert float(ref.abs().max()) < 2 ** 24
    if not torch.equal(got.double(), ref):
        bad = (got.double() != ref).nonzero()
        raise AssertionError((name, shape, len(bad), bad[:8].tolist()))


def _bits(t):
    return t.view(torch.int32)


GEMM_CASES = [pytest.param(key, shape, kind, id=f"f{key[0]}-form{key[1]}-kw{key[2]}-{'x'.join(map(str, shape))}-{kind}")
              for key in GEMM_FORMS for shape in GEMM_FORMS[key] for kind in ("int", "randn")]
assert len(GEMM_CASES) == 48


def _gemm_calls(case, M, K, HW, B):
    """the entry points of one case as closures over the device operands.  The forward has w = a [M = Cout][K = Cin]; the data gradient has
    w = a^T [K = Cout][M = Cin], which is also the forward's W^T"""
    _lib, L = _L()
    d, st = case.d, _lib.stream_ptr()
    inp, a, at = d["inp"].data_ptr(), d["a"].data_ptr(), d["at"].data_ptr()
    shape = (B, M, HW)

    def epi(combo, transposed, act=None):
        ug, ub, ur, ac = combo
        ac = ac if act is None else act
        return case.call(lambda y: L.srbh_pwconv_fwd_epi(inp, at if transposed else a, transposed, y.data_ptr(), B, K, M, HW, _ptr(d["gate"]) if ug else None,
                                                         _ptr(d["scale"]) if ub else None, _ptr(d["shift"]) if ub else None,
                                                         _ptr(d["res"]) if ur else None, ac, st), shape)
    return {
        "fwd": lambda: case.call(lambda y: L.srbh_pwconv_fwd(inp, a, y.data_ptr(), B, K, M, HW, st), shape),
        "fwd_wt": lambda: case.call(lambda y: L.srbh_pwconv_fwd_wt(inp, at, y.data_ptr(), B, K, M, HW, st), shape),
        "bwd_data": lambda: case.call(lambda y: L.srbh_pwconv_bwd_data(inp, at, y.data_ptr(), B, M, K, HW, st), shape),
        "bwd_data_res": lambda: case.call(lambda y: L.srbh_pwconv_bwd_data_res(inp, at, d["res"].data_ptr(), y.data_ptr(), B, M, K, HW, st), shape),
        "epi": epi,
    }


@gpu
@pytest.mark.parametrize("key,shape,kind", GEMM_CASES)
def test_gemm_form(key, shape, kind):
    """srbh_pwconv_fwd, _fwd_wt, _bwd_data, _bwd_data_res and the five epilogue combinations of _fwd_epi (W and W^T) at one shape of one
    form: the plan query names the form; integer operands exact, Gaussian operands within the element-wise bound; the three plain products
    bit-equal to each other and to a second call"""
    M, K, HW, B = shape
    assert gemm_plan(M, K, HW, B) == key, (gemm_plan(M, K, HW, B), "the shape no longer selects the form it is here for")
    kw = key[2]
    fold = kw if kw > 1 else 0
    ops = O.gemm_operands(M, K, HW, B, kind)
    ops["at"] = ops["a"].t().contiguous()
    case = _Case(ops)
    call = _gemm_calls(case, M, K, HW, B)
    exact = kind == "int"
    # ---- the plain products: one reference from the forward's definition, one from the data gradient's
    y_ref, y_S = O.fwd(ops["inp"], ops["a"])
    dx_ref, dx_S = O.bwd_data(ops["inp"], ops["at"])
    got = {n: call[n]() for n in ("fwd", "fwd_wt", "bwd_data")}
    for n, (ref, S) in (("fwd", (y_ref, y_S)), ("fwd_wt", (y_ref, y_S)), ("bwd_data", (dx_ref, dx_S))):
        if exact:
            _exact(n, shape, got[n], ref)
        else:
            _compare(n, shape, got[n], ref, (K + fold) * U * S)
    assert torch.equal(_bits(got["fwd"]), _bits(got["fwd_wt"])) and torch.equal(_bits(got["fwd"]), _bits(got["bwd_data"])), "same form, same K order"
    if not exact:
        assert torch.equal(_bits(call["fwd"]()), _bits(got["fwd"])), "a second call gave other bits"
    dxr_ref, dxr_S = O.bwd_data(ops["inp"], ops["at"], ops["res"])
    g = call["bwd_data_res"]()
    if exact:
        _exact("bwd_data_res", shape, g, dxr_ref)
    else:
        _compare("bwd_data_res", shape, g, dxr_ref, (K + fold + 1) * U * dxr_S)
    # ---- the epilogue
    product = {0: (y_ref, y_S), 1: O.fwd(ops["inp"], ops["a"], ops["gate"])}
    for combo in EPI_COMBOS:
        ug, ub, ur, act = combo
        o = O.fwd_epi(ops["inp"], ops["a"], ops["gate"] if ug else None, ops["scale"] if ub else None, ops["shift"] if ub else None,
                      ops["res"] if ur else None, act, product=product[ug])
        bound = O.epi_bound(o, K, fold + ug + ub, ops["res"] if ur else None, act, C_SILU, exact_pre=exact)
        outs = [call["epi"](combo, t) for t in (0, 1)]
        assert torch.equal(_bits(outs[0]), _bits(outs[1])), ("W and W^T: same form, same K order", combo)
        if exact and act != 1:
            _exact(f"fwd_epi{combo}", shape, outs[0], o["y"])
        else:
            _compare(f"fwd_epi{combo}{' exact-pre' if exact else ''}", shape, outs[0], o["y"], bound)
        if combo == (0, 0, 0, 0):
            assert torch.equal(_bits(outs[0]), _bits(got["fwd"])), "the empty epilogue is the plain forward"
        if act == 1:
            # the activation alone: the kernel's own pre-activation (same call, act = 0) through float64 SiLU and through the stock fp32 one
            v = call["epi"](combo, 0, act=0)
            s64 = O.silu(v.double().cpu())
            unit = (U * s64.abs()).clamp_min(1e-300)
            big = s64.abs() > 2.0 ** -100          # (below: the fp32 underflow floor, not the activation's relative error)
            ours = float((((outs[0].double().cpu() - s64).abs() / unit)[big]).max()) if bool(big.any()) else 0.0
            stock = float((((F.silu(v).double().cpu() - s64).abs() / unit)[big]).max()) if bool(big.any()) else 0.0
            print(f"[pwconv forms] silu-only {kind} {shape}: kernel {ours:.3f}, stock F.silu {stock:.3f} (units of 2^-23 |silu|), max |v| = {float(v.abs().max()):.1f}")
            if not exact:
                assert ours <= C_SILU / 2, (ours, "C_SILU is no longer twice the measured SiLU error")


WGRAD_CASES = [pytest.param(key, shape, ns, id=f"vec{key[0]}-kw{key[1]}-{'x'.join(map(str, shape))}-ns{ns}")
               for key in WGRAD_FORMS for shape, ns in WGRAD_FORMS[key]]
assert len(WGRAD_CASES) == 13


def _run_wgrad(ops, Cout, Cin, B, HW, null_ws=False):
    _lib, L = _L()
    nws = L.srbh_pwconv_bwd_weight_ws_floats(B, Cin, Cout, HW)
    g = GuardedBuffers()
    x, dy = g.inp(ops["x"]), g.inp(ops["dy"])
    ws = g.out((nws,)) if nws else None          # exactly the floats asked for, NaN in every slot
    dw = g.out((Cout, Cin))
    rc = L.srbh_pwconv_bwd_weight(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), None if null_ws else _ptr(ws), B, Cin, Cout, HW, _lib.stream_ptr())
    if null_ws:
        assert rc != 0, "a split weight gradient without its workspace should be refused"
        g.verify(written=False)
        return None
    _lib.check(rc, "pwconv_bwd_weight")
    g.verify()
    return dw


@gpu
@pytest.mark.parametrize("key,shape,nsplit", WGRAD_CASES)
def test_wgrad_form(key, shape, nsplit):
    """srbh_pwconv_bwd_weight at one shape of one (vec, kw) form and split count: integer operands exact, Gaussian operands within
    (B HW + kw + nsplit) 2^-23 S at every element, two calls bit-equal, the workspace exactly as large as asked for and NaN before the call,
    and (nsplit > 1) a null workspace refused with nothing written"""
    _lib, L = _L()
    Cout, Cin, B, HW = shape
    assert wgrad_plan(Cout, Cin, B, HW) == key + (nsplit,), (wgrad_plan(Cout, Cin, B, HW), "the shape no longer selects the form it is here for")
    nws = L.srbh_pwconv_bwd_weight_ws_floats(B, Cin, Cout, HW)
    assert nws == (nsplit * Cout * Cin if nsplit > 1 else 0) and (nws == 0) == (nsplit == 1)
    ops = O.wgrad_operands(Cout, Cin, B, HW, "int")
    ref, _ = O.bwd_weight(ops["x"], ops["dy"])
    _exact("bwd_weight", shape, _run_wgrad(ops, Cout, Cin, B, HW), ref)
    ops = O.wgrad_operands(Cout, Cin, B, HW, "randn")
    ref, S = O.bwd_weight(ops["x"], ops["dy"])
    got = _run_wgrad(ops, Cout, Cin, B, HW)
    _compare("bwd_weight", shape, got, ref, (B * HW + key[1] + nsplit) * U * S)
    assert torch.equal(_bits(_run_wgrad(ops, Cout, Cin, B, HW)), _bits(got)), "a second call gave other bits"
    if nsplit > 1:
        _run_wgrad(ops, Cout, Cin, B, HW, null_ws=True)


# ---- srbh_transpose_many -------------------------------------------------------------------------------------------------------------------
def _transpose_table(g, mats):
    import numpy as np
    src = [g.inp(m) for m in mats]
    dst = [g.out((m.shape[1], m.shape[0])) for m in mats]
    desc = np.zeros(len(mats), dtype=np.dtype([("src", "<u8"), ("dst", "<u8"), ("rows", "<i4"), ("cols", "<i4")]))
    for i, m in enumerate(mats):
        desc[i] = (src[i].data_ptr(), dst[i].data_ptr(), m.shape[0], m.shape[1])
    return src, dst, g.inp(torch.from_numpy(desc.view(np.uint8).copy()), dtype=torch.uint8)


@gpu
@pytest.mark.parametrize("sizes", [[(1, 1), (1, 37), (37, 1), (31, 33), (32, 32), (65, 100), (530, 520)], [(31, 33)]], ids=["table7", "table1"])
def test_transpose_many(sizes):
    """one table, one launch: every result bit-equal to .t(), guards intact, sources unchanged; 530x520 has 289 tiles of 32x32, more than
    the 256 workgroups the grid has along x; and a table of one"""
    _lib, L = _L()
    gen = torch.Generator().manual_seed(17)
    mats = [torch.randn(s, generator=gen) for s in sizes]
    assert sizes == [(31, 33)] or ((530 + 31) // 32) * ((520 + 31) // 32) == 289
    g = GuardedBuffers()
    src, dst, table = _transpose_table(g, mats)
    _lib.check(L.srbh_transpose_many(table.data_ptr(), len(mats), _lib.stream_ptr()), "transpose_many")
    g.verify()
    for m, d in zip(mats, dst):
        assert torch.equal(_bits(d.cpu()), _bits(m.t().contiguous())), tuple(m.shape)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_refused_calls_write_nothing():
    """every SRBH_REQUIRE of these entry points: a null pointer, a zero dimension, HW = 9 for the weight gradient, one of scale / shift
    without the other, act = 3 (and -1), n = 0 and n = 65536 for the transpose, a null table; non-zero return and no output element written"""
    _lib, L = _L()
    st = _lib.stream_ptr()
    M, K, HW, B = 19, 7, 9, 3
    ops = O.gemm_operands(M, K, HW, B, "randn")
    ops["at"] = ops["a"].t().contiguous()
    case = _Case(ops)
    d = case.d
    inp, a, at, res, gate, sc, sh = (d[k].data_ptr() for k in ("inp", "a", "at", "res", "gate", "scale", "shift"))
    shape = (B, M, HW)
    dims = [(0, K, M, HW), (B, 0, M, HW), (B, K, 0, HW), (B, K, M, 0), (-1, K, M, HW)]
    for fn, w in ((L.srbh_pwconv_fwd, a), (L.srbh_pwconv_fwd_wt, at)):
        case.call(lambda y: fn(None, w, y.data_ptr(), B, K, M, HW, st), shape, refused=True)
        case.call(lambda y: fn(inp, None, y.data_ptr(), B, K, M, HW, st), shape, refused=True)
        assert fn(inp, w, None, B, K, M, HW, st) != 0
        for b_, k_, m_, hw_ in dims:
            case.call(lambda y: fn(inp, w, y.data_ptr(), b_, k_, m_, hw_, st), shape, refused=True)
    # data gradient: Cin = M, Cout = K
    case.call(lambda y: L.srbh_pwconv_bwd_data(None, at, y.data_ptr(), B, M, K, HW, st), shape, refused=True)
    case.call(lambda y: L.srbh_pwconv_bwd_data(inp, None, y.data_ptr(), B, M, K, HW, st), shape, refused=True)
    assert L.srbh_pwconv_bwd_data(inp, at, None, B, M, K, HW, st) != 0
    case.call(lambda y: L.srbh_pwconv_bwd_data_res(None, at, res, y.data_ptr(), B, M, K, HW, st), shape, refused=True)
    case.call(lambda y: L.srbh_pwconv_bwd_data_res(inp, None, res, y.data_ptr(), B, M, K, HW, st), shape, refused=True)
    case.call(lambda y: L.srbh_pwconv_bwd_data_res(inp, at, None, y.data_ptr(), B, M, K, HW, st), shape, refused=True)
    assert L.srbh_pwconv_bwd_data_res(inp, at, res, None, B, M, K, HW, st) != 0
    for b_, k_, m_, hw_ in dims:
        case.call(lambda y: L.srbh_pwconv_bwd_data(inp, at, y.data_ptr(), b_, m_, k_, hw_, st), shape, refused=True)
        case.call(lambda y: L.srbh_pwconv_bwd_data_res(inp, at, res, y.data_ptr(), b_, m_, k_, hw_, st), shape, refused=True)
    # epilogue
    def epi(y, x_=inp, w_=a, dims_=(B, K, M, HW), g_=gate, sc_=sc, sh_=sh, r_=res, act=0):
        return L.srbh_pwconv_fwd_epi(x_, w_, 0, y.data_ptr(), *dims_, g_, sc_, sh_, r_, act, st)
    case.call(lambda y: epi(y, x_=None), shape, refused=True)
    case.call(lambda y: epi(y, w_=None), shape, refused=True)
    assert L.srbh_pwconv_fwd_epi(inp, a, 0, None, B, K, M, HW, gate, sc, sh, res, 0, st) != 0
    for dm in dims:
        case.call(lambda y: epi(y, dims_=dm), shape, refused=True)
    case.call(lambda y: epi(y, sc_=None), shape, refused=True)
    case.call(lambda y: epi(y, sh_=None), shape, refused=True)
    case.call(lambda y: epi(y, act=3), shape, refused=True)
    case.call(lambda y: epi(y, act=-1), shape, refused=True)
    # weight gradient
    Cout, Cin, Bw, HWw = 19, 37, 3, 4
    wo = O.wgrad_operands(Cout, Cin, Bw, HWw, "randn")
    g = GuardedBuffers()
    x, dy = g.inp(wo["x"]), g.inp(wo["dy"])
    dw, ws = g.out((Cout, Cin)), g.out((64,))
    bw = L.srbh_pwconv_bwd_weight
    assert bw(None, dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), Bw, Cin, Cout, HWw, st) != 0
    assert bw(x.data_ptr(), None, dw.data_ptr(), ws.data_ptr(), Bw, Cin, Cout, HWw, st) != 0
    assert bw(x.data_ptr(), dy.data_ptr(), None, ws.data_ptr(), Bw, Cin, Cout, HWw, st) != 0
    for b_, ci_, co_, hw_ in ((0, Cin, Cout, HWw), (Bw, 0, Cout, HWw), (Bw, Cin, 0, HWw), (Bw, Cin, Cout, 0), (Bw, Cin, Cout, 9), (Bw, Cin, Cout, 8),
                              (Bw, Cin, Cout, 24)):
        assert bw(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), b_, ci_, co_, hw_, st) != 0, (b_, ci_, co_, hw_)
    g.verify(written=False)
    # transpose
    g = GuardedBuffers()
    _, _, table = _transpose_table(g, [torch.randn((5, 3), generator=torch.Generator().manual_seed(3))])
    assert L.srbh_transpose_many(None, 1, st) != 0
    assert L.srbh_transpose_many(table.data_ptr(), 0, st) != 0 and L.srbh_transpose_many(table.data_ptr(), -1, st) != 0
    assert L.srbh_transpose_many(table.data_ptr(), 65536, st) != 0
    g.verify(written=False)
    plan_queries_refuse()


def plan_queries_refuse():
    """the plan queries' own refusals: a null pointer, a dimension <= 0, a weight-gradient plane the kernel does not take; nothing stored
    (host only: tests/test_pwconv_oracle_cpu.py runs this too)"""
    _, L = _L()
    v = [C.c_int(-7) for _ in range(3)]
    p = [C.byref(t) for t in v]
    gp, wp = L.srbh_pwconv_gemm_plan, L.srbh_pwconv_wgrad_plan
    for i in range(3):
        q = list(p)
        q[i] = None
        assert gp(4, 16, 16, 4, *q) != 0 and wp(4, 16, 16, 4, *q) != 0
    for dm in ((0, 16, 16, 4), (4, 0, 16, 4), (4, 16, 0, 4), (4, 16, 16, 0), (-1, 16, 16, 4)):
        assert gp(*dm, *p) != 0 and wp(*dm, *p) != 0, dm
    for hw in (9, 8, 24, 1):
        assert wp(4, 16, 16, hw, *p) != 0, hw
    assert [t.value for t in v] == [-7, -7, -7]
    assert gp(4, 16, 16, 9, *p) == 0 and [t.value for t in v] == [0, 0, 1]          # (the forward and the data gradient take any plane)
