"""The loader's plain kernels (csrc/srbh_loader.hip: srbh_label_prep, srbh_normalize_clamp) -- they feed every training and inference tile,
and tests/test_gpu_augment.py and tests/test_gpu_grid_tiles.py use them as the expected value -- each on its own through the C ABI against
oracle/loader_oracle.py (batched in tests/io_ends_oracle.py), bit for bit and with no allowance: a cell's sum of 16 uint8 labels is an
integer <= 4080, exact in fp32 in any order, and fl32(16 + 1e-10) is 16, so the aggregates are exact; (x - min) / range is two correctly
rounded fp32 operations (the build carries no fast-math flag), so the normalised tile equals the IEEE value, compared through an integer
view: the sign of zero and the bits of a NaN count.  Every output lives in guard-filled storage, every input is compared with its clone
afterwards (tests/gpu_util.GuardedBuffers).  tests/test_io_ends_cpu.py proves that the tables reach the forms named here.

  label_prep   (B, H, W) = (1, 4, 4), (3, 8, 12), (2, 20, 36) -- multiples of 4 but not of 8 --, (5, 64, 68) = 1360 cells: several workgroups and
               a ragged last one; every label 0..255, cells whose sum is a multiple of 16 and one below it at every class edge (the
               truncation decides weight_aggre), an image of 255s; hir ending in 255 (label 255 in no class) and in 256; class weights
               that are arbitrary bit patterns (negative, subnormal, not bf16-representable); outputs off a 16-byte boundary; refusals:
               H or W not a multiple of 4, a zero dimension, a null pointer for each argument, a misaligned `height`; LabelPrep on a view
               that starts at an odd byte.
  normalize    (B, C, H, W) = (3, 5, 1, 1) -- hw == 1 --, (2, 8, 7, 9), (1, 1, 16, 16), (1, 3, 600, 600) = 1 080 000 elements: a second
               grid-stride trip with a ragged end; clip to (0, 1), (-1, 1), (0.25, 0.75) and none; inputs exactly on lo and hi and one ulp
               either side, -0.0, +-inf, NaN, a subnormal result, a band of range 0 (+-inf and NaN before the clip); refusals.

Measured on an MI355X: exact everywhere -- all five outputs of label_prep in all 12 cases and through LabelPrep on five views, and every bit of the normalised tiles in all 16
cases: -0.0 stays -0.0, 0 / 0 of the zero range is 0xffc00000 on the device as on the host, a NaN input keeps its bits (0x7fc00000),
subnormal results are not flushed.  Nothing was found wrong in the kernels' values; the one change is the alignment requirement on `height`.

Mutation check (scratch builds of the kernel with one change each, never committed; "older" = tests/test_loader_math.py as tightened here):
  `(int)rintf(ha)` for `(int)ha` in label_prep        test_label_prep (8: the three larger shapes and the one-below cell, under either hir),
                                                      test_label_prep_wrapper_on_a_view_at_any_byte (5); the older file catches it (both
                                                      tests, before the tightening too: weight_aggre changes in far more than 1 % of the cells)
  `v <= lo ? lo` in the clip (the sign of zero)       test_normalize_clamp[(0, 1)] at 3x5x1x1, 2x8x7x9 and 1x3x600x600 (the shapes with the
                                                      identity band), test_normalize_tiles_wrapper_equals_the_entry; the older file passes,
                                                      before and after the tightening (its inputs hold no -0.0)
  hi and lo swapped for the upper bound               test_normalize_clamp (all 12 with a clip), test_normalize_tiles_wrapper_equals_the_entry;
                                                      the older file catches it (both tests, before the tightening too)"""
import numpy as np
import pytest
import torch

from tests import io_ends_oracle as O
from tests.gpu_util import GuardedBuffers as Buffers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib():
    from srbh_amd import _lib as m
    return m, m.lib()


def _p(t):
    return None if t is None else t.data_ptr()


def _same_bits(what, got, want):
    g, w = O.bits(got), O.bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    msg = ""
    if bad.any():
        i = int(np.flatnonzero(bad.reshape(-1))[0])
        msg = f" (first at {i}: got {int(g.reshape(-1)[i]) & 0xffffffff:#010x} want {int(w.reshape(-1)[i]) & 0xffffffff:#010x})"
    print(f"IOENDS {what}: {int(bad.sum())} of {g.size} differ{msg}")
    assert not bad.any(), what


def _refused(rc, bufs, name):
    _, L = _lib()
    assert rc != 0, f"{name}: accepted"
    bufs.verify(written=False)
    assert name.encode() in L.srbh_last_error(), L.srbh_last_error()


# ---- srbh_label_prep ----------------------------------------------------------------------------------------------------------------------------
class _Prep:
    def __init__(self, lab, hir, height_offset=0):
        from oracle.loader_oracle import buildhir_lut
        self.bufs = b = Buffers()
        self.shape = B, H, W = lab.shape
        self.height = b.inp(torch.from_numpy(lab), offset=height_offset, dtype=torch.uint8)
        self.lut = b.inp(torch.from_numpy(buildhir_lut(hir)), offset=1, dtype=torch.uint8)
        self.cw = b.inp(torch.from_numpy(O.CLASS_WEIGHTS), offset=1)
        self.build = b.out((B, H, W), offset=1, dtype=torch.int64)
        self.hf, self.wt = b.out((B, H, W), offset=1), b.out((B, H, W), offset=3)
        self.ha, self.wa = b.out((B, H // 4, W // 4), offset=1), b.out((B, H // 4, W // 4), offset=2)

    def args(self):
        m, _ = _lib()
        B, H, W = self.shape
        return [_p(self.height), B, H, W, _p(self.lut), _p(self.cw), _p(self.build), _p(self.hf), _p(self.wt), _p(self.ha), _p(self.wa),
                m.stream_ptr()]


_PREP_CASES = [(s, "mixed") for s in O.PREP_SHAPES] + [((1, 4, 4), "one_below"), ((1, 4, 4), "all255")]


@pytest.mark.parametrize("hir", [O.HIR256, O.HIR255], ids=["hir256", "hir255"])
@pytest.mark.parametrize("shape,kind", _PREP_CASES, ids=[f"{s[0]}x{s[1]}x{s[2]}-{k}" for s, k in _PREP_CASES])
def test_label_prep(shape, kind, hir):
    m, L = _lib()
    lab = O.prep_labels(shape, kind)
    p = _Prep(lab, hir)
    m.check(L.srbh_label_prep(*p.args()), "label_prep")
    p.bufs.verify()
    build, hf, wt, ha, wa = O.label_prep(lab, hir, O.CLASS_WEIGHTS)
    name = f"label_prep {shape} {kind} hir{hir[-1]}"
    bad = int((p.build.cpu() != build).sum())
    print(f"IOENDS {name} build: {bad} of {build.numel()} differ")
    assert bad == 0 and p.build.dtype == build.dtype
    _same_bits(f"{name} height", p.hf, hf)
    _same_bits(f"{name} weight", p.wt, wt)
    _same_bits(f"{name} height_aggre", p.ha, ha)
    _same_bits(f"{name} weight_aggre", p.wa, wa)


_PREP_ARG = ("height", "B", "H", "W", "buildhir_lut", "class_weight", "build", "height_f", "weight", "height_aggre", "weight_aggre")


@pytest.mark.parametrize("what", ["H=10", "W=6", "H=0", "W=0", "B=0"] + [f"{n}=null" for n in _PREP_ARG if len(n) > 1])
def test_label_prep_refusals(what):
    _, L = _lib()
    p = _Prep(O.prep_labels((3, 8, 12)), O.HIR256)
    args = p.args()
    name, val = what.split("=")
    args[_PREP_ARG.index(name)] = None if val == "null" else int(val)
    _refused(L.srbh_label_prep(*args), p.bufs, "srbh_label_prep")


@pytest.mark.parametrize("off", [1, 2, 3])
def test_label_prep_refuses_a_misaligned_height(off):
    """the kernel reads four labels at a time: a pointer that is not 4-byte aligned is refused, nothing is launched"""
    _, L = _lib()
    p = _Prep(O.prep_labels((3, 8, 12)), O.HIR256, height_offset=off)
    assert _p(p.height) % 4 == off
    _refused(L.srbh_label_prep(*p.args()), p.bufs, "srbh_label_prep")


@pytest.mark.parametrize("off", [0, 1, 2, 3, 4])
def test_label_prep_wrapper_on_a_view_at_any_byte(off):
    """LabelPrep takes a contiguous view as it is; one that starts at an odd byte is copied, never handed to the kernel"""
    from srbh_amd.loader_math import LabelPrep
    shape = (3, 8, 12)
    lab = O.prep_labels(shape)
    n = lab.size
    store = torch.full((n + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    view = store[off: off + n].view(shape)
    view.copy_(torch.from_numpy(lab))
    assert view.is_contiguous() and view.data_ptr() % 4 == off % 4
    keep = store.clone()
    prep = LabelPrep(O.HIR256, O.CLASS_WEIGHTS, DEV)
    hf, ha, build, wt, wa = prep(view)
    torch.cuda.synchronize()
    assert torch.equal(store, keep)
    wb, whf, wwt, wha, wwa = O.label_prep(lab, O.HIR256, O.CLASS_WEIGHTS)
    assert torch.equal(build.cpu(), wb)
    for name, g, w in (("height", hf, whf), ("weight", wt, wwt), ("height_aggre", ha, wha), ("weight_aggre", wa, wwa)):
        _same_bits(f"LabelPrep view+{off} {name}", g, w)


# ---- srbh_normalize_clamp ---------------------------------------------------------------------------------------------------------------------
class _Norm:
    def __init__(self, x, mins, ranges, clamp):
        self.bufs = b = Buffers()
        self.shape, self.clamp = x.shape, clamp
        self.src = b.inp(torch.from_numpy(x), offset=1)
        self.mins, self.ranges = b.inp(torch.from_numpy(mins), offset=1), b.inp(torch.from_numpy(ranges), offset=3)
        self.dst = b.out(x.shape, offset=3)

    def args(self):
        m, _ = _lib()
        lo, hi = self.clamp if self.clamp else (0.0, 0.0)
        return [_p(self.src), _p(self.dst), *self.shape, _p(self.mins), _p(self.ranges), float(lo), float(hi), int(self.clamp is not None),
                m.stream_ptr()]


def _verify_norm(n):
    """GuardedBuffers.verify, except that NaN is a value here: the input clones are compared as bits, the output is not asked to be NaN-free"""
    torch.cuda.synchronize()
    for v, c in n.bufs.inputs:
        assert torch.equal(v.view(torch.int32), c.view(torch.int32)), "an input was written"
    n.bufs.inputs = []
    buf, v = n.bufs.outputs[0]
    lo = (v.data_ptr() - buf.data_ptr()) // 4
    assert bool(buf[:lo].isnan().all()) and bool(buf[lo + v.numel():].isnan().all()), "a write outside the output"


@pytest.mark.parametrize("clamp", O.NORM_CLAMPS, ids=[str(c) for c in O.NORM_CLAMPS])
@pytest.mark.parametrize("shape", O.NORM_SHAPES, ids=["x".join(map(str, s)) for s in O.NORM_SHAPES])
def test_normalize_clamp(shape, clamp):
    m, L = _lib()
    x, mins, ranges = O.norm_inputs(shape, clamp)
    n = _Norm(x, mins, ranges, clamp)
    m.check(L.srbh_normalize_clamp(*n.args()), "normalize_clamp")
    _verify_norm(n)
    want = O.normalize(x, mins, ranges, clamp)
    got = n.dst.cpu()
    nan_w, nan_g = torch.isnan(want).numpy(), torch.isnan(got).numpy()
    print(f"IOENDS normalize {shape} {clamp}: NaN in want {int(nan_w.sum())}, in got {int(nan_g.sum())}; NaN bit patterns got "
          f"{sorted({hex(int(v) & 0xffffffff) for v in O.bits(got)[nan_g]})} want {sorted({hex(int(v) & 0xffffffff) for v in O.bits(want)[nan_w]})}")
    _same_bits(f"normalize {shape} {clamp}", got, want)


@pytest.mark.parametrize("what", ["B=0", "C=0", "H=0", "W=0", "src=null", "dst=null", "mins=null", "ranges=null"])
def test_normalize_clamp_refusals(what):
    _, L = _lib()
    x, mins, ranges = O.norm_inputs((2, 8, 7, 9), (0.0, 1.0))
    n = _Norm(x, mins, ranges, (0.0, 1.0))
    names = ("src", "dst", "B", "C", "H", "W", "mins", "ranges")
    args = n.args()
    name, val = what.split("=")
    args[names.index(name)] = None if val == "null" else int(val)
    assert L.srbh_normalize_clamp(*args) != 0
    assert b"srbh_normalize_clamp" in L.srbh_last_error()
    _verify_norm(n)
    assert bool(n.dst.isnan().all()), "a refused call wrote to the output"


def test_normalize_tiles_wrapper_equals_the_entry():
    """loader_math.normalize_tiles forms the range in float64 and rounds it once; with clip and without"""
    from srbh_amd import loader_math as LM
    shape = (2, 8, 7, 9)
    for clamp in ((0.0, 1.0), None):
        x, mins, ranges = O.norm_inputs(shape, clamp)
        maxs = mins.astype(np.float64) + ranges.astype(np.float64)
        out = LM.normalize_tiles(torch.from_numpy(x).to(DEV), mins.astype(np.float64), maxs, clamp)
        _same_bits(f"normalize_tiles {clamp}", out, O.normalize(x, mins, ranges, clamp))
