"""The inference epilogue (csrc/srbh_mosaic.hip) -- what the project delivers, and the instrument other tests measure the network with --
against the integer oracle of tests/io_ends_oracle.py at every edge of the city output: srbh_mosaic_accumulate and srbh_mosaic_finalize each
on their own through the C ABI, then mosaic.Mosaic on top.  Inputs are made on the CPU, never another kernel's output; every output lives
in guard-filled storage, every input is compared with its clone afterwards (tests/gpu_util.GuardedBuffers); accumulators start from non-zero
contents.  tests/test_io_ends_cpu.py proves by arithmetic that the case tables reach the forms named here.

NO mismatch is tolerated anywhere: res_height, res_weight, res_build, the finalised height and the finalised class map must EQUAL the oracle.
That can be demanded because the logits are chosen with no entry near a rounding boundary of round(softmax * 255), the one floating-point
step whose last bits are not determined (the derivation of the margin: tests/io_ends_oracle.py).

  accumulate   C 1 / 2 / 7 / 15 / 16; tiles 4 x 4, 8 x 20, 12 x 8, 64 x 64; 240 threads (below one workgroup), 272 / 288 / 800 (a ragged last
               workgroup), up to 57 344; against a city of 40 x 52 pixels windows that are full, cropped, of count 0 / 1 / negative / larger
               than the tile, overlapping, hanging over each of the four edges, wholly outside on each side (offsets within a tile of the
               city: the documented guard, not integer overflow); heights negative, -0.0, x10 ties on even and odd floors, 6553.5; outputs
               one element off a 16-byte boundary; 300 stacked tiles whose weight wraps past 255 (pixels with w8 == 0 and a height sum),
               4 x 2000.0 whose height sum passes 65 535, 300 tiles whose dominant class sum wraps so that another class wins; one call,
               two calls in reversed order and two Mosaic objects merged give the same bits; every refusal with nothing written.
  finalize     crafted accumulators with random bits above every mask; w8 = 0 with and without bit 8, w 1 / 2 / 3 / 255; the half-even ties of
               h / 2 (1 -> 0, 3 -> 2, 5 -> 2, 7 -> 4, 65535 -> 32768), quotients just off a tie with w = 255; all classes equal, a tie of a
               low and the last class, the maximum in the last class only, a tie and an order that exist only after the 16-bit mask;
               C 1 / 2 / 7 / 16 / 20 (finalisation has no upper limit on C: include/srbh.h); H W 1 / 255 / 256 / 257 / 1000.
  Mosaic       fp16 predictions and logits, channels-last and non-contiguous logits, posall as list / CPU tensor / device tensor; `_rows`
               after add, after merge_ and for a batch wholly outside; an empty batch.

Measured on an MI355X: exact everywhere -- no entry of any accumulator, height or class map differs in any of the 67 cases (under 4 s for this file and the loader's together, the
slowest case 0.3 s), the class-order case included; nothing was found wrong in the kernel's values.

Mutation check (scratch builds of the kernel with one change each, never committed; "older" = tests/test_gpu_mosaic.py):
  finalisation without `& 0xffu` on the weight        test_finalize (all 25), test_accumulate (all 10: the start weights carry bits above
                                                      bit 7), test_accumulate_wraps[weight, class]; older file passes
  `v >= best` for `v > best` in the argmax            test_finalize (every C > 1: 20), test_accumulate[c7_12x8_b30, c16_64x64_b14],
                                                      test_accumulate_wraps (3), test_mosaic_input_forms (4), test_mosaic_shards...; the older
                                                      file catches it as well (both tests: pixels no tile covers tie at zero)
  roundf for rintf in the height quantum              test_accumulate (all 10), test_accumulate_wraps[weight, class], test_accumulate_order_and_calls,
                                                      test_mosaic_input_forms (4), test_mosaic_shards...; the older file catches it (both tests)
  floor(x + 0.5) for rint in the final division       test_finalize (every shape beyond one pixel: 20), test_accumulate (all 10),
                                                      test_mosaic_input_forms (4), test_mosaic_shards...; the older file catches it (both tests)
  the softmax sum taken in descending class order     test_accumulate_sums_in_class_order[7, 16] ONLY: every other input keeps clear of the
                                                      rounding boundaries by construction, so that a sum in any order has the same right
                                                      answer; older file passes
The 64-bit window arithmetic of mosaic_accumulate_kernel has no test of its own (offsets near +-2^31 are not run); it rests on reading."""
import numpy as np
import pytest
import torch

from tests import io_ends_oracle as O
from tests.gpu_util import GuardedBuffers as Buffers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = O.CITY_H, O.CITY_W


def _lib():
    from srbh_amd import _lib as m
    return m, m.lib()


def _p(t):
    return None if t is None else t.data_ptr()


def _i32(a):
    """uint32 / int64 numpy (values below 2^32) -> int32 tensor of the same bits"""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.uint32)).view(np.int32))


def _u32(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _same(what, got, want):
    """print the figure, then demand zero"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = int((got != want).sum())
    print(f"IOENDS {what}: {bad} of {got.size} differ" + (f" (largest |d| {int(np.abs(got.astype(np.int64) - want.astype(np.int64)).max())})" if bad else ""))
    assert bad == 0, what


def _refused(rc, bufs, name):
    _, L = _lib()
    assert rc != 0, f"{name}: accepted"
    bufs.verify(written=False)
    assert name.encode() in L.srbh_last_error(), L.srbh_last_error()


class _Acc:
    """the device buffers of one srbh_mosaic_accumulate call: outputs one element past a 16-byte boundary, filled with `state`"""

    def __init__(self, inp, C):
        self.bufs = b = Buffers()
        Bn, th, tw = inp.height.shape
        self.shape = (C, Bn, th, tw)
        self.height = b.inp(torch.from_numpy(inp.height.copy()))
        self.logits = b.inp(torch.from_numpy(inp.logits.copy()), offset=1)
        self.pos = b.inp(torch.from_numpy(inp.pos.astype(np.int32)), dtype=torch.int32)
        st = inp.state if inp.state is not None else (np.zeros((H, W)), np.zeros((C, H, W)), np.zeros((H, W)))
        self.res_h = b.out((H, W), offset=1, fill=_i32(st[0]), dtype=torch.int32)
        self.res_b = b.out((C, H, W), offset=3, fill=_i32(st[1]), dtype=torch.int32)
        self.res_w = b.out((H, W), offset=2, fill=_i32(st[2]), dtype=torch.int32)

    def args(self):
        m, _ = _lib()
        C, Bn, th, tw = self.shape
        return [_p(self.height), _p(self.logits), C, Bn, th, tw, _p(self.pos), _p(self.res_h), _p(self.res_b), _p(self.res_w), H, W, m.stream_ptr()]

    def run(self):
        m, L = _lib()
        m.check(L.srbh_mosaic_accumulate(*self.args()), "mosaic_accumulate")
        self.bufs.verify()

    def compare(self, name, want):
        _same(f"{name} res_height", _u32(self.res_h), want.res_h)
        _same(f"{name} res_weight", _u32(self.res_w), want.res_w)
        _same(f"{name} res_build", _u32(self.res_b), want.res_b)


def _finalize(res_h, res_b, res_w, C, name):
    """srbh_mosaic_finalize on int32 device tensors of shape (H, W) / (C, H, W) -> uint16, uint8 numpy; guards and inputs verified"""
    m, L = _lib()
    h, w = res_h.shape
    bufs = Buffers()
    dh, db, dw = (bufs.inp(t, dtype=torch.int32) for t in (res_h, res_b, res_w))
    hout = bufs.out((h, w), offset=1, dtype=torch.int16)
    bout = bufs.out((h, w), offset=3, dtype=torch.uint8)
    m.check(L.srbh_mosaic_finalize(_p(dh), _p(db), _p(dw), C, h, w, _p(hout), _p(bout), m.stream_ptr()), "mosaic_finalize")
    bufs.verify()
    return hout.cpu().numpy().view(np.uint16), bout.cpu().numpy()


# ---- srbh_mosaic_accumulate ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", O.ACC_CASES, ids=[c.name for c in O.ACC_CASES])
def test_accumulate(case):
    inp = O.acc_inputs(case)
    a = _Acc(inp, case.C)
    a.run()
    a.compare(case.name, inp.want)
    # and what the city gets from these sums
    fh, fb = _finalize(a.res_h, a.res_b, a.res_w, case.C, case.name)
    wh, wb = O.mosaic_finalize(inp.want.res_h, inp.want.res_b, inp.want.res_w, case.C)
    _same(f"{case.name} height", fh, wh)
    _same(f"{case.name} class map", fb, wb)


@pytest.mark.parametrize("name", O.WRAP_CASES)
def test_accumulate_wraps(name):
    inp = O.wrap_inputs(name)
    C = inp.logits.shape[-1]
    a = _Acc(inp, C)
    a.run()
    a.compare(f"wrap_{name}", inp.want)
    fh, fb = _finalize(a.res_h, a.res_b, a.res_w, C, name)
    wh, wb = O.mosaic_finalize(inp.want.res_h, inp.want.res_b, inp.want.res_w, C)
    _same(f"wrap_{name} height", fh, wh)
    _same(f"wrap_{name} class map", fb, wb)


def test_accumulate_order_and_calls():
    """the same tiles in one call and in two calls in reversed order onto the same start: bit-identical accumulators"""
    case = O.ACC_CASES[5]
    assert case.name == "c7_12x8_b30"
    inp = O.acc_inputs(case)
    one = _Acc(inp, case.C)
    one.run()
    m, L = _lib()
    two = _Acc(inp, case.C)          # its outputs; the halves get input buffers of their own
    order = list(range(case.B))[::-1]
    for idx in (order[:13], order[13:]):
        part = inp._replace(height=inp.height[idx], logits=inp.logits[idx], pos=inp.pos[idx])
        h = _Acc(part, case.C)
        args = h.args()
        args[7:10] = [_p(two.res_h), _p(two.res_b), _p(two.res_w)]
        m.check(L.srbh_mosaic_accumulate(*args), "mosaic_accumulate")
        h.bufs.verify(written=False)         # (its own outputs were not the call's)
    two.bufs.verify()
    two.compare("two calls", inp.want)
    assert torch.equal(one.res_h, two.res_h) and torch.equal(one.res_b, two.res_b) and torch.equal(one.res_w, two.res_w)


@pytest.mark.parametrize("C", [7, 16])
def test_accumulate_sums_in_class_order(C):
    """the one case inside the rounding margin: its answer follows from the header's order of the sum, not from float64 (O.order_case)"""
    zf, qf = O.order_case(C, True)
    zl, ql = O.order_case(C, False)
    z = np.stack([zf, zl] * 8).reshape(1, 4, 4, C)
    inp = O.AccInputs(np.zeros((1, 4, 4), np.float32), z, np.array([[5, 7, 4, 4]]), None, None)
    a = _Acc(inp, C)
    a.run()
    want = np.zeros((C, H, W), dtype=np.uint32)
    want[:, 7:11, 5:9] = np.stack([qf, ql] * 8).reshape(4, 4, C).transpose(2, 0, 1)
    _same(f"class order C={C} res_build", _u32(a.res_b), want)


_ACC_ARG = ("height", "build", "C", "B", "th", "tw", "pos", "res_height", "res_build", "res_weight", "H", "W")


@pytest.mark.parametrize("what", ["C=0", "C=17", "B=0", "th=0", "tw=0", "H=0", "W=0"] + [f"{n}=null" for n in _ACC_ARG if n[0] in "hbpr"])
def test_accumulate_refusals(what):
    _, L = _lib()
    inp = O.acc_inputs(O.ACC_CASES[1])
    a = _Acc(inp, 2)
    args = a.args()
    name, val = what.split("=")
    args[_ACC_ARG.index(name)] = None if val == "null" else int(val)
    _refused(L.srbh_mosaic_accumulate(*args), a.bufs, "srbh_mosaic_accumulate")


# ---- srbh_mosaic_finalize on crafted accumulators --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", O.FIN_C)
@pytest.mark.parametrize("shape", O.FIN_SHAPES, ids=[f"hw{h * w}" for h, w in O.FIN_SHAPES])
def test_finalize(shape, C):
    res_h, res_b, res_w = O.finalize_inputs(C, *shape)
    fh, fb = _finalize(_i32(res_h), _i32(res_b), _i32(res_w), C, f"fin{shape}")
    wh, wb = O.mosaic_finalize(res_h, res_b, res_w, C)
    _same(f"finalize {shape} C={C} height", fh, wh)
    _same(f"finalize {shape} C={C} class map", fb, wb)
    n = min(shape[0] * shape[1], len(O.FIN_HW))
    assert fh.reshape(-1)[:n].tolist() == list(O.FIN_HW_WANT[:n])                 # the table's known answers, literally


@pytest.mark.parametrize("what", ["C=0", "H=0", "W=0", "res_height=null", "res_build=null", "res_weight=null", "height_out=null", "build_out=null"])
def test_finalize_refusals(what):
    m, L = _lib()
    res_h, res_b, res_w = O.finalize_inputs(2, 5, 51)
    bufs = Buffers()
    dh, db, dw = (bufs.inp(_i32(t), dtype=torch.int32) for t in (res_h, res_b, res_w))
    hout, bout = bufs.out((5, 51), dtype=torch.int16), bufs.out((5, 51), dtype=torch.uint8)
    names = ("res_height", "res_build", "res_weight", "C", "H", "W", "height_out", "build_out")
    args = [_p(dh), _p(db), _p(dw), 2, 5, 51, _p(hout), _p(bout), m.stream_ptr()]
    name, val = what.split("=")
    args[names.index(name)] = None if val == "null" else int(val)
    _refused(L.srbh_mosaic_finalize(*args), bufs, "srbh_mosaic_finalize")


# ---- mosaic.Mosaic ---------------------------------------------------------------------------------------------------------------------------
def _mosaic_equals(mo, want, name):
    _same(f"{name} res_height", _u32(mo.res_height), want.res_h)
    _same(f"{name} res_weight", _u32(mo.res_weight), want.res_w)
    _same(f"{name} res_build", _u32(mo.res_build), want.res_b)
    fh, fb = mo.finalize()
    wh, wb = O.mosaic_finalize(want.res_h, want.res_b, want.res_w, mo.C)
    _same(f"{name} height", fh.cpu().view(torch.int16).numpy().view(np.uint16), wh)
    _same(f"{name} class map", fb.cpu().numpy(), wb)


def _nchw(z):
    return torch.from_numpy(z.copy()).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("form", ["plain_list", "fp16_cpu_pos", "channels_last_device_pos", "sliced"])
def test_mosaic_input_forms(form):
    from srbh_amd.mosaic import Mosaic
    c = O.WRAPPER
    h, z, cells = O.wrapper_inputs(fp16=form.startswith("fp16"))
    want = O.mosaic_accumulate(h, z, cells * 4, H, W)
    y, b = torch.from_numpy(h.copy())[:, None].to(DEV), _nchw(z).to(DEV)
    pos = cells.tolist()
    if form == "fp16_cpu_pos":
        y, b, pos = y.half(), b.half(), torch.from_numpy(cells)
        assert torch.equal(y.float().cpu()[:, 0], torch.from_numpy(h.copy())) and torch.equal(b.float().cpu(), _nchw(z))
    elif form == "channels_last_device_pos":
        b, pos = b.contiguous(memory_format=torch.channels_last), torch.from_numpy(cells).to(DEV)
        assert not b.is_contiguous()
    elif form == "sliced":           # every second tile / channel / column of larger tensors
        yy = torch.full((c.B, 2, c.th, 2 * c.tw), 7.5, device=DEV)
        bb = torch.full((2 * c.B, 2 * c.C, c.th, c.tw), 1.5, device=DEV)
        yy[:, 1:, :, ::2], bb[::2, ::2] = y, b
        y, b = yy[:, 1:, :, ::2], bb[::2, ::2]
        assert not y.is_contiguous() and not b.is_contiguous()
    before = (y.clone(), b.clone())
    mo = Mosaic(H, W, c.C, DEV)
    mo.add(y, b, pos)
    assert torch.equal(y, before[0]) and torch.equal(b, before[1])
    _mosaic_equals(mo, want, form)
    ys = cells[:, 1] * 4
    assert mo._rows == [max(0, int(ys.min())), min(H, int((ys + cells[:, 3] * 4).max()))] == [0, H]


def test_mosaic_shards_rows_and_empty_batch():
    from srbh_amd.mosaic import Mosaic
    c = O.WRAPPER
    h, z, cells = O.wrapper_inputs()
    want = O.mosaic_accumulate(h, z, cells * 4, H, W)
    y, b = torch.from_numpy(h.copy())[:, None].to(DEV), _nchw(z).to(DEV)
    inside = [i for i in range(c.B) if 0 <= cells[i, 1] and cells[i, 3] > 0 and cells[i, 1] * 4 < H]
    lo = sorted(inside, key=lambda i: cells[i, 1])[: len(inside) // 2]                 # the tiles of the upper rows ...
    rest = [i for i in range(c.B) if i not in lo][::-1]                                # ... and every other one, reversed
    a, r = Mosaic(H, W, c.C, DEV), Mosaic(H, W, c.C, DEV)
    a.add(y[lo], b[lo], cells[lo].tolist())
    band = [int(cells[lo, 1].min()) * 4, min(H, int((cells[lo, 1] + cells[lo, 3]).max()) * 4)]
    assert a._rows == band and band[1] > band[0]
    r.add(y[rest], b[rest], cells[rest].tolist())
    rows_r = list(r._rows)
    # an empty batch adds nothing and launches nothing
    snap = (a.res_height.clone(), a.res_build.clone(), a.res_weight.clone())
    a.add(y[:0], b[:0], [])
    a.add(y[:0], b[:0], torch.zeros((0, 4), dtype=torch.int64))
    assert a._rows == band and all(torch.equal(s, t) for s, t in zip(snap, (a.res_height, a.res_build, a.res_weight)))
    a.merge_(r)
    assert a._rows == [min(band[0], rows_r[0]), max(band[1], rows_r[1])]
    _mosaic_equals(a, want, "merged shards")
    # a batch wholly outside the city: nothing added, an empty band
    out = Mosaic(H, W, c.C, DEV)
    out.add(y[:3], b[:3], [[0, H // 4 + 1, 2, 2], [3, H // 4, 2, 2], [1, H // 4 + 2, 1, 1]])
    assert out._rows[1] <= out._rows[0] and not out.res_weight.any() and not out.res_height.any() and not out.res_build.any()
    up = Mosaic(H, W, c.C, DEV)
    up.add(y[:2], b[:2], [[3, -2, 2, 2], [W // 4, -2, 2, 2]])
    assert up._rows[1] <= up._rows[0] and not up.res_weight.any() and not up.res_build.any()
    before = list(a._rows)
    a.merge_(out)                    # merging an empty band leaves the band as it was
    assert a._rows == before
