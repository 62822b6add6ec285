"""GPU: the city summary (srbh_window_sums, srbh_block_sums, srbh_value_hist; city_summary.window_sums / block_sums / value_histogram /
cell_heights / aggregate_city / city_summary) against the numpy oracle tests/city_summary_oracle.py.

Everything the kernels return is an integer, so every number is compared EXACTLY; the floats of the host layer are compared bit for bit
(a NaN with a NaN).  The shapes are the smallest at which the kernels can go wrong: a 131-wide raster (odd: the 16-byte alignment of a
row changes from row to row), windows that start at every byte offset of a 16-byte group, rasters that are interior views of a larger
buffer whose every other element is the LARGEST value (a load or a predicate that left the raster shows as a wrong sum, not as a
fault), every block size at which srbh_block_sums changes its owner (lane <= 8 < wave <= 64 < workgroup), sums beyond 2^32."""
import numpy as np
import pytest
import torch

from srbh_amd import _lib
from srbh_amd import city_grid as CG
from srbh_amd import city_summary as CS
from srbh_amd.loader_math import grid_windows
from tests import city_summary_oracle as SO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, U16, I16, U8 = 0, 1, 2, 3                           # include/srbh.h SRBH_GRID_*
H0, W0 = 70, 131
INT_MAX = 2 ** 31 - 1
GARBAGE = -0x0123456789abcdef
ERR_ARG = -1                                             # include/srbh.h SRBH_ERR_ARG
BLOCKS = (1, 3, 4, 5, 40, 64, 400, 5000)                 # (5000: larger than every raster here)


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).to(DEV).view(torch.uint16)
    return torch.from_numpy(a).to(DEV)


def raster(dtype, H, W, seed, zeros=0.5):
    """`zeros` of the pixels are 0; both ends of the type are present"""
    rs = np.random.RandomState(seed)
    top = np.iinfo(dtype).max
    a = rs.randint(0, top + 1, size=(H, W)).astype(dtype)
    a[rs.rand(H, W) < zeros] = 0
    a[0, 0], a[-1, -1], a[0, -1], a[-1, 0] = top, top, 1, top - 1
    return a


def framed(a, top=1, left=3, bottom=1, right=2):
    """`a` as an interior view of a larger device buffer whose every other element is the type's largest value (selected at every
    threshold below it, and the largest addend there is); the view starts at an odd element of the buffer"""
    H, W = a.shape
    buf = np.full((H + top + bottom, W + left + right), np.iinfo(a.dtype).max, dtype=a.dtype)
    buf[top:top + H, left:left + W] = a
    return dev(buf)[top:top + H, left:left + W]


def edge_windows(H, W):
    """xoff 0..17 x xcount 1..40 (a stride of widths, every one of them once) x ycount 1, 3 and H; the same flush with the right edge;
    the four corner pixels; the whole raster"""
    pos = []
    for xoff in range(18):
        for i, xcount in enumerate(range(1 + xoff % 3, 41, 3)):
            for ycount, yoff in ((1, (xoff * 7 + xcount) % H), (3, (xoff * 5 + xcount) % (H - 2)), (H, 0)):
                pos.append((xoff, yoff, xcount, ycount))
                pos.append((W - xcount - (xoff + i) % 3, yoff, xcount, ycount))
    pos += [(0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1), (0, 0, W, H), (0, 0, W, 1), (0, H - 1, W, 1),
            (0, 0, 1, H), (W - 1, 0, 1, H), (0, 0, 40, H), (W - 40, 0, 40, H)]
    return np.array(pos, dtype=np.int64)


def sums(*a, **k):
    return CS.window_sums(*a, **k).cpu().numpy()


def test_edge_windows_cover_what_they_claim():
    pos = edge_windows(H0, W0)
    assert set(pos[:, 0].tolist()) >= set(range(18)) and set(pos[:, 2].tolist()) >= set(range(1, 41))
    assert {1, 3, H0} <= set(pos[:, 3].tolist()) and (pos[:, 0] + pos[:, 2] == W0).any() and (pos[:, 1] + pos[:, 3] == H0).any()


# ---- windows ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tv", [np.uint16, np.uint8])
@pytest.mark.parametrize("tm", [None, np.uint8, np.uint16])
def test_window_edges_and_row_alignment(tv, tm):
    v = raster(tv, H0, W0, 1)
    m = None if tm is None else raster(tm, H0, W0, 2)
    pos = edge_windows(H0, W0)
    pos = np.concatenate([pos, pos[5:9], pos[:3], CG.fishgrid_windows(W0, H0, 16, 14)])                # repeated and overlapping windows
    want = SO.window_sums(v, pos, m)
    assert (want[:, 1] == 0).any() and (want[:, 1] == want[:, 0]).sum() < len(pos) // 2 and (want[:, 0] == pos[:, 2] * pos[:, 3]).all()
    got = sums(dev(v), pos, None if m is None else dev(m))
    assert got.dtype == np.int64 and np.array_equal(got, want)
    # the memory contract: interior views of larger buffers -- strided rows, unaligned bases, different strides for the two
    fv = framed(v)
    fm = None if m is None else framed(m, 2, 5, 3, 1)
    assert not fv.is_contiguous() and fv.data_ptr() % 16 != 0 and (fm is None or fm.stride(0) != fv.stride(0))
    assert np.array_equal(sums(fv, pos, fm), want)


def test_windows_partly_wholly_and_absurdly_outside():
    """a device pos is used as is: count and the sums cover only what lies inside the raster"""
    v, m = raster(np.uint16, H0, W0, 3), raster(np.uint8, H0, W0, 4, zeros=0.2)
    pos = np.array([(-5, -4, 20, 10), (W0 - 7, H0 - 2, 30, 30), (-16, 10, 17, 5), (-16, 10, 16, 5), (W0, 0, 5, 5), (0, H0, 5, 5),
                    (W0 - 1, H0 - 1, INT_MAX, INT_MAX), (-3, -3, INT_MAX, INT_MAX), (100, 60, INT_MAX, 3), (-INT_MAX, -INT_MAX, INT_MAX, INT_MAX),
                    (-INT_MAX, 0, INT_MAX, 5), (5, 5, 0, 5), (5, 5, 5, 0), (5, 5, -3, 5), (5, 5, 5, -INT_MAX), (-40, 3, W0 + 80, 1),
                    (W0 - 16, 0, 17, H0), (W0 - 15, -1, 16, 2), (-INT_MAX - 1, -INT_MAX - 1, INT_MAX, INT_MAX), (0, 0, W0, H0)], dtype=np.int64)
    want = SO.window_sums(v, pos, m)
    assert (want[:, 0] == 0).sum() >= 8 and want[7, 0] == H0 * W0 and (want[:, 1] > 0).sum() >= 8
    pos_d = torch.from_numpy(pos.astype(np.int32)).to(DEV)
    assert np.array_equal(sums(framed(v), pos_d, framed(m, 2, 5, 3, 1)), want)
    assert np.array_equal(sums(framed(v), pos_d), SO.window_sums(v, pos))
    assert np.array_equal(sums(framed(m), pos_d, framed(v, 2, 6, 1, 1)), SO.window_sums(m, pos, v))
    with pytest.raises(ValueError, match="window_sums.*row 0"):       # the host path refuses them
        CS.window_sums(dev(v), pos)


@pytest.fixture(scope="module")
def city():
    """the median-city size: 4000 x 3000 rasters built like predict_city's, the 3 888 windows of 64 / 56 and their sums"""
    rs = np.random.RandomState(8)
    b = np.zeros((3000, 4000), dtype=np.uint8)
    for _ in range(400):                                              # blobs: most of a city's cells hold no building
        x, y = rs.randint(0, 3900), rs.randint(0, 2900)
        b[y:y + rs.randint(5, 120), x:x + rs.randint(5, 120)] = rs.randint(1, 7)
    h = (rs.gamma(2.0, 60.0, size=b.shape)).astype(np.uint16)
    h[(b == 0) & (rs.rand(*b.shape) < 0.9)] = 0                       # (class 0 with a non-zero height stays here and there)
    pos = CG.fishgrid_windows(4000, 3000)
    assert pos.shape == (3888, 4)
    return h, b, pos, SO.window_sums(h, pos, b)


def test_one_window_a_whole_city_overwrite_repeat_and_device_pos(city):
    h, b, pos, want = city
    dh, db = dev(h), dev(b)
    pos_d = torch.from_numpy(pos.astype(np.int32)).to(DEV)
    out = torch.full((len(pos), 5), GARBAGE, dtype=torch.int64, device=DEV)                     # garbage: every element is overwritten
    _lib.check(_lib.lib().srbh_window_sums(dh.data_ptr(), U16, 4000, db.data_ptr(), U8, 4000, 3000, 4000, pos_d.data_ptr(), len(pos), 0, 0,
                                           out.data_ptr(), _lib.stream_ptr()), "srbh_window_sums")
    assert np.array_equal(out.cpu().numpy(), want) and (want[:, 1] == 0).any() and (want[:, 1] > 2000).any()
    first, second, host = CS.window_sums(dh, pos_d, db), CS.window_sums(dh, pos_d, db), CS.window_sums(dh, pos, db)
    assert first.dtype == torch.int64 and first.is_cuda and torch.equal(first, second) and torch.equal(first, host) and torch.equal(first, out)
    for n in (0, 1234, 3887):
        assert np.array_equal(sums(dh, pos[n:n + 1], db), want[n:n + 1])                          # N = 1
    table = CS.cell_heights(dh, pos, db)
    ref = SO.heights(want)
    for k in ("n", "count", "max"):
        assert np.array_equal(table[k], ref[k]), k
    for k in ("fraction", "mean", "std"):
        assert SO.same_bits(table[k], ref[k]), k
    assert np.isnan(table["mean"]).any() and (table["std"] > 0).any()


def test_sums_beyond_32_bits():
    full = np.full((1024, 1024), 65535, dtype=np.uint16)
    pos = np.array([(0, 0, 1024, 1024), (100, 200, 300, 300), (0, 0, 1, 1)])
    got = sums(dev(full), pos)
    assert got.tolist() == [[n, n, n * 65535, n * 65535 ** 2, 65535] for n in (1024 * 1024, 90000, 1)]
    assert got[0, 2] > 2 ** 32 and got[0, 3] > 4.5e15 and got[1, 3] > 2 ** 32
    assert np.array_equal(sums(dev(full), pos, dev(np.full((1024, 1024), 255, np.uint8))), got)
    one = np.zeros((300, 300), dtype=np.uint16)
    one[177, 203] = 65535                                             # one selected pixel among zeros
    assert sums(dev(one), [(0, 0, 300, 300), (203, 177, 1, 1), (0, 0, 203, 300)]).tolist() == \
        [[90000, 1, 65535, 65535 ** 2, 65535], [1, 1, 65535, 65535 ** 2, 65535], [203 * 300, 0, 0, 0, 0]]
    blocks = CS.block_sums(dev(full), 400).cpu().numpy()              # a workgroup's block: 160 000 pixels of 65535
    assert np.array_equal(blocks, SO.block_sums(full, 400)) and blocks[2].max() == 160000 * 65535 ** 2
    assert CS.block_sums(dev(full), 1024).cpu().numpy().reshape(-1).tolist() == got[0, 1:].tolist()


def test_thresholds():
    values = (0, 1, 6, 7, 254, 255, 256, 65534, 65535)
    rs = np.random.RandomState(5)
    v = np.array(values, dtype=np.uint16)[rs.randint(0, len(values), size=(29, 37))]
    m = np.array((0, 1, 6, 7, 254, 255), dtype=np.uint8)[rs.randint(0, 6, size=(29, 37))]
    m16 = np.array(values, dtype=np.uint16)[rs.randint(0, len(values), size=(29, 37))]
    v[0, :len(values)] = values
    pos = np.array([(0, 0, 37, 29), (0, 0, len(values), 1), (5, 3, 19, 11), (36, 28, 1, 1)] + [(i, 0, 1, 1) for i in range(len(values))])
    dv, dm, dm16 = dev(v), dev(m), dev(m16)
    for vthr in (-1, 0, 254, 65534, 65535):
        assert np.array_equal(sums(dv, pos, value_threshold=vthr), SO.window_sums(v, pos, None, vthr)), vthr
        for mthr in (-1, 0, 6, 255):
            want = SO.window_sums(v, pos, m, vthr, mthr)
            assert np.array_equal(sums(dv, pos, dm, vthr, mthr), want), (vthr, mthr)
            assert np.array_equal(sums(dv, pos, dm16, vthr, mthr), SO.window_sums(v, pos, m16, vthr, mthr)), (vthr, mthr)
            if vthr == 65535 or mthr == 255:                          # an all-unselected window
                assert (want[:, 1:] == 0).all() and want[0, 0] == 37 * 29
            assert np.array_equal(CS.block_sums(dv, 5, dm, vthr, mthr).cpu().numpy(), SO.block_sums(v, 5, m, vthr, mthr))
    everything = sums(dv, pos, dm, -1, -1)
    assert np.array_equal(everything[:, 0], everything[:, 1]) and np.array_equal(everything, SO.window_sums(v, pos, None, -1))


# ---- blocks -----------------------------------------------------------------------------------------------------------------------------------
def raw_blocks(v, m, block, out, vthr=0, mthr=0):
    H, W = v.shape
    return _lib.lib().srbh_block_sums(v.data_ptr(), U16 if v.dtype == torch.uint16 else U8, v.stride(0), None if m is None else m.data_ptr(),
                                      0 if m is None else (U16 if m.dtype == torch.uint16 else U8), 0 if m is None else m.stride(0), H, W,
                                      block, vthr, mthr, out.data_ptr(), _lib.stream_ptr())


@pytest.mark.parametrize("H,W", [(H0, W0), (150, 200)])
@pytest.mark.parametrize("block", BLOCKS)
def test_blocks_equal_windows_and_oracle(H, W, block):
    v, m = raster(np.uint16, H, W, 6), raster(np.uint8, H, W, 7, zeros=0.3)
    want = SO.block_sums(v, block, m)
    Hb, Wb = -(-H // block), -(-W // block)
    dv, dm = dev(v), dev(m)
    got = CS.block_sums(dv, block, dm)
    assert tuple(got.shape) == (4, Hb, Wb) and got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
    cell = min(block, max(H, W))
    by_window = CS.window_sums(dv, grid_windows(W, H, cell, cell), dm)                             # row-major, clipped: the (Hb, Wb) order
    assert torch.equal(got.reshape(4, -1).t(), by_window[:, 1:])
    # strided views of buffers full of the largest value, a NaN-patterned out (there is no workspace), the other type pairing
    fv, fm = framed(v), framed(m, 2, 5, 3, 1)
    out = torch.full((4, Hb, Wb), float("nan"), dtype=torch.float64, device=DEV).view(torch.int64)
    _lib.check(raw_blocks(fv, fm, block, out), "srbh_block_sums")
    assert np.array_equal(out.cpu().numpy(), want)
    if (H, W) == (H0, W0):                                            # (the oracle walks every block in Python: the variants on the smaller raster)
        assert np.array_equal(CS.block_sums(framed(m), block, framed(v, 1, 1, 2, 4)).cpu().numpy(), SO.block_sums(m, block, v))
        assert np.array_equal(CS.block_sums(fv, block).cpu().numpy(), SO.block_sums(v, block))


@pytest.mark.parametrize("block", [400, 1001, INT_MAX])
def test_large_blocks_on_a_larger_raster(block):
    v, m = raster(np.uint16, 801, 1000, 9), raster(np.uint8, 801, 1000, 10, zeros=0.3)
    got = CS.block_sums(dev(v), block, dev(m))
    assert np.array_equal(got.cpu().numpy(), SO.block_sums(v, min(block, 1001), m))
    assert tuple(got.shape) == ((4, 3, 3) if block == 400 else (4, 1, 1))
    assert torch.equal(CS.block_sums(framed(v), block, framed(m, 2, 5, 3, 1)), got)


# ---- histogram --------------------------------------------------------------------------------------------------------------------------------
def hist_cases():
    every = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    return {"7x9": raster(np.uint16, 7, 9, 11), "131x70": raster(np.uint16, H0, W0, 12), "300x300": raster(np.uint16, 300, 300, 13),
            "zeros": np.zeros((H0, W0), np.uint16), "one value": np.full((H0, W0), 777, np.uint16), "every value": every,
            "uint8": raster(np.uint8, H0, W0, 14)}


@pytest.mark.parametrize("name", list(hist_cases()))
def test_histogram_equals_bincount(name):
    v = hist_cases()[name]
    m = raster(np.uint8, *v.shape, 15, zeros=0.3)
    dv, dm, fv, fm = dev(v), dev(m), framed(v), framed(m, 2, 5, 3, 1)
    for bin_width in (1, 10, 257):
        for nbins in (1, 7, 256, 4096):
            for mask, dmask, fmask in ((None, None, None), (m, dm, fm)):
                want = SO.value_hist(v, bin_width, nbins, mask)
                sel = (v > 0) if mask is None else (v > 0) & (mask > 0)
                assert np.array_equal(want, np.bincount(np.minimum(v[sel].astype(np.int64) // bin_width, nbins - 1), minlength=nbins))
                got = CS.value_histogram(dv, bin_width, nbins, dmask)
                assert got.dtype == torch.int64 and tuple(got.shape) == (nbins,) and np.array_equal(got.cpu().numpy(), want), (bin_width, nbins)
                need = _lib.lib().srbh_value_hist_ws_bytes(v.shape[0], v.shape[1], nbins)
                ws = torch.full((need // 8 + 1,), float("nan"), dtype=torch.float64, device=DEV)      # strided rows, a NaN-filled workspace
                assert np.array_equal(CS.value_histogram(fv, bin_width, nbins, fmask, workspace=ws).cpu().numpy(), want)
    counts = CS.value_histogram(dv, 1, 4096, value_threshold=-1).cpu().numpy()                      # every pixel, zeros included
    assert counts.sum() == v.size and np.array_equal(counts, SO.value_hist(v, 1, 4096, None, -1))
    with pytest.raises(ValueError, match="workspace"):
        CS.value_histogram(dv, 1, 4096, workspace=torch.empty(16, dtype=torch.uint8, device=DEV))


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_like_predict_city():
    rs = np.random.RandomState(16)
    H, W = 280, 524
    build = np.zeros((H, W), dtype=np.uint8)
    for _ in range(60):
        x, y = rs.randint(0, W - 10), rs.randint(0, H - 10)
        build[y:y + rs.randint(3, 60), x:x + rs.randint(3, 60)] = rs.randint(1, 7)
    height = np.round(10 * rs.gamma(2.0, 6.0, size=(H, W))).astype(np.uint16)
    height[(build == 0) & (rs.rand(H, W) < 0.8)] = 0                  # zeros where nothing was predicted; class 0 with a height remains
    height[rs.rand(H, W) < 0.05] = 0
    assert ((build == 0) & (height > 0)).any() and ((build > 0) & (height == 0)).any()
    dh, db = dev(height), dev(build)
    pos = CG.fishgrid_windows(W, H)
    table, ref = CS.cell_heights(dh, pos, db), SO.heights(SO.window_sums(height, pos, build))
    for k in ("n", "count", "max"):
        assert np.array_equal(table[k], ref[k]), k
    for k in ("fraction", "mean", "std"):
        assert SO.same_bits(table[k], ref[k]), k
    for block in (4, 40):
        got, want = CS.aggregate_city(dh, block, db), SO.aggregate(height, block, build)
        assert set(got) == set(want)
        for k in ("n", "count", "max"):
            assert got[k].dtype == torch.int64 and np.array_equal(got[k].cpu().numpy(), want[k]), (block, k)
        for k in ("mean", "fraction", "density"):
            g = got[k].cpu().numpy()
            nan = np.isnan(want[k])
            assert g.dtype == np.float64 and np.array_equal(np.isnan(g), nan) and SO.same_bits(g[~nan], want[k][~nan]), (block, k)
        assert np.isnan(want["mean"]).any() and not np.isnan(want["density"]).any() and got["count"].sum().item() == H * W
    for b_np, b_dev in ((build, db), (None, None)):
        got, want = CS.city_summary(dh, b_dev), SO.summary(height, b_np)
        assert got["count"] == want["count"] == H * W and got["n"] == want["n"] and got["max"] == want["max"]
        assert SO.same_bits(got["mean"], want["mean"]) and SO.same_bits(got["std"], want["std"])
        assert np.array_equal(got["hist"], want["hist"]) and got["hist"].sum() == got["n"]
        if b_np is None:
            assert got["class_counts"] is None
        else:
            assert np.array_equal(got["class_counts"], want["class_counts"]) and got["class_counts"].sum() == got["count"]
            assert np.array_equal(got["class_counts"], np.bincount(build.reshape(-1), minlength=7))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_c_abi_refusals_launch_nothing():
    v, m = raster(np.uint16, H0, W0, 17), raster(np.uint8, H0, W0, 18)
    dv, dm = dev(v), dev(m)
    pos_d = torch.tensor([[0, 0, 16, 16]], dtype=torch.int32, device=DEV)
    lib, ptr = _lib.lib(), (lambda t: None if t is None else t.data_ptr())
    common = dict(v=dv, tv=U16, rsv=W0, m=dm, tm=U8, rsm=W0, H=H0, W=W0, vthr=0, mthr=0)
    outs = {"win": torch.full((1, 5), GARBAGE, dtype=torch.int64, device=DEV), "blk": torch.full((4, 2, 4), GARBAGE, dtype=torch.int64, device=DEV),
            "hist": torch.full((7,), GARBAGE, dtype=torch.int64, device=DEV)}
    ws = torch.zeros(lib.srbh_value_hist_ws_bytes(H0, W0, 7), dtype=torch.uint8, device=DEV)

    def win(a):
        return lib.srbh_window_sums(ptr(a["v"]), a["tv"], a["rsv"], ptr(a["m"]), a["tm"], a["rsm"], a["H"], a["W"], ptr(a.get("pos", pos_d)),
                                    a.get("N", 1), a["vthr"], a["mthr"], ptr(a.get("out", outs["win"])), _lib.stream_ptr())

    def blk(a):
        return lib.srbh_block_sums(ptr(a["v"]), a["tv"], a["rsv"], ptr(a["m"]), a["tm"], a["rsm"], a["H"], a["W"], a.get("block", 40),
                                   a["vthr"], a["mthr"], ptr(a.get("out", outs["blk"])), _lib.stream_ptr())

    def hist(a):
        return lib.srbh_value_hist(ptr(a["v"]), a["tv"], a["rsv"], ptr(a["m"]), a["tm"], a["rsm"], a["H"], a["W"], a["vthr"], a["mthr"],
                                   a.get("bin_width", 10), a.get("nbins", 7), ptr(a.get("out", outs["hist"])), ptr(a.get("ws", ws)),
                                   _lib.stream_ptr())

    shared = [dict(tv=I16), dict(tv=F32), dict(tv=4), dict(tv=-1), dict(tm=I16), dict(tm=F32), dict(tm=9), dict(v=None), dict(out=None),
              dict(H=0), dict(W=0), dict(H=-3), dict(rsv=W0 - 1), dict(rsm=W0 - 1), dict(H=2 ** 16, W=2 ** 15, rsv=2 ** 15, rsm=2 ** 15),
              dict(vthr=-2), dict(vthr=65536), dict(mthr=-2), dict(mthr=65536), dict(v=dv.view(torch.uint8)[:, 1:]),
              dict(m=dev(m.astype(np.uint16)).view(torch.uint8)[:, 1:], tm=U16)]
    own = {"srbh_window_sums": (win, [dict(pos=None), dict(N=0), dict(N=-1)]),
           "srbh_block_sums": (blk, [dict(block=0), dict(block=-40)]),
           "srbh_value_hist": (hist, [dict(ws=None), dict(bin_width=0), dict(bin_width=65536), dict(nbins=0), dict(nbins=4097)])}
    for name, (call, extra) in own.items():
        for change in shared + extra:
            rc = call({**common, **change})
            assert rc == ERR_ARG, (name, change)
            with pytest.raises(RuntimeError, match=name):
                _lib.check(rc, name)
    torch.cuda.synchronize()
    for out in outs.values():                                         # nothing was launched: the garbage stands
        assert (out == GARBAGE).all()
    assert win(common) == 0 and blk(common) == 0 and hist(common) == 0
    assert np.array_equal(outs["win"].cpu().numpy(), SO.window_sums(v, [(0, 0, 16, 16)], m))
    assert np.array_equal(outs["blk"].cpu().numpy(), SO.block_sums(v, 40, m))
    assert np.array_equal(outs["hist"].cpu().numpy(), SO.value_hist(v, 10, 7, m))
    # a null mask makes its type code and stride irrelevant
    assert win({**common, "m": None, "tm": 99, "rsm": 0}) == 0
    assert np.array_equal(outs["win"].cpu().numpy(), SO.window_sums(v, [(0, 0, 16, 16)]))
    # the Python layer on device tensors
    with pytest.raises(TypeError, match="window_sums"):
        CS.window_sums(dv.view(torch.int16), [(0, 0, 16, 16)])
    with pytest.raises(ValueError, match="int32"):
        CS.window_sums(dv, torch.zeros((1, 4), dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU"):
        CS.block_sums(torch.from_numpy(m), 4)
