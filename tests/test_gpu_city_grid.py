"""GPU: the per-window counts of a city's grid (srbh_cell_counts, city_grid.cell_counts / fishgrid_stats / compare_cells / city_windows)
against the numpy oracle tests/city_grid_oracle.py, which tests/golden/g20_city_grid.npz pins against the reference's own functions.

Everything is an integer, so every count of every window is compared EXACTLY.  The shapes are the smallest at which the kernel can
go wrong: a 131-wide raster (odd: the 16-byte alignment of a window row changes from row to row), windows that start at every byte
offset of a 16-byte group and end before, on and behind a group boundary, windows flush with every edge, rasters that are interior
views of a larger buffer whose every other element WOULD count (a load or a predicate that leaves the raster shows as a wrong count,
not as a fault), windows of more than 256 groups, and the 3 888 windows of a 4000 x 3000 city."""
import os

import numpy as np
import pytest
import torch

from srbh_amd import _lib
from srbh_amd import city_grid as CG
from srbh_amd import loader_math as LM
from tests import city_grid_oracle as CO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, U16, I16, U8 = 0, 1, 2, 3                           # include/srbh.h SRBH_GRID_*
H0, W0 = 70, 131
INT_MAX = 2 ** 31 - 1


def dev(a):
    """a numpy raster on the device as a torch tensor of its own type (uint16 travels as int16 bits)"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).to(DEV).view(torch.uint16)
    return torch.from_numpy(a).to(DEV)


def raster(dtype, H, W, seed):
    """about half the pixels count at threshold 0, under either value map; both ends of the type are present"""
    rs = np.random.RandomState(seed)
    info = np.iinfo(dtype)
    a = rs.randint(info.min, info.max + 1, size=(H, W)).astype(dtype)
    a[rs.rand(H, W) < 0.5] = 0
    a[0, 0], a[-1, -1], a[0, -1], a[-1, 0] = info.max, info.max, info.min, 1
    return a


def framed(a, top=1, left=3, bottom=1, right=2):
    """`a` as an interior view of a larger device buffer whose every other element counts at any threshold below 255 under either
    value map (255: the largest uint8, the low byte of a positive int16); the view starts at an odd element of the buffer"""
    H, W = a.shape
    buf = np.full((H + top + bottom, W + left + right), 255, dtype=a.dtype)
    buf[top:top + H, left:left + W] = a
    return dev(buf)[top:top + H, left:left + W]


def edge_windows(H, W):
    """xoff 0..17 (every byte offset of a 16-byte group and two more) x xcount around one, two and three groups x ycount 1, 3 and H;
    the same flush with the right edge; the four corner pixels; the whole raster"""
    pos = []
    for xoff in range(18):
        for xcount in (1, 2, 15, 16, 17, 33, 40):
            for ycount, yoff in ((1, (xoff * 7 + xcount) % H), (3, (xoff * 5 + xcount) % (H - 2)), (H, 0)):
                pos.append((xoff, yoff, xcount, ycount))
                pos.append((W - xcount - xoff % 3, yoff, xcount, ycount))
    pos += [(0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1), (0, 0, W, H)]
    return np.array(pos, dtype=np.int64)


def counts(*a, **k):
    return CG.cell_counts(*a, **k).cpu().numpy()


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int16])
def test_window_edges_and_row_alignment(dtype):
    a = raster(dtype, H0, W0, 1)
    pos = edge_windows(H0, W0)
    for as_uint8 in ((True,) if dtype == np.uint8 else (True, False)):
        want = CO.cell_counts(a, pos, None, 0, as_uint8)
        assert want[:, 0].min() == 0 < want[:, 0].max() and (want[:, 3] == pos[:, 2] * pos[:, 3]).all()
        got = counts(dev(a), pos, as_uint8=as_uint8)
        assert got.dtype == np.int64 and np.array_equal(got, want)
        # the raster inside a buffer that would count everywhere else: strided rows, an unaligned base, head and tail masks
        view = framed(a)
        assert not view.is_contiguous() and view.data_ptr() % 16 != 0
        assert np.array_equal(counts(view, pos, as_uint8=as_uint8), want)


@pytest.mark.parametrize("H,W", [(300, 5000), (5000, 300)])
def test_windows_of_many_passes(H, W):
    a = raster(np.uint8, H, W, 2)
    pos = [(0, 0, 300, 300), (W - 300, H - 300, 300, 300), (7, 0, 293, 300), (0, 0, W, 1), (0, H - 1, W, 1), (3, 5, W - 3, 1),
           (0, 0, 1, H), (W - 1, 0, 1, H), (5, 3, 1, H - 3), (0, 0, W, H)]
    pos = np.array(pos, dtype=np.int64)
    assert sorted(pos[:, 2:].max(axis=0).tolist()) == [300, 5000] and [300, 300] in pos[:, 2:].tolist()
    want = CO.cell_counts(a, pos)
    assert np.array_equal(counts(dev(a), pos), want)
    assert np.array_equal(counts(framed(a), pos), want)


@pytest.mark.parametrize("dtype,values", [(np.uint16, (0, 1, 255, 256, 257, 511, 512, 65535)),
                                          (np.int16, (-32768, -256, -1, 0, 1, 255, 256))])
def test_uint8_wrap_and_thresholds(dtype, values):
    rs = np.random.RandomState(3)
    a = np.array(values, dtype=dtype)[rs.randint(0, len(values), size=(29, 37))]
    a[0, :len(values)] = values
    pos = np.array([(0, 0, 37, 29), (0, 0, len(values), 1), (5, 3, 19, 11), (36, 28, 1, 1)] + [(i, 0, 1, 1) for i in range(len(values))])
    # as the reference sees the values after its cast: numpy's own wrap
    assert np.array([256, 511, 65535], np.uint16).astype(np.uint8).tolist() == [0, 255, 255]
    assert np.array([-1, -256, 300], np.int16).astype(np.uint8).tolist() == [255, 0, 44]
    d = dev(a)
    for as_uint8, thresholds in ((True, (0, 127, 254)), (False, (0, 127, 254, 255, -1))):
        for thr in thresholds:
            want = CO.cell_counts(a, pos, None, thr, as_uint8)
            assert np.array_equal(counts(d, pos, threshold=thr, as_uint8=as_uint8), want), (as_uint8, thr)
    # the two value maps differ where they must
    assert not np.array_equal(CO.cell_counts(a, pos, None, 0, True), CO.cell_counts(a, pos, None, 0, False))


@pytest.mark.parametrize("ta,tb", [(np.uint8, np.int16), (np.uint16, np.uint8), (np.int16, np.uint16), (np.uint8, np.uint8),
                                   (np.uint8, np.uint16), (np.int16, np.uint8)])
def test_two_rasters_of_different_types_and_strides(ta, tb):
    a, b = raster(ta, H0, W0, 4), raster(tb, H0, W0, 5)
    b[20:40, 30:90] = np.where(a[20:40, 30:90].astype(np.uint8) > 0, 7, 0).astype(tb)      # a region where the two masks agree
    pos = np.concatenate([edge_windows(H0, W0)[::5], CG.fishgrid_windows(W0, H0, 16, 14)])
    da = framed(a)                                                     # row stride W + 5, base at element 3 of the buffer's row 1
    db = dev(np.stack([raster(tb, H0, W0 + 1, 6), np.pad(b, ((0, 0), (0, 1)), constant_values=255)]))[1, :, :W0]   # a band, stride W + 1
    assert da.stride(0) != db.stride(0) and db.stride(1) == 1
    for as_uint8 in (True, False):
        want = CO.cell_counts(a, pos, b, 0, as_uint8)
        got = counts(da, pos, other=db, as_uint8=as_uint8)
        assert np.array_equal(got, want)
        assert (want[:, 2] > 0).any() and (want[:, 2] < np.minimum(want[:, 0], want[:, 1])).any()
        if as_uint8:
            cmp_want = CO.compare_cells(a, b, pos, None, (0, 40, 256, 0.3), "iou")
            assert np.array_equal(got[:, 0] + got[:, 1] - 2 * got[:, 2], cmp_want["absdiff"])
            with np.errstate(invalid="ignore", divide="ignore"):
                assert np.array_equal(1 - got[:, 2] / (got[:, 0] + got[:, 1] - got[:, 2]).astype(np.float64), cmp_want["diou"], equal_nan=True)
    # swapped: n_a and n_b change places, n_and stays
    sw = counts(db, pos, other=da)
    assert np.array_equal(sw[:, [1, 0, 2, 3]], CO.cell_counts(a, pos, b))


def test_empty_and_identical_pairs():
    pos = CG.fishgrid_windows(W0, H0, 16, 14)
    z8, z16 = np.zeros((H0, W0), np.uint8), np.zeros((H0, W0), np.uint16)
    got = counts(framed(z8), pos, other=framed(z16))
    assert (got[:, :3] == 0).all() and (got[:, 3] == 256).all()                      # union 0
    res = CG.compare_cells(framed(z8), framed(z16), pos, condition=(0, 0, 256, 0.3))
    assert np.isnan(res["diou"]).all() and not res["isv3"].any() and res["isv2"].all() and not res["isv4"].any()
    a = raster(np.uint8, H0, W0, 7)
    got = counts(framed(a), pos, other=dev(a.astype(np.int16)))
    assert np.array_equal(got[:, 0], got[:, 1]) and np.array_equal(got[:, 0], got[:, 2]) and np.array_equal(got, CO.cell_counts(a, pos, a))
    res = CG.compare_cells(dev(a), dev(a), pos, condition=(0, 0, 256, 0.3))
    filled = got[:, 0] > 0
    assert filled.any() and (res["absdiff"] == 0).all() and (res["diou"][filled] == 0).all() and res["isv4"][filled].all()


@pytest.fixture(scope="module")
def city():
    """the median-city size: a 4000 x 3000 footprint raster, its 3 888 windows of 64 / 56 and their counts"""
    rs = np.random.RandomState(8)
    a = np.zeros((3000, 4000), dtype=np.uint8)
    for _ in range(400):                                              # blobs: most of a city's cells hold no settlement
        x, y = rs.randint(0, 3900), rs.randint(0, 2900)
        a[y:y + rs.randint(5, 120), x:x + rs.randint(5, 120)] = 255
    a[rs.rand(3000, 4000) < 0.3] = 0
    pos = CG.fishgrid_windows(4000, 3000)
    assert pos.shape == (3888, 4)
    return a, pos, CO.cell_counts(a, pos)


def test_one_window_and_a_whole_city(city):
    a, pos, want = city
    d = dev(a)
    got = counts(d, pos)
    assert np.array_equal(got, want) and (want[:, 0] == 0).any() and (want[:, 0] > 2000).any()
    for n in (0, 1234, 3887):
        assert np.array_equal(counts(d, pos[n:n + 1]), want[n:n + 1])               # N = 1
    twice = np.concatenate([pos[-2:], pos[:3], pos[-2:], pos[:3]])                 # repeated windows, as the duplicate corner cell is
    assert np.array_equal(counts(d, twice), np.concatenate([want[-2:], want[:3]] * 2))
    dup = CG.fishgrid_windows(4000 - 16, 3000)                                     # one remainder zero: the reference's duplicate
    assert len(dup) - len(set(map(tuple, dup.tolist()))) == 1 and np.array_equal(counts(d[:, :-16], dup), CO.cell_counts(a[:, :-16], dup))
    stats = CG.fishgrid_stats(d, pos)
    assert np.array_equal(stats["isv"], ((want[:, 0] >= 20) & (want[:, 3] >= 4096)).astype(np.int64)) and 0 < stats["isv"].sum() < 3888
    assert np.array_equal(CG.city_windows(4000, 3000, d), pos[stats["isv"] > 0])


def raw_call(a, type_a, rs_a, b, type_b, rs_b, H, W, pos, N, thr, wrap8, out):
    ptr = lambda t: None if t is None else t.data_ptr()              # noqa: E731
    return _lib.lib().srbh_cell_counts(ptr(a), type_a, rs_a, ptr(b), type_b, rs_b, H, W, ptr(pos), N, thr, wrap8, ptr(out),
                                       _lib.stream_ptr())


def test_output_overwritten_repeatable_and_device_pos(city):
    a, pos, want = city
    d, pos_d = dev(a), torch.from_numpy(pos.astype(np.int32)).to(DEV)
    out = torch.full((len(pos), 4), -0x0123456789abcdef, dtype=torch.int64, device=DEV)          # garbage: every element is overwritten
    _lib.check(raw_call(d, U8, 4000, None, 0, 0, 3000, 4000, pos_d, len(pos), 0, 1, out), "srbh_cell_counts")
    assert np.array_equal(out.cpu().numpy(), want)
    first, second, host = CG.cell_counts(d, pos_d), CG.cell_counts(d, pos_d), CG.cell_counts(d, pos)
    assert first.dtype == torch.int64 and first.is_cuda and torch.equal(first, second) and torch.equal(first, host)
    assert np.array_equal(first.cpu().numpy(), want)


@pytest.mark.parametrize("dtype", [np.uint8, np.int16])
def test_windows_partly_outside_the_raster(dtype):
    """a device pos is used as is: count = the pixels inside the raster, and nothing outside is counted"""
    a = raster(dtype, H0, W0, 9)
    a[:3, :], a[-3:, :], a[:, :17], a[:, -17:] = 1, 1, 1, 1           # the rim counts: a clipped window is not empty
    pos = np.array([(-5, -4, 20, 10), (W0 - 7, H0 - 2, 30, 30), (-16, 10, 17, 5), (-16, 10, 16, 5), (W0, 0, 5, 5), (0, H0, 5, 5),
                    (W0 - 1, H0 - 1, INT_MAX, INT_MAX), (-3, -3, INT_MAX, INT_MAX), (100, 60, INT_MAX, 3), (-INT_MAX, -INT_MAX, INT_MAX, INT_MAX),
                    (-INT_MAX, 0, INT_MAX, 5), (5, 5, 0, 5), (5, 5, 5, 0), (5, 5, -3, 5), (5, 5, 5, -INT_MAX), (-40, 3, W0 + 80, 1),
                    (W0 - 16, 0, 17, H0), (W0 - 15, -1, 16, 2), (0, 0, W0, H0)], dtype=np.int64)
    b = raster(np.uint16, H0, W0, 10)
    want = CO.cell_counts(a, pos, b)
    assert (want[:, 3] == 0).sum() >= 7 and want[7].tolist()[3] == H0 * W0 and (want[:, 0] > 0).sum() >= 8
    pos_d = torch.from_numpy(pos.astype(np.int32)).to(DEV)
    assert np.array_equal(counts(framed(a), pos_d, other=framed(b, 2, 5, 3, 1)), want)
    assert np.array_equal(counts(framed(a), pos_d), CO.cell_counts(a, pos))
    with pytest.raises(ValueError, match="cell_counts.*row 0"):       # the host path refuses them
        CG.cell_counts(dev(a), pos)


def test_fixture_end_to_end(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "g20_city_grid.npz")))
    a, b, pos = dev(g["mask"]), dev(g["other"]), g["pos"]
    W, H, window, offset = (int(v) for v in g["grid"])
    cs, cc = tuple(int(v) for v in g["cond_stats"]), tuple(g["cond_compare"])
    stats = CG.fishgrid_stats(a, pos, cs)
    for k in ("sum", "count", "isv"):
        assert stats[k].dtype == np.int64 and np.array_equal(stats[k], g[k]), k
    for metric in ("absdiff", "iou"):
        for tag, isv in (("", stats["isv"]), ("_all", None)):
            got = CG.compare_cells(a, b, pos, isv, cc, metric)
            for k in ("vrt_sum", "vrt_count", "absdiff", "isv2", "isv3", "isv4"):
                assert np.array_equal(got[k], g[f"{metric}{tag}_{k}"]), (metric, tag, k)
            assert np.array_equal(got["diou"].view(np.int64), g[f"iou{tag}_diou"].view(np.int64)), (metric, tag)
    assert np.isnan(g["iou_all_diou"]).any()
    assert np.array_equal(CG.city_windows(W, H, a, window, offset, cs), g["index_isv"])
    # straight into the tile cutter: every cell of a reference grid is full-size, so every cell batches
    rs = np.random.RandomState(11)
    s2 = dev(rs.randint(0, 9000, size=(6, 150, 200)).astype(np.uint16))
    wsf = np.zeros((150, 200), dtype=np.uint8)
    wsf[10:100, 30:160] = 255
    cells = CG.city_windows(200, 150, dev(wsf))
    assert 0 < len(cells) <= 12 and np.array_equal(cells, CG.valid_windows(g["pos_200x150_64_56"], CO.fishgrid_stats(wsf, g["pos_200x150_64_56"])["isv"]))
    gt = LM.GridTiles(s2, None, cells, np.stack([np.zeros(6), np.full(6, 9000.0)]), None)
    assert len(gt) == len(cells) and tuple(gt[0:len(gt)].shape) == (len(cells), 6, 64, 64)


def test_errors():
    a = raster(np.uint8, H0, W0, 12)
    d, pos = dev(a), np.array([(0, 0, 16, 16)])
    with pytest.raises(RuntimeError, match="no CPU"):
        CG.cell_counts(torch.from_numpy(a), pos)
    with pytest.raises(TypeError, match="float32"):
        CG.cell_counts(d.float(), pos)
    with pytest.raises(TypeError, match="float32"):
        CG.cell_counts(d, pos, other=d.float())
    with pytest.raises(ValueError, match="does not match"):
        CG.cell_counts(d, pos, other=d[:, :-1])
    with pytest.raises(ValueError, match="along W"):
        CG.cell_counts(dev(a.T.copy()).t(), pos)
    with pytest.raises(ValueError, match="along W"):
        CG.cell_counts(d[:, ::2], pos)
    with pytest.raises(ValueError, match=r"\(H, W\)"):
        CG.cell_counts(d[None], pos)
    for bad in ([(0, 0, 16, 0)], [(120, 0, 16, 16)], [(0, 60, 16, 16)], [(-1, 0, 16, 16)], [(0, 0, 16)], np.zeros((0, 4), dtype=np.int64)):
        with pytest.raises(ValueError, match="cell_counts"):
            CG.cell_counts(d, bad)
    with pytest.raises(ValueError, match="int32"):
        CG.cell_counts(d, torch.zeros((1, 4), dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="threshold"):
        CG.cell_counts(d, pos, threshold=70000)
    with pytest.raises(ValueError, match="city_windows"):
        CG.city_windows(W0 + 1, H0, d)
    # the raw C ABI
    pos_d = torch.tensor([[0, 0, 16, 16]], dtype=torch.int32, device=DEV)
    out = torch.zeros((1, 4), dtype=torch.int64, device=DEV)
    good = dict(a=d, type_a=U8, rs_a=W0, b=None, type_b=0, rs_b=0, H=H0, W=W0, pos=pos_d, N=1, thr=0, wrap8=1, out=out)
    assert raw_call(**good) == 0
    for change in (dict(type_a=4), dict(type_a=-1), dict(type_a=F32), dict(b=d, type_b=7, rs_b=W0), dict(b=d, type_b=F32, rs_b=W0),
                   dict(a=None), dict(pos=None), dict(out=None), dict(N=0), dict(H=0), dict(W=0), dict(rs_a=W0 - 1),
                   dict(b=d, type_b=U8, rs_b=W0 - 1), dict(thr=-32769), dict(thr=65536), dict(wrap8=2), dict(H=2 ** 16, W=2 ** 15, rs_a=2 ** 15)):
        rc = raw_call(**{**good, **change})
        assert rc != 0, change
        with pytest.raises(RuntimeError, match="srbh_cell_counts"):
            _lib.check(rc, "srbh_cell_counts")
    torch.cuda.synchronize()
    assert out.cpu().numpy().tolist() == [[int((a[:16, :16] > 0).sum()), 0, 0, 256]]
