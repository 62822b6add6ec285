"""GPU: the city comparison (srbh_pair_sums, srbh_pair_class_sums; city_compare.pair_sums / cell_errors / class_sums / city_validation /
block_errors) against the numpy oracle tests/city_compare_oracle.py.

Everything the kernels return is an integer, so every number is compared EXACTLY; the floats of the host layer are compared bit for bit
(a NaN with a NaN).  The shapes are those of tests/test_gpu_city_summary.py, the smallest at which the kernels can go wrong: a 131-wide
raster (odd: the 16-byte alignment of a row changes from row to row), windows that start at every byte offset of a 16-byte group, all
twelve element-size combinations of (pred, ref, mask), rasters that are interior views of a larger buffer whose every other element is the
LARGEST value (a load or a predicate that left the raster shows as a wrong sum, not as a fault), sums beyond 2^32 of either sign."""
import numpy as np
import pytest
import torch

from srbh_amd import _lib
from srbh_amd import city_compare as CC
from srbh_amd import city_grid as CG
from srbh_amd import city_summary as CS
from srbh_amd.metrics import HeightMetric
from tests import city_compare_oracle as CO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, U16, I16, U8 = 0, 1, 2, 3                           # include/srbh.h SRBH_GRID_*
H0, W0 = CO.H0, CO.W0
INT_MAX = 2 ** 31 - 1
GARBAGE = -0x0123456789abcdef
ERR_ARG = -1                                             # include/srbh.h SRBH_ERR_ARG
SIZES = [(tp, tr, tm) for tp in (np.uint16, np.uint8) for tr in (np.uint16, np.uint8) for tm in (None, np.uint8, np.uint16)]


def dev(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).to(DEV).view(torch.uint16)
    return torch.from_numpy(a).to(DEV)


def framed(a, top=1, left=3, bottom=1, right=2):
    """`a` as an interior view of a larger device buffer whose every other element is the type's largest value (compared at every
    threshold below it, and the largest addend there is); the view starts at an odd element of the buffer"""
    if a is None:
        return None
    H, W = a.shape
    buf = np.full((H + top + bottom, W + left + right), np.iinfo(a.dtype).max, dtype=a.dtype)
    buf[top:top + H, left:left + W] = a
    return dev(buf)[top:top + H, left:left + W]


def framed3(p, r, m):
    """the three rasters as views with strided rows, unaligned bases and a different stride each"""
    fp, fr, fm = framed(p), framed(r, 2, 5, 3, 1), framed(m, 1, 1, 2, 7)
    assert not fp.is_contiguous() and fp.data_ptr() % 16 != 0 and fp.stride(0) != fr.stride(0)
    assert fm is None or len({fp.stride(0), fr.stride(0), fm.stride(0)}) == 3
    return fp, fr, fm


def sums(*a, **k):
    return CC.pair_sums(*a, **k).cpu().numpy()


def classes(*a, **k):
    rows, bad = CC.class_sums(*a, **k)
    assert rows.dtype == torch.int64 and bad.dtype == torch.int64 and bad.dim() == 0
    return rows.cpu().numpy(), int(bad)


# ---- windows ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tp,tr,tm", SIZES)
def test_window_edges_and_row_alignment(tp, tr, tm):
    p, r, m = CO.triple(tp, tr, tm)
    pos = CO.edge_windows(H0, W0)
    pos = np.concatenate([pos, pos[5:9], pos[:3], CG.fishgrid_windows(W0, H0, 16, 14)])                # repeated and overlapping windows
    want = CO.pair_sums(p, r, pos, m)
    assert (want[:, 1] == 0).any() and ((want[:, 1] > 0) & (want[:, 1] < want[:, 0])).any() and (want[:, 0] == pos[:, 2] * pos[:, 3]).all()
    assert (want[:, 2] < 0).any() and (want[:, 2] > 0).any()
    got = sums(dev(p), dev(r), pos, dev(m))
    assert got.dtype == np.int64 and got.shape == (len(pos), 10) and np.array_equal(got, want)
    fp, fr, fm = framed3(p, r, m)
    assert np.array_equal(sums(fp, fr, pos, fm), want)                 # the memory contract
    assert np.array_equal(sums(fp, fr, pos[-1:], fm), want[-1:])       # N = 1


def test_windows_partly_wholly_and_absurdly_outside():
    """a device pos is used as is: count and the sums cover only what lies inside the raster"""
    p, r, m = CO.triple(np.uint16, np.uint8, np.uint8, seed=3)
    pos = np.array([(-5, -4, 20, 10), (W0 - 7, H0 - 2, 30, 30), (-16, 10, 17, 5), (-16, 10, 16, 5), (W0, 0, 5, 5), (0, H0, 5, 5),
                    (W0 - 1, H0 - 1, INT_MAX, INT_MAX), (-3, -3, INT_MAX, INT_MAX), (100, 60, INT_MAX, 3), (-INT_MAX, -INT_MAX, INT_MAX, INT_MAX),
                    (-INT_MAX, 0, INT_MAX, 5), (5, 5, 0, 5), (5, 5, 5, 0), (5, 5, -3, 5), (5, 5, 5, -INT_MAX), (-40, 3, W0 + 80, 1),
                    (W0 - 16, 0, 17, H0), (W0 - 15, -1, 16, 2), (-INT_MAX - 1, -INT_MAX - 1, INT_MAX, INT_MAX), (0, 0, W0, H0)], dtype=np.int64)
    want = CO.pair_sums(p, r, pos, m)
    assert (want[:, 0] == 0).sum() >= 8 and want[7, 0] == H0 * W0 and (want[:, 1] > 0).sum() >= 8
    pos_d = torch.from_numpy(pos.astype(np.int32)).to(DEV)
    fp, fr, fm = framed3(p, r, m)
    assert np.array_equal(sums(fp, fr, pos_d, fm), want)
    assert np.array_equal(sums(fp, fr, pos_d), CO.pair_sums(p, r, pos))
    assert np.array_equal(sums(fr, fm, pos_d, fp), CO.pair_sums(r, m, pos, p))
    with pytest.raises(ValueError, match="pair_sums.*row 0"):         # the host path refuses them
        CC.pair_sums(dev(p), dev(r), pos)


@pytest.fixture(scope="module")
def city():
    """the median-city size: 4000 x 3000 rasters built like predict_city's, a reference near the prediction, the 3 888 windows of 64 / 56"""
    rs = np.random.RandomState(8)
    b = np.zeros((3000, 4000), dtype=np.uint8)
    for _ in range(400):                                              # blobs: most of a city's cells hold no building
        x, y = rs.randint(0, 3900), rs.randint(0, 2900)
        b[y:y + rs.randint(5, 120), x:x + rs.randint(5, 120)] = rs.randint(1, 7)
    h = rs.randint(0, 600, size=b.shape).astype(np.uint16)
    h[(b == 0) & (rs.rand(*b.shape) < 0.9)] = 0                       # (class 0 with a non-zero height stays here and there)
    ref = np.clip(h.astype(np.int32) + rs.randint(-50, 51, size=b.shape), 0, 65535).astype(np.uint16)
    ref[b == 0] = 0
    pos = CG.fishgrid_windows(4000, 3000)
    assert pos.shape == (3888, 4)
    return h, ref, b, pos, CO.pair_sums(h, ref, pos, b)


def test_a_whole_city_overwrite_repeat_and_device_pos(city):
    h, ref, b, pos, want = city
    dh, dr, db = dev(h), dev(ref), dev(b)
    pos_d = torch.from_numpy(pos.astype(np.int32)).to(DEV)
    out = torch.full((len(pos), 10), GARBAGE, dtype=torch.int64, device=DEV)                    # garbage: every element is overwritten
    _lib.check(_lib.lib().srbh_pair_sums(dh.data_ptr(), U16, 4000, dr.data_ptr(), U16, 4000, db.data_ptr(), U8, 4000, 3000, 4000,
                                         pos_d.data_ptr(), len(pos), 0, 0, 0, 0, out.data_ptr(), _lib.stream_ptr()), "srbh_pair_sums")
    assert np.array_equal(out.cpu().numpy(), want) and (want[:, 1] == 0).any() and (want[:, 1] > 2000).any()
    first, second, host = CC.pair_sums(dh, dr, pos_d, db), CC.pair_sums(dh, dr, pos_d, db), CC.pair_sums(dh, dr, pos, db)
    assert first.dtype == torch.int64 and first.is_cuda and torch.equal(first, second) and torch.equal(first, host) and torch.equal(first, out)
    for n in (0, 1234, 3887):
        assert np.array_equal(sums(dh, dr, pos[n:n + 1], db), want[n:n + 1])                      # N = 1
    # the per-cell table of the fishnet
    table, oracle = CC.cell_errors(dh, dr, pos, db), CO.errors(want)
    for k in ("n", "count"):
        assert np.array_equal(table[k], oracle[k]), k
    for k in ("fraction", "me", "mae", "rmse", "mean_pred", "mean_ref", "r", "r2"):
        assert CO.same_bits(table[k], oracle[k]), k
    assert np.isnan(table["rmse"]).any() and (table["rmse"] > 0).any() and (np.nan_to_num(table["r"]) > 0.5).any()
    # identity against the code that already exists: under "pred" the prediction's sums are window_sums'
    mine = CC.pair_sums(dh, dr, pos_d, db, mode="pred")
    assert torch.equal(mine[:, [0, 1, 5, 7]], CS.window_sums(dh, pos_d, db)[:, :4])


# ---- modes and thresholds ---------------------------------------------------------------------------------------------------------------------
def test_modes_and_thresholds():
    p, r, m, pos = CO.threshold_case()
    m16 = r.copy()
    dp, dr, dm, dm16 = dev(p), dev(r), dev(m), dev(m16)
    empty = partial = 0
    for mode in CO.MODES:
        for pthr in (-1, 0, 254, 65535):
            for rthr in (-1, 0, 254, 65535):
                assert np.array_equal(sums(dp, dr, pos, None, mode, pthr, rthr), CO.pair_sums(p, r, pos, None, mode, pthr, rthr)), (mode, pthr, rthr)
                for mthr in (-1, 0, 6, 255):
                    want = CO.pair_sums(p, r, pos, m, mode, pthr, rthr, mthr)
                    assert np.array_equal(sums(dp, dr, pos, dm, mode, pthr, rthr, mthr), want), (mode, pthr, rthr, mthr)
                    empty += int((want[:, 1] == 0).sum())
                    partial += int(((want[:, 1] > 0) & (want[:, 1] < want[:, 0])).sum())
                    if mthr == 255:                                   # an all-uncompared window; count ignores every test
                        assert (want[:, 1:] == 0).all() and want[0, 0] == 37 * 29
                assert np.array_equal(sums(dp, dr, pos, dm16, mode, pthr, rthr, 254), CO.pair_sums(p, r, pos, m16, mode, pthr, rthr, 254))
    assert empty > 0 and partial > 0
    everything = sums(dp, dr, pos, dm, "any", -1, -1, -1)
    assert np.array_equal(everything[:, 0], everything[:, 1]) and np.array_equal(everything, CO.pair_sums(p, r, pos, None, "any", -1, -1))
    both, any_ = sums(dp, dr, pos, mode="both"), sums(dp, dr, pos, mode="any")
    assert (both[:, 1] < any_[:, 1]).any()


# ---- extreme sums -----------------------------------------------------------------------------------------------------------------------------
def test_sums_beyond_32_bits_of_either_sign():
    n, top = 1024 * 1024, 65535
    full, zero = dev(np.full((1024, 1024), top, dtype=np.uint16)), dev(np.zeros((1024, 1024), dtype=np.uint16))
    pos = [(0, 0, 1024, 1024)]
    assert sums(full, zero, pos).tolist() == [[n, n, n * top, n * top, n * top ** 2, n * top, 0, n * top ** 2, 0, 0]]
    assert sums(zero, full, pos).tolist() == [[n, n, -n * top, n * top, n * top ** 2, 0, n * top, 0, n * top ** 2, 0]]      # negative through the shuffle fold
    assert sums(full, full, pos).tolist() == [[n, n, 0, 0, 0, n * top, n * top, n * top ** 2, n * top ** 2, n * top ** 2]]
    assert n * top > 6.8e10 and n * top ** 2 > 4.5e15
    u8 = dev(np.full((1024, 1024), 255, dtype=np.uint8))
    assert sums(u8, full, pos, u8).tolist() == [[n, n, n * (255 - top), n * (top - 255), n * (top - 255) ** 2, n * 255, n * top, n * 255 ** 2,
                                                 n * top ** 2, n * 255 * top]]
    assert sums(full, u8, pos, mode="both", ref_threshold=254).tolist() == [[n, n, n * (top - 255), n * (top - 255), n * (top - 255) ** 2, n * top,
                                                                             n * 255, n * top ** 2, n * 255 ** 2, n * 255 * top]]
    rows, bad = classes(zero, full, CC.DEFAULT_EDGES)                  # the same extremes through the class tables
    assert rows[6, :4].tolist() == [n, -n * top, n * top, n * top ** 2] and rows[6, 4] == n and rows[:6].sum() == 0 and bad == 0
    rows, bad = classes(zero, full, CC.DEFAULT_EDGES, u8)              # ... with every class beyond the table: groups of one value throughout
    assert rows[6, :4].tolist() == [n, -n * top, n * top, n * top ** 2] and rows[:, 4:].sum() == 0 and rows[:6].sum() == 0 and bad == n
    rows, bad = classes(full, u8, CC.DEFAULT_EDGES, dev(np.full((1024, 1024), 3, dtype=np.uint16)))
    assert rows[3, :4].tolist() == [n, n * (top - 255), n * (top - 255), n * (top - 255) ** 2] and rows[3, 4 + 3] == n and bad == 0
    assert rows.sum() == rows[3].sum()


# ---- identities -------------------------------------------------------------------------------------------------------------------------------
def test_identities():
    p, r, m = CO.triple(np.uint16, np.uint16, np.uint8, seed=21)
    dp, dr, dm = dev(p), dev(r), dev(m)
    pos = CO.edge_windows(H0, W0)[::3]
    s = sums(dp, dp, pos, dm)
    assert (s[:, 2:5] == 0).all() and np.array_equal(s[:, 9], s[:, 7]) and np.array_equal(s[:, 8], s[:, 7]) and (s[:, 7] > 0).any()
    for mode in ("any", "both"):
        a, b = sums(dp, dr, pos, dm, mode), sums(dr, dp, pos, dm, mode)
        assert np.array_equal(a[:, 2], -b[:, 2]) and np.array_equal(a[:, [0, 1, 3, 4, 9]], b[:, [0, 1, 3, 4, 9]])
        assert np.array_equal(a[:, [5, 6, 7, 8]], b[:, [6, 5, 8, 7]]) and (a[:, 2] != 0).any()
    for mask in (None, dm):
        assert np.array_equal(sums(dp, dr, pos, mask, "pred")[:, [0, 1, 5, 7]], CS.window_sums(dp, pos, mask).cpu().numpy()[:, :4])
        assert np.array_equal(sums(dp, dr, pos, mask, "ref")[:, [0, 1, 6, 8]], CS.window_sums(dr, pos, mask).cpu().numpy()[:, :4])


# ---- classes ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["7x9", "131x70", "300x300", "zeros"])
def test_class_sums_equal_the_oracle(name):
    p, r, b = CO.class_case(name)
    dp, dr, db = dev(p), dev(r), dev(b)
    fp, fr, fb = framed3(p, r, b)
    H, W = p.shape
    for C, edges in list(CO.CLASS_EDGES.items()) + [(9, CO.EMPTY_CLASS_EDGES)]:
        for build, dbuild, fbuild in ((None, None, None), (b, db, fb)):
            want, want_bad = CO.class_sums(p, r, edges, build)
            got, bad = classes(dp, dr, edges, dbuild)
            assert got.shape == (C, 4 + C) and np.array_equal(got, want) and bad == want_bad, (C, build is None)
            assert got[:, 4:].sum() + bad == got[:, 0].sum() == H * W              # every pixel is compared by default
            if name in ("131x70", "300x300") and C <= 7:
                assert (bad > 0) == (build is not None)                # build holds values >= C: counted, in no column of cm
            if C == 9 and name in ("131x70", "300x300"):
                assert got[6, 0] == 0 and (got[6] == 0).all() and (got[[5, 7], 0] > 0).all()       # a class with no pixel
            # a NaN-patterned workspace and out, the elements behind them intact; strided views; two calls bit-equal
            need = _lib.lib().srbh_pair_class_ws_bytes(H, W, C)
            ws = torch.full((need // 8 + 2,), float("nan"), dtype=torch.float64, device=DEV)
            again, bad2 = classes(fp, fr, edges, fbuild, workspace=ws)
            assert np.array_equal(again, want) and bad2 == want_bad and torch.isnan(ws[need // 8:]).all()
            # the sum over the classes is the whole raster's pair_sums row of the same selection
            whole = sums(dp, dr, [(0, 0, W, H)], None, "any", -1, -1)
            assert got[:, :4].sum(0).tolist() == whole[0, 1:5].tolist()
    # a selection: the reference's built pixels under the class mask
    for mode, pthr, rthr, mthr in (("ref", -1, 0, -1), ("both", 0, 0, 0), ("any", 29, 30, 2), ("pred", 30, -1, 6)):
        want, want_bad = CO.class_sums(p, r, CO.CLASS_EDGES[7], b, mode, pthr, rthr, mthr)
        got, bad = classes(dp, dr, CO.CLASS_EDGES[7], db, mode, pthr, rthr, mthr)
        assert np.array_equal(got, want) and bad == want_bad, mode
        assert got[:, :4].sum(0).tolist() == sums(dp, dr, [(0, 0, W, H)], db, mode, pthr, rthr, mthr)[0, 1:5].tolist()
    if name == "300x300":                                             # raw call: out is overwritten and nothing behind it is touched
        C, edges = 7, CO.CLASS_EDGES[7]
        out = torch.full((C * (4 + C) + 3,), float("nan"), dtype=torch.float64, device=DEV).view(torch.int64)
        ws = torch.empty(_lib.lib().srbh_pair_class_ws_bytes(H, W, C) // 8, dtype=torch.int64, device=DEV)
        import ctypes
        _lib.check(_lib.lib().srbh_pair_class_sums(dp.data_ptr(), U16, W, dr.data_ptr(), U16, W, db.data_ptr(), U8, W, H, W,
                                                   (ctypes.c_int * C)(*edges), C, 0, -1, -1, -1, out.data_ptr(), ws.data_ptr(),
                                                   _lib.stream_ptr()), "srbh_pair_class_sums")
        want, want_bad = CO.class_sums(p, r, edges, b)
        assert np.array_equal(out[:-3].cpu().numpy(), want.reshape(-1)) and int(out[-3]) == want_bad
        assert torch.isnan(out.view(torch.float64)[-2:]).all()


@pytest.mark.parametrize("tp,tr,tm", SIZES)
def test_class_sums_every_element_size(tp, tr, tm):
    p, r, m = CO.triple(tp, tr, tm, seed=31)
    p, r = (p.astype(np.int64) % 1000).astype(tp), (r.astype(np.int64) % 1000).astype(tr)      # heights around the edges
    b = None if tm is None else (m.astype(np.int64) % 9).astype(tm)
    want, want_bad = CO.class_sums(p, r, CO.CLASS_EDGES[7], b)
    fp, fr, fb = framed3(p, r, b)
    assert (want[:, 0] > 0).sum() >= 4 and (b is None or want_bad > 0)
    got, bad = classes(fp, fr, CO.CLASS_EDGES[7], fb)
    assert np.array_equal(got, want) and bad == want_bad


# ---- the Python layer end to end ----------------------------------------------------------------------------------------------------------------
def test_city_validation_and_block_errors():
    rs = np.random.RandomState(16)
    H, W = 150, 200
    ref = np.round(10 * rs.gamma(2.0, 6.0, size=(H, W))).astype(np.uint16)
    ref[rs.rand(H, W) < 0.8] = 0                                       # the label histogram: mostly zeros
    height = np.clip(ref.astype(np.int32) + rs.randint(-40, 41, size=(H, W)), 0, 65535).astype(np.uint16)
    height[(ref == 0) & (rs.rand(H, W) < 0.9)] = 0
    build = CO.class_of(height, CC.DEFAULT_EDGES).astype(np.uint8)
    build[rs.rand(H, W) < 0.1] = rs.randint(0, 7)
    dh, dr, db = dev(height), dev(ref), dev(build)
    for b_np, b_dev in ((build, db), (None, None)):
        got = CC.city_validation(dh, dr, b_dev)
        rows, bad = CO.class_sums(height, ref, CC.DEFAULT_EDGES, b_np)
        stats, count, cm = CO.metric_tables(rows)
        assert got["bad"] == bad == 0
        hm = HeightMetric(7, device=DEV)
        hm.stats += torch.from_numpy(stats).to(DEV)
        hm.count += torch.from_numpy(count).to(DEV)
        assert torch.equal(got["height"].getAvgEach(), hm.getAvgEach()) and torch.equal(got["height"].getCount(), hm.getCount())
        assert CO.same_bits(got["height"].stats.cpu().numpy(), stats) and (stats[:, 0] > 0).sum() >= 5
        assert np.array_equal(got["seg"].getConfusionMatrix().cpu().numpy(), cm) and cm.sum() == H * W
        assert np.array_equal(cm, np.bincount(CO.class_of(ref, CC.DEFAULT_EDGES).reshape(-1) * 7 + (CO.class_of(height, CC.DEFAULT_EDGES) if b_np is None
                                                                                                   else b_np.astype(np.int64)).reshape(-1),
                                              minlength=49).reshape(7, 7))
        whole = CO.errors(CO.pair_sums(height, ref, [(0, 0, W, H)], None, "any", -1, -1))
        for k, v in whole.items():
            assert CO.same_bits(got["sums"][k].astype(np.float64), v.astype(np.float64)), k
        assert got["sums"]["n"][0] == H * W and got["sums"]["r"][0] > 0.5
    build[5, 7] = 9                                                   # a class beyond the table: counted, flagged where the scores are read
    got = CC.city_validation(dh, dr, dev(build))
    assert got["bad"] == 1 and got["seg"].confusionMatrix.sum().item() == H * W - 1 and got["height"].getCount().sum().item() == H * W
    with pytest.raises(ValueError, match="outside"):
        got["seg"].getConfusionMatrix()
    # the aggregated scale.  The terms e_b = D_b / n_b, mp_b, mr_b are ONE correctly rounded float64 division of exact integers below 2^53
    # on both sides, so the terms of every sum are bit-equal and only the ORDER of the float64 additions differs: a float64 sum of k
    # terms in any order lies within k 2^-53 sum |terms| of the exact sum (the oracle adds them with math.fsum: exactly).
    mask = (build > 0).astype(np.uint8)
    for block in (4, 40):
        for m_np, m_dev in ((None, None), (mask, dev(mask))):
            got, want = CC.block_errors(dh, dr, block, m_dev), CO.block_errors(height, ref, block, m_np)
            k = want["n_blocks"]
            assert int(got["n_blocks"]) == k > 0 and got["sums"].dtype == torch.float64 and got["sums"].is_cuda
            s = got["sums"].cpu().numpy()
            bound = k * 2.0 ** -53 * want["abs_sums"]
            assert (np.abs(s - want["sums"]) <= bound).all(), (block, s, want["sums"])
            # the measures follow from the sums by a division (correctly rounded) and a square root (faithful: within 1 ulp)
            me, mae, rmse = s[0] / k, s[1] / k, np.sqrt(s[2] / k)
            r = (k * s[7] - s[3] * s[4]) / np.sqrt((k * s[5] - s[3] * s[3]) * (k * s[6] - s[4] * s[4]))
            assert got["me"].item() == me and got["mae"].item() == mae
            assert abs(got["rmse"].item() - rmse) <= 2 * np.spacing(rmse) and abs(got["r"].item() - r) <= 4 * np.spacing(abs(r))
            assert abs(rmse - want["rmse"]) < 1e-9 * want["rmse"] and abs(r - want["r"]) < 1e-9 and want["r"] > 0.5


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_c_abi_refusals_launch_nothing():
    import ctypes
    p, r, m = CO.triple(np.uint16, np.uint16, np.uint8, seed=17)
    dp, dr, dm = dev(p), dev(r), dev(m)
    pos_d = torch.tensor([[0, 0, 16, 16]], dtype=torch.int32, device=DEV)
    lib, ptr = _lib.lib(), (lambda t: None if t is None else t.data_ptr())
    E7 = CO.CLASS_EDGES[7]
    common = dict(p=dp, tp=U16, rsp=W0, r=dr, tr=U16, rsr=W0, m=dm, tm=U8, rsm=W0, H=H0, W=W0, mode=0, pthr=0, rthr=0, mthr=0)
    outs = {"win": torch.full((1, 10), GARBAGE, dtype=torch.int64, device=DEV), "cls": torch.full((7 * 11 + 1,), GARBAGE, dtype=torch.int64, device=DEV)}
    ws = torch.zeros(lib.srbh_pair_class_ws_bytes(H0, W0, 7), dtype=torch.uint8, device=DEV)

    def lead(a):
        return (ptr(a["p"]), a["tp"], a["rsp"], ptr(a["r"]), a["tr"], a["rsr"], ptr(a["m"]), a["tm"], a["rsm"], a["H"], a["W"])

    def win(a):
        return lib.srbh_pair_sums(*lead(a), ptr(a.get("pos", pos_d)), a.get("N", 1), a["mode"], a["pthr"], a["rthr"], a["mthr"],
                                  ptr(a.get("out", outs["win"])), _lib.stream_ptr())

    def cls(a):
        e = a.get("edges", E7)
        return lib.srbh_pair_class_sums(*lead(a), None if e is None else (ctypes.c_int * len(e))(*e), a.get("C", 7), a["mode"], a["pthr"], a["rthr"],
                                        a["mthr"], ptr(a.get("out", outs["cls"])), ptr(a.get("ws", ws)), _lib.stream_ptr())

    odd16 = dev(m.astype(np.uint16)).view(torch.uint8)[:, 1:]
    shared = [dict(tp=I16), dict(tp=F32), dict(tp=4), dict(tp=-1), dict(tr=I16), dict(tr=F32), dict(tr=9), dict(tm=I16), dict(tm=F32), dict(tm=9),
              dict(p=None), dict(r=None), dict(out=None), dict(H=0), dict(W=0), dict(H=-3), dict(rsp=W0 - 1), dict(rsr=W0 - 1), dict(rsm=W0 - 1),
              dict(H=2 ** 16, W=2 ** 15, rsp=2 ** 15, rsr=2 ** 15, rsm=2 ** 15), dict(pthr=-2), dict(pthr=65536), dict(rthr=-2), dict(rthr=65536),
              dict(mthr=-2), dict(mthr=65536), dict(mode=-1), dict(mode=4), dict(p=dp.view(torch.uint8)[:, 1:]), dict(r=dr.view(torch.uint8)[:, 1:]),
              dict(m=odd16, tm=U16)]
    own = {"srbh_pair_sums": (win, [dict(pos=None), dict(N=0), dict(N=-1)]),
           "srbh_pair_class_sums": (cls, [dict(ws=None), dict(edges=None), dict(C=1), dict(C=17, edges=tuple(range(17))), dict(C=0),
                                          dict(edges=(1, 30, 120, 210, 300, 600, 900)), dict(edges=(0, 30, 30, 210, 300, 600, 900)),
                                          dict(edges=(0, 30, 120, 210, 300, 900, 600)), dict(ws=ws[4:]), dict(out=outs["cls"].view(torch.int32)[1:])])}
    for name, (call, extra) in own.items():
        for change in shared + extra:
            rc = call({**common, **change})
            assert rc == ERR_ARG, (name, change)
            with pytest.raises(RuntimeError, match=name):
                _lib.check(rc, name)
    torch.cuda.synchronize()
    for out in outs.values():                                         # nothing was launched: the garbage stands
        assert (out == GARBAGE).all()
    assert win(common) == 0 and cls({**common, "mthr": -1, "pthr": -1, "rthr": -1}) == 0
    assert np.array_equal(outs["win"].cpu().numpy(), CO.pair_sums(p, r, [(0, 0, 16, 16)], m))
    rows, bad = CO.class_sums(p, r, E7, m)
    assert np.array_equal(outs["cls"].cpu().numpy(), np.concatenate([rows.reshape(-1), [bad]]))
    # a null third raster makes its type code and stride irrelevant
    assert win({**common, "m": None, "tm": 99, "rsm": 0}) == 0
    assert np.array_equal(outs["win"].cpu().numpy(), CO.pair_sums(p, r, [(0, 0, 16, 16)]))
    # the Python layer on device tensors: a short workspace, a wrong pos
    with pytest.raises(ValueError, match="workspace"):
        CC.class_sums(dp, dr, E7, workspace=torch.empty(16, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="int32"):
        CC.pair_sums(dp, dr, torch.zeros((1, 4), dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU"):
        CC.block_errors(torch.from_numpy(m), torch.from_numpy(m), 4)
