"""CPU: the city grid's host half -- city_grid.fishgrid_windows, the flag arithmetic (stats_from_counts, compare_from_counts,
valid_windows) and the numpy oracle tests/city_grid_oracle.py -- against what the reference's own Fishgridnew_bound, Fishgrid_stats,
compare_twotiff_valid(_iou) and generateindex produced (tests/golden/g20_city_grid.npz, tools/make_golden_city_grid.py).  No kernel
is launched here: the flag functions are fed the counts the oracle forms from the stored rasters."""
import os

import numpy as np
import pytest

from srbh_amd import city_grid as CG
from srbh_amd.loader_math import check_windows
from tests import city_grid_oracle as CO

INTS = ("vrt_sum", "vrt_count", "absdiff", "isv2", "isv3", "isv4")
# (width, height, window, offset): both remainders zero; one non-zero each way (the duplicate corner); both non-zero; window == width
# (and == height); offset == window; offset 1; the inference layout; the fixture's layout
SWEEP = [(176, 120, 64, 56), (64, 64, 64, 56), (65, 64, 64, 56), (64, 65, 64, 56), (177, 120, 64, 56), (176, 121, 64, 56),
         (200, 150, 64, 56), (64, 200, 64, 56), (200, 64, 64, 56), (128, 192, 64, 64), (130, 70, 64, 64), (20, 18, 16, 1),
         (300, 257, 64, 48), (131, 70, 16, 14), (33, 47, 8, 5), (9, 9, 1, 1)]


@pytest.fixture(scope="module")
def g20(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g20_city_grid.npz")))


def _same_bits(a, b):
    return a.dtype == b.dtype == np.float64 and np.array_equal(a.view(np.int64), b.view(np.int64))


def test_layout_equals_the_reference_lists(g20):
    W, H, window, offset = (int(v) for v in g20["grid"])
    for f in (CG.fishgrid_windows, CO.fishgrid_windows):
        assert np.array_equal(f(W, H, window, offset), g20["pos"]) and np.array_equal(g20["index_all"], g20["pos"])
        assert np.array_equal(f(200, 150, 64, 56), g20["pos_200x150_64_56"]) and len(g20["pos_200x150_64_56"]) == 12
        assert np.array_equal(f(65, 64, 64, 56), g20["pos_65x64_64_56"])
    dup = g20["pos_65x64_64_56"]
    assert len(dup) == 3 and np.array_equal(dup[1], dup[2])          # the corner cell written twice
    assert CG.fishgrid_windows(W, H, window, offset).dtype == np.int64


def test_oracle_equals_the_reference_fields(g20):
    a, b, pos = g20["mask"], g20["other"], g20["pos"]
    stats = CO.fishgrid_stats(a, pos, tuple(g20["cond_stats"]))
    for k in ("sum", "count", "isv"):
        assert np.array_equal(stats[k], g20[k]), k
    cond = tuple(g20["cond_compare"])
    for metric in ("absdiff", "iou"):
        for tag, isv in (("", g20["isv"]), ("_all", np.ones(len(pos), dtype=np.int64))):
            key = f"{metric}{tag}_"
            assert np.array_equal(g20[key + "set"], isv != 0)
            got = CO.compare_cells(a, b, pos, isv, cond, metric)
            for k in INTS:
                assert np.array_equal(got[k], g20[key + k]), (key, k)
            if metric == "iou":
                assert _same_bits(got["diou"], g20[key + "diou"]), key
    assert np.isnan(g20["iou_all_diou"]).any() and not g20["iou_all_isv3"][np.isnan(g20["iou_all_diou"])].any()


def test_flag_functions_on_stored_counts(g20):
    """stats_from_counts / compare_from_counts / valid_windows fed the counts of the stored rasters: no device"""
    a, b, pos = g20["mask"], g20["other"], g20["pos"]
    counts = CO.cell_counts(a, pos, b, 0, True)
    assert np.array_equal(counts[:, 0], g20["sum"]) and np.array_equal(counts[:, 3], g20["count"])
    stats = CG.stats_from_counts(counts, tuple(g20["cond_stats"]))
    for k in ("sum", "count", "isv"):
        assert stats[k].dtype == np.int64 and np.array_equal(stats[k], g20[k]), k
    assert np.array_equal(CG.valid_windows(pos, stats["isv"]), g20["index_isv"])
    assert np.array_equal(CG.valid_windows(pos, np.ones(len(pos))), g20["index_all"])
    cond = tuple(g20["cond_compare"])
    for metric in ("absdiff", "iou"):
        for tag, isv in (("", g20["isv"]), ("_all", None)):
            key = f"{metric}{tag}_"
            got = CG.compare_from_counts(counts, isv, cond, metric)
            for k in INTS:
                assert got[k].dtype == np.int64 and np.array_equal(got[k], g20[key + k]), (key, k)
            want = g20["iou" + tag + "_diou"]                        # (diou is formed for both metrics; the reference stores it for one)
            assert _same_bits(got["diou"], want), key
            assert np.array_equal(np.isnan(got["diou"][g20[key + "set"]]), (counts[g20[key + "set"], 0] + counts[g20[key + "set"], 1]) == 0)
    with pytest.raises(ValueError, match="metric"):
        CG.compare_from_counts(counts, None, cond, "rmse")
    with pytest.raises(ValueError, match="isv"):
        CG.compare_from_counts(counts, np.ones(3), cond, "iou")
    with pytest.raises(ValueError, match="flags"):
        CG.valid_windows(pos, np.ones(3))


def test_zero_union_is_nan_and_fails_isv3():
    counts = np.array([[0, 0, 0, 256], [256, 256, 256, 256], [100, 100, 50, 256]], dtype=np.int64)
    got = CG.compare_from_counts(counts, None, (0, 0, 256, 0.3), "iou")
    assert np.isnan(got["diou"][0]) and got["diou"][1] == 0.0 and got["diou"][2] == 1 - 50 / 150.0
    assert got["isv3"].tolist() == [0, 1, 0] and got["isv2"].tolist() == [1, 1, 1] and got["isv4"].tolist() == [0, 1, 0]
    got = CG.compare_from_counts(counts, None, (0, 0, 256, 0.3), "absdiff")
    assert got["absdiff"].tolist() == [0, 0, 100] and got["isv3"].tolist() == [1, 1, 0]


@pytest.mark.parametrize("W,H,window,offset", SWEEP)
def test_layout_sweep(W, H, window, offset):
    pos = CG.fishgrid_windows(W, H, window, offset)
    assert pos.dtype == np.int64 and np.array_equal(pos, CO.fishgrid_windows(W, H, window, offset))
    assert (pos[:, 2:] == window).all() and (pos[:, :2] >= 0).all()
    assert (pos[:, 0] + window <= W).all() and (pos[:, 1] + window <= H).all()
    cover = np.zeros((H, W), dtype=np.int64)
    for x, y, w, h in pos.tolist():
        cover[y:y + h, x:x + w] += 1
    assert (cover > 0).all()
    rem_c, rem_r = (W - window) % offset, (H - window) % offset
    dups = len(pos) - len(set(map(tuple, pos.tolist())))
    assert dups == (1 if (rem_c > 0) != (rem_r > 0) else 0)
    uniq = CG.fishgrid_windows(W, H, window, offset, unique=True)
    assert len(uniq) == len(pos) - dups and len(set(map(tuple, uniq.tolist()))) == len(uniq)
    first = sorted({tuple(r): i for i, r in reversed(list(enumerate(pos.tolist())))}.values())
    assert np.array_equal(uniq, pos[first])                           # the first of every repeat, order kept
    assert np.array_equal(check_windows(pos, W, H, tile=window), pos)


def test_sweep_covers_every_remainder_case():
    rem = {((W - w) % o > 0, (H - w) % o > 0) for W, H, w, o in SWEEP}
    assert rem == {(False, False), (True, False), (False, True), (True, True)}
    assert any(W == w for W, H, w, o in SWEEP) and any(H == w for W, H, w, o in SWEEP) and any(o == w for W, H, w, o in SWEEP)


def test_median_city_size():
    pos = CG.fishgrid_windows(4000, 3000)
    assert pos.shape == (3888, 4) and np.array_equal(pos, CO.fishgrid_windows(4000, 3000))


@pytest.mark.parametrize("args", [(63, 64, 64, 56), (64, 63, 64, 56), (200, 150, 64, 0), (200, 150, 64, 65), (200, 150, 64, -3)])
def test_layout_refuses_what_the_reference_cannot_place(args):
    with pytest.raises(ValueError, match="fishgrid_windows"):
        CG.fishgrid_windows(*args)
