"""CPU: the host side of the inference tile cutter -- tests/grid_oracle.py against what the reference's own gridimgLoader.__getitem__
returned (tests/golden/g18_grid_tiles.npz, tools/make_golden_grid.py), and loader_math.grid_windows / check_windows."""
import os

import numpy as np
import pytest

from srbh_amd import loader_math as LM
from tests import grid_oracle as GO


@pytest.fixture(scope="module")
def g18(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g18_grid_tiles.npz")))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def test_oracle_reproduces_every_stored_image_bit_for_bit(g18):
    nchans, tile, wins = int(g18["nchans"]), int(g18["tile"]), g18["windows"]
    assert len(wins) >= 12 and g18["s2"].dtype == np.uint16 and g18["s1"].dtype == np.float32
    kinds = set()
    for i, w in enumerate(wins):
        img = g18[f"img_{i}"]
        assert np.array_equal(g18[f"pos_{i}"], w)
        assert img.dtype == np.float32 and img.shape == (nchans + 2, w[3], w[2])
        got = GO.cell(g18["s2"], g18["s1"], w, g18["s2_stats"], g18["s1_stats"], nchans)
        assert np.array_equal(_bits(got), _bits(img)), f"window {i}"
        # the float64-then-round form IS the statement: rounding cell64 gives the same bits
        c64 = GO.cell64(g18["s2"], g18["s1"], w, g18["s2_stats"], g18["s1_stats"], nchans)
        assert c64.dtype == np.float64 and np.array_equal(_bits(c64.astype(np.float32)), _bits(img))
        t = GO.tile(g18["s2"], g18["s1"], w, g18["s2_stats"], g18["s1_stats"], nchans, tile)
        assert t.shape == (nchans + 2, tile, tile)
        assert np.array_equal(_bits(t[:, :w[3], :w[2]]), _bits(img))
        outside = np.ones((tile, tile), dtype=bool)
        outside[:w[3], :w[2]] = False
        assert not _bits(t)[:, outside].any(), f"window {i}: outside the window a tile is +0.0 (all bits clear)"
        kinds.add((w[2] == tile, w[3] == tile, bool(w[0] % 2), w[0] + w[2] == g18["s2"].shape[2], w[1] + w[3] == g18["s2"].shape[1]))
    assert any(k[0] and k[1] for k in kinds) and any(not k[0] and k[3] for k in kinds) and any(not k[1] and k[4] for k in kinds)
    assert any(k[2] for k in kinds) and any(tuple(w[2:]) == (1, 1) for w in wins)


GRIDS = [(24, 20, 8, 8), (26, 20, 8, 6), (8, 8, 8, 8), (5, 7, 8, 6), (208, 208, 64, 48)]


@pytest.mark.parametrize("w,h,cell,stride", GRIDS, ids=lambda v: str(v))
def test_grid_windows_cover_the_raster_without_redundant_cells(w, h, cell, stride):
    pos = LM.grid_windows(w, h, cell, stride)
    assert pos.dtype == np.int64 and pos.ndim == 2 and pos.shape[1] == 4
    cover = np.zeros((h, w), dtype=np.int64)
    for x, y, xc, yc in pos:
        cover[y:y + yc, x:x + xc] += 1
    assert cover.min() >= 1
    assert np.array_equal(LM.check_windows(pos, w, h, cell), pos)
    for starts, counts, length in ((pos[:, 0], pos[:, 2], w), (pos[:, 1], pos[:, 3], h)):
        assert np.array_equal(counts, np.minimum(cell, length - starts))
        for s in np.unique(starts):
            assert s % stride == 0 and s < length
            assert s == 0 or s + cell - stride < length, f"start {s} holds no pixel its predecessor lacks"
        # and none that the rule keeps is missing
        assert sorted(np.unique(starts)) == [k for k in range(0, length, stride) if k == 0 or k + cell - stride < length]
    # row-major: y outer, x inner
    nx = len(np.unique(pos[:, 0]))
    assert np.array_equal(pos[:, 0], np.tile(np.unique(pos[:, 0]), len(pos) // nx))
    assert np.array_equal(pos[:, 1], np.repeat(np.unique(pos[:, 1]), nx))


def test_grid_windows_stride_48_is_the_sharded_citys_layout():
    pos = LM.grid_windows(208, 208, 64, 48)
    assert pos.tolist() == [[(i % 4) * 48, (i // 4) * 48, 64, 64] for i in range(16)]      # test_gpu_predict_sharded._city(n, 4)


def test_grid_windows_defaults_and_bad_arguments():
    assert LM.grid_windows(130, 64).tolist() == [[0, 0, 64, 64], [64, 0, 64, 64], [128, 0, 2, 64]]
    for bad in ((0, 8, 8, 8), (8, 0, 8, 8), (8, 8, 8, 0), (8, 8, 8, 9)):
        with pytest.raises(ValueError, match="grid_windows"):
            LM.grid_windows(*bad)


BAD_WINDOWS = {
    "negative offset": [-1, 0, 4, 4],
    "negative y offset": [0, -2, 4, 4],
    "count 0": [0, 0, 0, 4],
    "y count 0": [0, 0, 4, 0],
    "count above the tile": [0, 0, 9, 4],
    "y count above the tile": [0, 0, 4, 12],
    "past the right edge": [20, 0, 8, 8],
    "past the bottom edge": [0, 14, 8, 8],
}


@pytest.mark.parametrize("what", list(BAD_WINDOWS))
def test_check_windows_names_the_first_offending_row(what):
    good = [[0, 0, 8, 8], [19, 12, 8, 8], [26, 19, 1, 1]]
    assert LM.check_windows(good, 27, 20, 8).tolist() == good
    pos = good[:2] + [BAD_WINDOWS[what]] + good[2:] + [[-5, -5, 0, 0]]
    with pytest.raises(ValueError, match=r"row 2 ") as e:
        LM.check_windows(pos, 27, 20, 8)
    assert "check_windows" in str(e.value)


def test_check_windows_refuses_other_shapes():
    for bad in ([[0, 0, 8]], [0, 0, 8, 8], [[0.0, 0.0, 8.0, 8.0]]):
        with pytest.raises(ValueError, match="check_windows"):
            LM.check_windows(bad, 27, 20, 8)
    assert LM.check_windows(np.zeros((0, 4), dtype=np.int64), 27, 20, 8).shape == (0, 4)
