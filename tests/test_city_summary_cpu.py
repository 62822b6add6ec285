"""CPU: the host half of the city summary -- city_summary.heights_from_sums against fractions.Fraction arithmetic bit for bit, the
numpy oracle tests/city_summary_oracle.py against itself (block form == window form), the bin arithmetic of srbh_value_hist for every
uint16 value, the C ABI's declarations, and every refusal the Python layer can make without a device.  No kernel is launched here."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from srbh_amd import _lib
from srbh_amd import city_summary as CS
from srbh_amd.loader_math import grid_windows
from tests import city_summary_oracle as SO

ENTRIES = ("srbh_window_sums", "srbh_block_sums", "srbh_value_hist", "srbh_value_hist_ws_bytes", "srbh_value_hist_magic")


def u16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).view(torch.uint16)


def rows_of(values_per_window, count=None):
    """(N, 5) [count, n, sum, sumsq, max] of lists of selected values, in Python integers"""
    return np.array([[count or max(len(v), 1), len(v), sum(v), sum(t * t for t in v), max(v) if v else 0] for v in values_per_window],
                    dtype=np.int64)


def test_heights_from_sums_against_fractions_bit_for_bit():
    rs = np.random.RandomState(1)
    wins = [[], [7] * 300, [65535] * 2 ** 16, [65534, 65535], [65534] * 1000 + [65535] * 1001, [0, 0, 0], [1], [3, 4],
            rs.randint(0, 65536, size=4096).tolist(), rs.randint(0, 300, size=777).tolist()]
    sums = rows_of(wins, count=2 ** 17)
    got, want = CS.heights_from_sums(sums), SO.heights(sums)
    for k in ("n", "count", "max"):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), k
    for k in ("fraction", "mean", "std"):
        assert got[k].dtype == np.float64 and SO.same_bits(got[k], want[k]), k
    assert math.isnan(got["mean"][0]) and math.isnan(got["std"][0]) and got["fraction"][0] == 0.0            # n == 0
    assert got["std"][1] == 0.0 and got["mean"][1] == 7.0                                                     # a constant window
    assert got["std"][2] == 0.0 and got["mean"][2] == 65535.0 and got["max"][2] == 65535                      # the extreme
    assert got["std"][3] == 0.5 and got["mean"][3] == 65534.5                                                 # {65534, 65535}
    # ... where the float64 one-pass form cancels: it does not give the true value, the integer form does
    n, s, q = (int(v) for v in sums[4, 1:4])
    exact = math.sqrt(float(Fraction(q, n) - Fraction(s, n) ** 2))
    assert got["std"][4] == exact and abs(exact - 0.5) < 1e-6
    assert math.sqrt(max(q / n - (s / n) ** 2, 0.0)) != exact
    # count == 0 (a window wholly outside the raster)
    out = CS.heights_from_sums(np.zeros((1, 5), dtype=np.int64))
    assert all(math.isnan(out[k][0]) for k in ("fraction", "mean", "std")) and out["n"][0] == out["count"][0] == 0
    for bad in (np.zeros((3, 4), dtype=np.int64), np.zeros((2, 5), dtype=np.float64), np.zeros(5, dtype=np.int64)):
        with pytest.raises(ValueError, match="heights_from_sums"):
            CS.heights_from_sums(bad)


@pytest.mark.parametrize("H,W", [(70, 131), (64, 64)])
@pytest.mark.parametrize("block", [1, 3, 4, 5, 40, 64, 400])
def test_oracle_block_form_equals_window_form(H, W, block):
    rs = np.random.RandomState(2)
    v = rs.randint(0, 65536, size=(H, W)).astype(np.uint16)
    v[rs.rand(H, W) < 0.4] = 0
    m = rs.randint(0, 7, size=(H, W)).astype(np.uint8)
    cell = min(block, max(H, W))                                      # (grid_windows clips; a block beyond the raster is the raster)
    pos = grid_windows(W, H, cell, cell)
    blocks = SO.block_sums(v, block, m)
    assert blocks.shape == (4, -(-H // block), -(-W // block)) and len(pos) == blocks[0].size
    assert np.array_equal(blocks.reshape(4, -1).T, SO.window_sums(v, pos, m)[:, 1:])
    agg = SO.aggregate(v, block, m)
    assert np.array_equal(agg["count"].reshape(-1), pos[:, 2] * pos[:, 3]) and agg["count"].sum() == H * W


@pytest.mark.parametrize("bin_width", [1, 3, 10, 255, 256, 65535])
def test_bin_arithmetic_for_every_uint16(bin_width):
    """the kernel's division: (v * M) >> 32 with the library's own M, for all 65 536 values; and the clamp to the last bin"""
    v = np.arange(65536, dtype=np.uint64)
    magic = _lib.lib().srbh_value_hist_magic(bin_width)
    if bin_width == 1:
        assert magic == 0                                              # stands for "the quotient is v"
        q = v
    else:
        assert magic == 2 ** 32 // bin_width + 1
        q = (v * np.uint64(magic)) >> np.uint64(32)
    assert np.array_equal(q, v // np.uint64(bin_width))
    for nbins in (1, 7, 256, 4096):
        b = SO.bin_index(v, bin_width, nbins)
        assert b.min() == 0 and b.max() == min(65535 // bin_width, nbins - 1) and (np.diff(b) >= 0).all()
        assert np.array_equal(b, np.minimum(q.astype(np.int64), nbins - 1))
        img = v.astype(np.uint16).reshape(256, 256)
        h = SO.value_hist(img, bin_width, nbins, None, -1)
        assert h.sum() == 65536 and h[0] == (65536 if nbins == 1 else bin_width)


def test_magic_refuses_what_it_cannot_divide_by():
    for bad in (0, -1, 65536, 2 ** 31 - 1):
        assert _lib.lib().srbh_value_hist_magic(bad) == 0
    assert _lib.lib().srbh_value_hist_ws_bytes(0, 5, 7) == 0 and _lib.lib().srbh_value_hist_ws_bytes(5, 5, 4097) == 0
    assert _lib.lib().srbh_value_hist_ws_bytes(2 ** 16, 2 ** 15, 7) == 0
    assert _lib.lib().srbh_value_hist_ws_bytes(70, 131, 256) % (256 * 4) == 0 < _lib.lib().srbh_value_hist_ws_bytes(70, 131, 256)


def test_declared_exported_and_built():
    assert "srbh_summary.hip" in _lib.SOURCES and os.path.exists(os.path.join(_lib.CSRC, "srbh_summary.hip"))
    header = open(os.path.join(_lib.INCLUDE, "srbh.h")).read()
    lib = _lib.lib()
    for name in ENTRIES:
        assert name + "(" in header and name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
    import srbh_amd
    import srbh_amd.city_summary as mod                                 # the alias package resolves the new module
    assert mod is CS and os.path.dirname(mod.__file__) == srbh_amd.__path__[0]


def test_python_layer_refusals_without_a_device():
    a16, a8 = u16(np.arange(70 * 131).reshape(70, 131) % 65536), torch.zeros((70, 131), dtype=torch.uint8)
    pos = np.array([(0, 0, 16, 16)])
    calls = {"window_sums": lambda v, **k: CS.window_sums(v, k.pop("pos", pos), **k),
             "block_sums": lambda v, **k: CS.block_sums(v, k.pop("block", 4), **k),
             "value_histogram": lambda v, **k: CS.value_histogram(v, **k)}
    for fn, call in calls.items():
        with pytest.raises(RuntimeError, match="no CPU"):              # a good call on host tensors: there is no CPU path
            call(a16, mask=a8)
        with pytest.raises(RuntimeError, match="no CPU"):
            call(a8)
        for bad in (a16.view(torch.int16), a8.float(), a8.to(torch.int32)):
            with pytest.raises(TypeError, match=fn):
                call(bad)
            with pytest.raises(TypeError, match=fn):
                call(a16, mask=bad)
        with pytest.raises(ValueError, match="along W"):
            call(torch.zeros((131, 70), dtype=torch.uint8).t())
        with pytest.raises(ValueError, match="along W"):
            call(a8[:, ::2])
        with pytest.raises(ValueError, match=r"\(H, W\)"):
            call(a8[None])
        with pytest.raises(ValueError, match="does not match"):
            call(a16, mask=a8[:, :-1])
        with pytest.raises(ValueError, match="does not match"):
            call(a16, mask=a8[:-1])
        for kw in (dict(value_threshold=-2), dict(value_threshold=65536), dict(mask_threshold=-2), dict(mask_threshold=65536)):
            with pytest.raises(ValueError, match="threshold"):
                call(a16, mask=a8, **kw)
    for block in (0, -4, 2.5, None, True):
        with pytest.raises(ValueError, match="block"):
            CS.block_sums(a16, block)
        with pytest.raises(ValueError, match="block"):
            CS.aggregate_city(a16, block)
    for kw in (dict(bin_width=0), dict(bin_width=65536), dict(bin_width=1.5), dict(nbins=0), dict(nbins=4097), dict(nbins=-1)):
        with pytest.raises(ValueError, match="bin_width|nbins"):
            CS.value_histogram(a16, **kw)
    for bad in (np.zeros((0, 4), dtype=np.int64), [(0, 0, 16, 0)], [(120, 0, 16, 16)], [(0, 60, 16, 16)], [(-1, 0, 16, 16)], [(0, 0, 16)]):
        with pytest.raises(ValueError, match="window_sums"):           # an empty pos, and host windows outside the raster
            CS.window_sums(a16, bad)
        with pytest.raises(ValueError, match="window_sums"):
            CS.cell_heights(a16, bad, a8)
