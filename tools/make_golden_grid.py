#!/usr/bin/env python3
"""Generate tests/golden/g18_grid_tiles.npz by running the reference's own gridimgLoader.__getitem__ (BH_loader.py:933-993).

    python tools/make_golden_grid.py --reference <checkout of the reference>

Nothing of the reference is stored but data: the seeded rasters, the stats, the windows and what __getitem__ returned for each of
them.  BH_loader is imported with the stub modules
tools/make_golden.py uses for g9 / g13; gdal.Open(...).ReadAsArray(xoff, yoff, xcount, ycount) is a fake over the seeded arrays,
get_tif_meta and generateindex are patched, and the two *_minmax.txt files are written into a temporary directory and read back by the
reference's own np.loadtxt.  tests/grid_oracle.py is pinned against every returned image bit for bit before the file is written."""
import argparse
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402

from tests import grid_oracle as GO      # noqa: E402

NCHANS, TILE = 6, 8
H, W = 20, 27
# full, clipped at the right edge, at the bottom edge, at the corner, odd offsets, one 1 x 1, a narrow and a flat one
WINDOWS = [(0, 0, 8, 8), (8, 0, 8, 8), (16, 8, 8, 8), (24, 0, 3, 8), (24, 8, 3, 8), (0, 16, 8, 4), (8, 16, 8, 4), (24, 16, 3, 4),
           (5, 3, 8, 8), (13, 11, 7, 5), (26, 19, 1, 1), (1, 1, 1, 8), (3, 7, 8, 1)]


class _Dummy(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return lambda *a, **k: None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="directory that holds the reference's BH_loader.py")
    sys.path.insert(0, ap.parse_args().reference)
    for m in ("tifffile", "albumentations", "osgeo", "osgeo.gdal", "geopandas", "matplotlib", "matplotlib.pyplot", "cv2", "rasterio",
              "torchvision", "torchvision.models"):
        sys.modules[m] = _Dummy(m)
    sys.modules["osgeo"].gdal = sys.modules["osgeo.gdal"]
    sys.modules.setdefault("pandas", __import__("pandas"))
    import BH_loader as ref_loader

    rs = np.random.RandomState(18)
    s2 = rs.randint(0, 9000, size=(8, H, W)).astype(np.uint16)
    s2[:, 0, 0], s2[:, -1, -1] = 0, 65535                                    # both ends of the type
    s1 = (rs.rand(2, H, W) * 40 - 32).astype(np.float32)
    # float32-representable stats: the bound of the GPU test counts the kernel's two roundings, not a rounding of its constants
    s2_stats = np.stack([np.array([100.0, 120.5, 90.25, 0.0, 310.0, 77.0, 5.0, 9.0]),
                         np.array([3100.0, 4020.5, 5090.75, 6000.0, 7310.0, 8077.0, 9005.0, 9009.0])])
    s1_stats = np.stack([np.array([-25.0, -28.5]), np.array([5.0, 2.25])])
    for a in (s2_stats, s1_stats, s2_stats[1] - s2_stats[0], s1_stats[1] - s1_stats[0]):
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a)

    tmp = tempfile.mkdtemp()
    np.savetxt(os.path.join(tmp, "s2_minmax.txt"), s2_stats, fmt="%.10f")
    np.savetxt(os.path.join(tmp, "s1_minmax.txt"), s1_stats, fmt="%.10f")
    rasters = {os.path.join(tmp, "city_s2.tif"): s2, os.path.join(tmp, "city_s1.tif"): s1}

    class _FakeDataset:
        def __init__(self, arr):
            self.arr = arr

        def ReadAsArray(self, xoff, yoff, xcount, ycount):
            return np.array(GO.read_window(self.arr, xoff, yoff, xcount, ycount))

    ref_loader.gdal = types.SimpleNamespace(Open=lambda path, mode=0: _FakeDataset(rasters[path]))
    ref_loader.get_tif_meta = lambda path: (W, H, (0.0, 1.0, 0.0, 0.0, 0.0, -1.0), "")
    ref_loader.generateindex = lambda shp, transform, validname=None: list(WINDOWS)
    ds = ref_loader.gridimgLoader(rootname=tmp, cityname="city", datastats=tmp, normmethod="minmax", s1dir="s1", s2dir="s2",
                                  nchans=NCHANS)
    assert len(ds) == len(WINDOWS)
    out = dict(s2=s2, s1=s1, s2_stats=s2_stats, s1_stats=s1_stats, nchans=np.int64(NCHANS), tile=np.int64(TILE),
               windows=np.array(WINDOWS, dtype=np.int64))
    for i in range(len(ds)):
        img, pos = ds[i]
        img = np.asarray(img)
        assert img.dtype == np.float32 and img.shape == (NCHANS + 2, WINDOWS[i][3], WINDOWS[i][2]), (img.dtype, img.shape)
        want = GO.cell(s2, s1, WINDOWS[i], s2_stats, s1_stats, NCHANS)
        assert np.array_equal(img.view(np.int32), want.view(np.int32)), f"window {i}: oracle != reference"
        out[f"img_{i}"], out[f"pos_{i}"] = img, np.asarray(pos)
    path = os.path.join(ROOT, "tests", "golden", "g18_grid_tiles.npz")
    np.savez_compressed(path, **out)
    print(f"  pinned G18 grid tiles: oracle == reference gridimgLoader.__getitem__ bit for bit ({len(ds)} windows); "
          f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
