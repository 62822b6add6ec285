#!/usr/bin/env python3
"""Generate tests/golden/g19_dataset_stats.npz by running the reference's own stats_dataset_globe functions over seeded tiles.

    python tools/make_golden_dataset_stats.py --reference <checkout of the reference>

Nothing of the reference is stored but data: the seeded tiles and labels, what its functions returned and the bytes of every file they
wrote.  stats_dataset_globe is imported behind the stub modules tools/make_golden_grid.py uses; tqdm passes its iterable through,
plt.subplots() returns a pair, cv2.imread returns the seeded label of a path, and

    gdal.Open(path, 0).GetRasterBand(b).ComputeStatistics(False)

is a FAKE: it returns tests/dataset_stats_oracle.band_row of the seeded band, i.e. this project's statement of what GDAL is understood
to return, not a result of GDAL (which is not available here).  What the fixture pins is therefore everything BEHIND the per-image
table: the reference's main_stats, main_stats_merge, main_stats_buildingheight and main_stats_buildheight_merge run as they are, in a
temporary directory, and BH_loader.hierweight over the merged histogram."""
import argparse
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402

from tests import dataset_stats_oracle as DO      # noqa: E402

REGIONS = ("china", "usa", "eu")
TILES = 4                    # per region: 12 images in all
LABELS = 3                   # label images per region
HIR = (0, 3, 12, 21, 30, 60, 90, 256)


class _Dummy(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return lambda *a, **k: None


def seeded_data():
    """{region: (s2 (TILES, 6, 8, 8) uint16, s1 (TILES, 2, 8, 8) float32, labels (LABELS, 16, 16) uint8)}"""
    rs = np.random.RandomState(19)
    out = {}
    for k, region in enumerate(REGIONS):
        s2 = (rs.randint(60, 4000, size=(TILES, 6, 8, 8)) + 500 * k).astype(np.uint16)
        s2[0, :, 0, 0], s2[1, :, -1, -1] = 0, 65535                      # both ends of the type
        s1 = (rs.rand(TILES, 2, 8, 8) * 30 - 28 + k).astype(np.float32)   # decibels
        lab = np.zeros((LABELS, 16, 16), dtype=np.uint8)                  # mostly 0, a tail up to 255
        built = rs.rand(LABELS, 16, 16) < 0.3
        lab[built] = np.minimum(255, rs.geometric(0.12, size=int(built.sum()))).astype(np.uint8)
        lab[0, 0, :8] = (1, 5, 15, 25, 40, 70, 120, 255 - k)              # every class of HIR is populated in every region
        out[region] = (s2, s1, lab)
    return out


def file_bytes(path):
    with open(path, "rb") as f:
        return np.frombuffer(f.read(), dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="directory that holds the reference's stats_dataset_globe.py")
    sys.path.insert(0, ap.parse_args().reference)
    for m in ("tifffile", "albumentations", "osgeo", "osgeo.gdal", "osgeo.ogr", "geopandas", "matplotlib", "matplotlib.pyplot", "cv2",
              "rasterio", "shapely", "shapely.geometry", "tqdm", "torchvision", "torchvision.models"):
        sys.modules[m] = _Dummy(m)
    sys.modules["osgeo"].gdal, sys.modules["osgeo"].ogr = sys.modules["osgeo.gdal"], sys.modules["osgeo.ogr"]
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    sys.modules["tqdm"].tqdm =lambda it, *a, **k: it
    sys.modules["matplotlib.pyplot"].subplots = lambda *a, **k: (_Dummy("fig"), _Dummy("ax"))
    sys.modules.setdefault("pandas", __import__("pandas"))
    import BH_loader as ref_loader
    import stats_dataset_globe as ref

    data = seeded_data()
    tmp = tempfile.mkdtemp()
    ipath, resroot = os.path.join(tmp, "data"), os.path.join(tmp, "datastats")
    os.makedirs(resroot)
    names = [f"tile_{i}.tif" for i in range(TILES)]
    lab_names = [f"bh_{i}.tif" for i in range(LABELS)]
    rasters, label_files = {}, {}
    for region, (s2, s1, lab) in data.items():
        for sub, arr in ((f"s2{region}", s2), (f"s1{region}", s1)):
            os.makedirs(os.path.join(ipath, sub))
            for i, nm in enumerate(names):
                rasters[os.path.join(ipath, sub, nm)] = arr[i]
        for i, nm in enumerate(lab_names):
            label_files[os.path.join(ipath, f"bh{region}", nm)] = lab[i]
    with open(os.path.join(ipath, "tiles.csv"), "w") as f:
        f.write("\n".join(names) + "\n")
    with open(os.path.join(ipath, "labels.csv"), "w") as f:
        f.write("\n".join(lab_names) + "\n")

    class _FakeBand:
        def __init__(self, band):
            self.band = band

        def ComputeStatistics(self, approx_ok):
            assert approx_ok is False
            row, count = DO.band_row(self.band)       # the oracle's numbers: NOT GDAL's own (see the module docstring)
            assert count == self.band.size
            return [float(v) for v in row]

    class _FakeDataset:
        def __init__(self, arr):
            self.arr = arr

        def GetRasterBand(self, b):
            return _FakeBand(self.arr[b - 1])

    ref.gdal = types.SimpleNamespace(Open=lambda path, mode=0: _FakeDataset(rasters[path]))
    ref.cv2 = types.SimpleNamespace(imread=lambda path, flag=None: label_files[path], IMREAD_UNCHANGED=-1)

    out = dict(hir=np.array(HIR, dtype=np.int64))
    for region, (s2, s1, lab) in data.items():
        out[f"s2_{region}"], out[f"s1_{region}"], out[f"labels_{region}"] = s2, s1, lab
        ref.main_stats(ipath=ipath, subdir=f"s2{region}", nband=6, resroot=resroot, imglistpath=os.path.join(ipath, "tiles.csv"))
        ref.main_stats(ipath=ipath, subdir=f"s1{region}", nband=2, resroot=resroot, imglistpath=os.path.join(ipath, "tiles.csv"))
        ref.main_stats_buildingheight(os.path.join(ipath, f"bh{region}"), resroot, f"bh_stats_{region}",
                                      filelist=os.path.join(ipath, "labels.csv"))
    ref.main_stats_merge(s1list=[f"s2{r}" for r in REGIONS], subdir="s2globe", nband=6, resroot=resroot)
    ref.main_stats_merge(s1list=[f"s1{r}" for r in REGIONS], subdir="s1globe", nband=2, resroot=resroot)
    ref.main_stats_buildheight_merge(bhlist=[f"bh_stats_{r}" for r in REGIONS], savepath=resroot, savename="bh_stats_globe")

    # what the reference's functions RETURN, per region table and for the merged one
    for sensor in ("s1", "s2"):
        tables = [np.load(os.path.join(resroot, f"{sensor}{r}.npy")) for r in REGIONS]
        for r, t in zip(REGIONS + ("globe",), tables + [np.concatenate(tables, axis=1)]):
            (mean_all, std_all), (min_all, max_all) = ref.cal_mean_std(list(t)), ref.cal_min_max(list(t), tmin=2, tmax=98)
            out[f"ret_{sensor}{r}"] = np.array([mean_all, std_all, min_all, max_all], dtype=np.float64)
        (min5, max95) = ref.cal_min_max(list(tables[0]), tmin=5, tmax=95)
        out[f"ret_{sensor}{REGIONS[0]}_p5_95"] = np.array([min5, max95], dtype=np.float64)
    merged = np.loadtxt(os.path.join(resroot, "bh_stats_globe.txt"))
    out["hierweight_globe"] = ref_loader.hierweight(merged, HIR)
    files = sorted(os.listdir(resroot))
    assert len(files) == 6 * 3 + 2 * 2 + 3 * 2 + 2, files
    for name in files:
        out["file_" + name] = file_bytes(os.path.join(resroot, name))

    # the oracle against what the reference kept of the fake's rows, bit for bit
    for region, (s2, s1, _) in data.items():
        for sensor, arr in (("s2", s2), ("s1", s1)):
            want = np.load(os.path.join(resroot, f"{sensor}{region}.npy"))
            got = DO.table(arr)[0].transpose(1, 0, 2)
            assert np.array_equal(got.view(np.int64), want.view(np.int64))
    path = os.path.join(ROOT, "tests", "golden", "g19_dataset_stats.npz")
    np.savez_compressed(path, **out)
    print(f"  pinned G19 dataset stats: {len(files)} files of the reference's main_stats / merges over {TILES * len(REGIONS)} tiles and "
          f"{LABELS * len(REGIONS)} labels; {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
