#!/usr/bin/env python3
"""Generate tests/golden/g20_city_grid.npz by running the reference's own Fishgridnew_bound, Fishgrid_stats, compare_twotiff_valid,
compare_twotiff_valid_iou and generateindex over two seeded in-memory rasters.

    python tools/make_golden_city_grid.py --reference <checkout of the reference>

Nothing of the reference is stored but data: the two seeded rasters, the windows its functions produced and the fields they wrote.
generate_WSF_mask_Globeheight_grid, demo_preprocess_height_v2 and BH_loader are imported behind stub modules, and the OGR / GDAL /
geopandas objects they touch are FAKES of this tool: a layer is a list of features with a dict of fields, a geometry is the list of
points the reference adds (GetEnvelope / .bounds are their min and max), GetRasterBand(1).ReadAsArray(xoff, yoff, xcount, ycount) is a
slice of the seeded array, gdal.Warp(..., outputBounds=...) returns the SAME window of the second raster (both rasters lie on one grid;
nothing is warped or resampled), the coordinate transformation is the identity, GeoDataFrame.from_file is a pandas DataFrame of the
layer, and get_tif_meta is patched.  What the fixture pins is therefore the reference's arithmetic and ordering BEHIND those objects --
the four steps of the layout, the int() / round() pixel arithmetic, the uint8 cast before the comparison, the sums, the flags, the rows
it skips -- not GDAL's rasterisation, warping or reprojection, which are not available here.

The geotransform is (500000, 10, 0, 4200000, 0, -10): every corner coordinate is a small multiple of 10 added to an integer, exact in
float64, so Fishgrid_stats' int() truncation and generateindex's round() agree (the tool asserts it)."""
import argparse
import os
import sys
import types

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402

from tests import city_grid_oracle as CO      # noqa: E402

GEOTRANS = (500000.0, 10.0, 0.0, 4200000.0, 0.0, -10.0)
W, H, WINDOW, OFFSET = 131, 70, 16, 14
COND_STATS = (0, 20, 256)
COND_CMP = (0, 40, 256, 0.3)
LAYOUTS = ((200, 150, 64, 56), (65, 64, 64, 56))
# further layouts that are compared with the oracle but not stored
CHECKED = ((176, 120, 64, 56), (120, 176, 64, 56), (176, 176, 64, 56), (64, 64, 64, 56), (300, 257, 64, 48), (4000, 3000, 64, 56))


class _Dummy(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return lambda *a, **k: None


def seeded_rasters():
    """two uint8 footprint rasters (H, W) of 0 / 255: blobs, a second raster that partly disagrees, the top-left cell empty in both, a
    block of cells identical in both, and single specks that stay below the isv threshold of 20 pixels"""
    rs = np.random.RandomState(20)
    a = np.zeros((H, W), dtype=np.uint8)
    for _ in range(14):                                              # blobs: rectangles with ragged edges
        x, y, w, h = rs.randint(20, W - 12), rs.randint(0, H - 10), rs.randint(4, 22), rs.randint(4, 16)
        a[y:y + h, x:x + w] = 255
    a[rs.rand(H, W) < 0.04] = 0
    b = a.copy()
    b[:, 60:] = np.roll(a[:, 60:], 3, axis=1)                        # the right part disagrees by a shift ...
    b[40:, 60:100] = 0                                               # ... and a block is missing altogether
    b[rs.rand(H, W) < 0.01] = 255
    a[:16, :16] = 0                                                  # cell (0, 0): empty in both
    b[:16, :16] = 0
    a[20:34, 0:14] = 0                                               # specks only: below the threshold
    a[22, 3] = a[30, 9] = a[25, 12] = 255
    b[20:34, 0:14] = a[20:34, 0:14]
    a[42:56, 28:42] = 255                                            # a block of cells identical in both
    a[45:50, 30:36] = 0
    b[42:56, 28:42] = a[42:56, 28:42]
    return a, b


# ---- fakes of the OGR / GDAL / geopandas objects the reference touches (see the module docstring) ----------------------------------------
class _Geom:
    def __init__(self, kind=None):
        self.pts, self.sub = [], []

    def AddPoint(self, x, y):
        self.pts.append((x, y))

    def CloseRings(self):
        pass

    def AddGeometry(self, ring):
        self.sub.append(ring)

    def Transform(self, ct):
        pass

    @property
    def bounds(self):
        p = [q for r in self.sub for q in r.pts]
        xs, ys = [x for x, _ in p], [y for _, y in p]
        return min(xs), min(ys), max(xs), max(ys)

    def GetEnvelope(self):
        minx, miny, maxx, maxy = self.bounds
        return minx, maxx, miny, maxy


class _Feature:
    def __init__(self, defn):
        self.defn, self.geom, self.fields = defn, None, {}

    def SetGeometry(self, g):
        self.geom = g

    def GetGeometryRef(self):
        return self.geom

    def SetField2(self, name, value):
        assert name in self.defn.names, name
        self.fields[name] = value

    def GetFieldAsInteger(self, index):
        return int(self.fields.get(self.defn.names[index], 0))


class _Defn:
    def __init__(self):
        self.names = []

    def GetFieldIndex(self, name):
        return self.names.index(name) if name in self.names else -1


class _Layer:
    def __init__(self):
        self.defn, self.features = _Defn(), []

    def GetLayerDefn(self):
        return self.defn

    def CreateFeature(self, f):
        self.features.append(f)

    def CreateField(self, fd):
        self.defn.names.append(fd)

    def SetFeature(self, f):
        assert f in self.features

    def GetSpatialRef(self):
        return None

    def __iter__(self):
        return iter(list(self.features))


class _Raster:
    def __init__(self, arr):
        self.arr = arr

    def GetRasterBand(self, b):
        assert b == 1
        return self

    def ReadAsArray(self, xoff=0, yoff=0, xcount=None, ycount=None):
        if xcount is None:
            return self.arr.copy()
        assert 0 <= xoff and 0 <= yoff and xoff + xcount <= self.arr.shape[1] and yoff + ycount <= self.arr.shape[0]
        return self.arr[yoff:yoff + ycount, xoff:xoff + xcount].copy()

    def GetGeoTransform(self):
        return GEOTRANS

    def GetProjectionRef(self):
        return "wkt"


def install_fakes(mods, layers, rasters):
    """point the ogr / gdal / osr names of the reference modules `mods` at the fakes; `layers` {path: _Layer}, `rasters` {path: array}"""
    class _DS:
        def __init__(self, path):
            self.path = path

        def CreateLayer(self, name, *a, **k):
            layers[name] = _Layer()
            return layers[name]

        def GetLayer(self):
            return layers[self.path]

    class _Driver:
        def CreateDataSource(self, path):
            return _DS(path)

        def Open(self, path, mode=0):
            return _DS(path)

    def warp(dst, src, format=None, outputBounds=None, xRes=None, yRes=None, dstSRS=None):
        minx, miny, maxx, maxy = outputBounds                       # the same window of the second raster: nothing is resampled
        x0, y0 = (minx - GEOTRANS[0]) / GEOTRANS[1], (GEOTRANS[3] - maxy) / -GEOTRANS[5]
        x1, y1 = (maxx - GEOTRANS[0]) / GEOTRANS[1], (GEOTRANS[3] - miny) / -GEOTRANS[5]
        assert all(float(v).is_integer() for v in (x0, y0, x1, y1))
        return _Raster(rasters[src][int(y0):int(y1), int(x0):int(x1)])

    ogr = types.SimpleNamespace(GetDriverByName=lambda name: _Driver(), Geometry=_Geom, Feature=_Feature, FieldDefn=lambda name, t: name,
                                wkbLinearRing=1, wkbPolygon=2, OFTInteger64=12, OFTReal=2)
    gdal = types.SimpleNamespace(Open=lambda path, mode=0: _Raster(rasters[path]), Warp=warp)
    osr = types.SimpleNamespace(SpatialReference=lambda wkt=None: None, CoordinateTransformation=lambda a, b: None)
    for m in mods:
        m.ogr, m.gdal, m.osr = ogr, gdal, osr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="directory that holds the reference's generate_WSF_mask_Globeheight_grid.py")
    sys.path.insert(0, ap.parse_args().reference)
    for m in ("cv2", "osgeo", "osgeo.gdal", "osgeo.ogr", "osgeo.osr", "osgeo.gdalconst", "xpinyin", "rasterio", "mask_revised", "geopandas",
              "tqdm", "shapely", "shapely.geometry", "matplotlib", "matplotlib.pyplot", "fiona", "tifffile", "albumentations",
              "torchvision", "torchvision.models"):
        sys.modules[m] = _Dummy(m)
    for a in ("gdal", "ogr", "osr", "gdalconst"):
        setattr(sys.modules["osgeo"], a, sys.modules["osgeo." + a])
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    import pandas as pd
    import BH_loader as ref_loader
    import demo_preprocess_height_v2 as ref_pre
    import generate_WSF_mask_Globeheight_grid as ref_grid

    a, b = seeded_rasters()
    layers, rasters = {}, {"/x/city_wsf.tif": a, "/x/city_ref.vrt": b}
    install_fakes((ref_grid, ref_pre), layers, rasters)
    ref_loader.gpd = types.SimpleNamespace(GeoDataFrame=types.SimpleNamespace(from_file=lambda shp: pd.DataFrame(
        [dict(geometry=f.geom, **f.fields) for f in layers[shp].features])))

    def fishnet(width, height, window, offset):
        """the reference's Fishgridnew_bound -> (its fresh layer, the windows generateindex reads from it)"""
        ref_grid.get_tif_meta = lambda path: (width, height, GEOTRANS, "wkt")
        ref_grid.Fishgridnew_bound("/x/city_s2.tif", window_size=window, offset=offset)
        shp = "/x/city_s2_grid.shp"
        pos = np.array(ref_loader.generateindex(shp, GEOTRANS), dtype=np.int64).reshape(-1, 4)
        for f, row in zip(layers[shp].features, pos.tolist()):       # Fishgrid_stats' int() against generateindex's round()
            minx, maxx, miny, maxy = f.geom.GetEnvelope()
            assert (int((minx - GEOTRANS[0]) / 10.0), int((GEOTRANS[3] - maxy) / 10.0), int((maxx - minx) / 10.0),
                    int((maxy - miny) / 10.0)) == tuple(row)
        assert np.array_equal(pos, CO.fishgrid_windows(width, height, window, offset)), (width, height, window, offset)
        return shp, pos

    out = dict(geotransform=np.array(GEOTRANS), mask=a, other=b, grid=np.array([W, H, WINDOW, OFFSET], dtype=np.int64),
               cond_stats=np.array(COND_STATS, dtype=np.int64), cond_compare=np.array(COND_CMP, dtype=np.float64))
    for lay in LAYOUTS + CHECKED:
        _, pos = fishnet(*lay)
        if lay in LAYOUTS:
            out["pos_%dx%d_%d_%d" % lay] = pos

    # Fishgrid_stats and generateindex with and without validname
    shp, pos = fishnet(W, H, WINDOW, OFFSET)
    ref_pre.Fishgrid_stats("/x/city_wsf.tif", shp, fieldname=("sum", "count", "isv"), condition=COND_STATS)
    feats = layers[shp].features
    out["pos"] = pos
    for k in ("sum", "count", "isv"):
        out[k] = np.array([f.fields[k] for f in feats], dtype=np.int64)
    out["index_all"] = np.array(ref_loader.generateindex(shp, GEOTRANS), dtype=np.int64).reshape(-1, 4)
    out["index_isv"] = np.array(ref_loader.generateindex(shp, GEOTRANS, validname="isv"), dtype=np.int64).reshape(-1, 4)
    want = CO.fishgrid_stats(a, pos, COND_STATS)
    assert all(np.array_equal(out[k], want[k]) for k in want)
    assert 0 < out["isv"].sum() < len(pos) and (out["sum"] == 0).any() and ((out["sum"] > 0) & (out["sum"] < COND_STATS[1])).any()

    # the two compare functions: over the isv of Fishgrid_stats, and over a layer whose every cell is valid (condition (0, 0, 256)) so
    # that the rows the first run skips -- the cell that is empty in both rasters among them -- are computed too
    ints = ("vrt_sum", "vrt_count", "absdiff", "isv2", "isv3", "isv4")
    for metric, fn in (("absdiff", ref_pre.compare_twotiff_valid), ("iou", ref_pre.compare_twotiff_valid_iou)):
        for tag, cond in (("", COND_STATS), ("_all", (0, 0, 256))):
            shp, pos = fishnet(W, H, WINDOW, OFFSET)
            ref_pre.Fishgrid_stats("/x/city_wsf.tif", shp, fieldname=("sum", "count", "isv"), condition=cond)
            feats = layers[shp].features
            isv = np.array([f.fields["isv"] for f in feats], dtype=np.int64)
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                       # (0 / 0.0 of calculate_iou)
                fn("/x/city_wsf.tif", "/x/city_ref.vrt", shp, condition=COND_CMP)
            key = f"{metric}{tag}_"
            done = np.array(["vrt_sum" in f.fields for f in feats])
            assert np.array_equal(done, isv != 0)
            out[key + "set"] = done                                   # False: the reference left the row's fields unset
            for k in ints:
                out[key + k] = np.array([int(f.fields.get(k, 0)) for f in feats], dtype=np.int64)
            if metric == "iou":
                out[key + "diou"] = np.array([float(f.fields.get("diou", np.nan)) for f in feats], dtype=np.float64)
            want = CO.compare_cells(a, b, pos, isv, COND_CMP, metric)
            for k in ints:
                assert np.array_equal(out[key + k], want[k]), (key, k)
            if metric == "iou":
                assert np.array_equal(out[key + "diou"].view(np.int64), want["diou"].view(np.int64)), key
    d = out["iou_all_diou"]
    assert np.isnan(d).any() and (d == 0).any() and ((d > 0) & (d < 1)).any() and out["iou_isv4"].any() and not out["iou_isv4"].all()

    path = os.path.join(ROOT, "tests", "golden", "g20_city_grid.npz")
    np.savez_compressed(path, **out)
    print(f"  pinned G20 city grid: oracle == reference Fishgridnew_bound / Fishgrid_stats / compare_twotiff_valid(_iou) / generateindex "
          f"({len(pos)} cells of {WINDOW} / {OFFSET} over {W} x {H}, {int(out['isv'].sum())} valid; {len(LAYOUTS + CHECKED)} further "
          f"layouts); {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
