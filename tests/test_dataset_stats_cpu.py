"""CPU: the host half of srbh_amd.dataset_stats against what the reference's own stats_dataset_globe functions returned and wrote
(tests/golden/g19_dataset_stats.npz, tools/make_golden_dataset_stats.py), the exact oracle, the C ABI's declarations and refusals, and
every argument check.  No kernel is launched here (the kernels: tests/test_gpu_dataset_stats.py)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from srbh_amd import dataset_stats as DS
from tests import dataset_stats_oracle as DO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "super-resolution-building-height-estimation_amd")
REGIONS = ("china", "usa", "eu")
SENSORS = {"s1": 2, "s2": 6}


@pytest.fixture(scope="module")
def g19(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g19_dataset_stats.npz")))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _stored_table(g19, name):
    """the (nband, num, 4) array of a stored <name>.npy"""
    import io
    return np.load(io.BytesIO(g19[f"file_{name}.npy"].tobytes()))


def _same_file(path, g19, name):
    with open(path, "rb") as f:
        assert f.read() == g19["file_" + name].tobytes(), name


def test_fixture_is_small_and_holds_what_the_issue_lists(g19, golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "g19_dataset_stats.npz")) < 64 * 1024
    for r in REGIONS:
        assert g19[f"s2_{r}"].shape == (4, 6, 8, 8) and g19[f"s2_{r}"].dtype == np.uint16
        assert g19[f"s1_{r}"].shape == (4, 2, 8, 8) and g19[f"s1_{r}"].dtype == np.float32
        lab = g19[f"labels_{r}"]
        assert lab.shape == (3, 16, 16) and lab.dtype == np.uint8 and (lab == 0).mean() > 0.6 and lab.max() >= 253
    assert g19["s2_china"].min() == 0 and g19["s2_china"].max() == 65535
    assert len([k for k in g19 if k.startswith("file_")]) == 30


def test_oracle_reproduces_the_stored_per_image_tables_bit_for_bit(g19):
    for sensor, nband in SENSORS.items():
        for r in REGIONS:
            want = _stored_table(g19, sensor + r)
            stats, count = DO.table(g19[f"{sensor}_{r}"])
            assert want.shape == (nband, 4, 4) and np.array_equal(_bits(stats.transpose(1, 0, 2)), _bits(want))
            assert np.array_equal(count, np.full((4, nband), 64))


def test_cal_functions_reproduce_every_stored_return_value(g19):
    for sensor in SENSORS:
        tables = [_stored_table(g19, sensor + r) for r in REGIONS]
        for r, t in zip(REGIONS + ("globe",), tables + [DS.DatasetStats.merge(tables).table()]):
            mean_all, std_all = DS.cal_mean_std(list(t))
            min_all, max_all = DS.cal_min_max(list(t))
            assert np.array_equal(_bits(np.array([mean_all, std_all, min_all, max_all])), _bits(g19[f"ret_{sensor}{r}"])), (sensor, r)
        got = DS.cal_min_max(list(tables[0]), tmin=5, tmax=95)
        assert np.array_equal(_bits(np.array(got)), _bits(g19[f"ret_{sensor}china_p5_95"]))


def test_dataset_stats_files_are_byte_identical(g19, tmp_path):
    """DatasetStats given the stored table writes the reference's three files; the region merge writes its two"""
    for sensor, nband in SENSORS.items():
        for r in REGIONS:
            ds = DS.DatasetStats.merge([_stored_table(g19, sensor + r)])
            assert ds.nband == nband and len(ds) == 4 and np.array_equal(_bits(ds.table()), _bits(_stored_table(g19, sensor + r)))
            (mean_all, _), (_, max_all) = ds.save(str(tmp_path), sensor + r)
            assert len(mean_all) == nband and len(max_all) == nband
            for suffix in (".npy", "_meanstd.txt", "_minmax.txt"):
                _same_file(tmp_path / (sensor + r + suffix), g19, sensor + r + suffix)
        DS.main_stats_merge(s1list=[sensor + r for r in REGIONS], subdir=sensor + "globe", nband=nband, resroot=str(tmp_path))
        for suffix in ("_meanstd.txt", "_minmax.txt"):
            _same_file(tmp_path / (sensor + "globe" + suffix), g19, sensor + "globe" + suffix)
    with pytest.raises(ValueError, match="nband"):
        DS.main_stats_merge(s1list=["s1china"], subdir="x", nband=3, resroot=str(tmp_path))


def test_height_files_are_byte_identical_and_the_csv_round_trips(g19, tmp_path):
    import io

    import pandas as pd
    regions = []
    for r in REGIONS:
        counts = DO.label_histogram(g19[f"labels_{r}"])
        regions.append(counts)
        DS._write_height_files(counts, str(tmp_path), f"bh_stats_{r}")
        _same_file(tmp_path / f"bh_stats_{r}.txt", g19, f"bh_stats_{r}.txt")
        got = pd.read_csv(tmp_path / f"bh_stats_{r}.csv", header=0, index_col=0)
        want = pd.read_csv(io.BytesIO(g19[f"file_bh_stats_{r}.csv"].tobytes()), header=0, index_col=0)
        assert list(got.columns) == ["height", "number", "rate"] and got.shape == (256, 3)
        for col in got.columns:
            assert got[col].dtype == want[col].dtype and np.array_equal(got[col].values, want[col].values), (r, col)
        assert np.array_equal(got["number"].values, counts.astype(np.float64)) and np.array_equal(got.index.values, np.arange(256))
        _same_file(tmp_path / f"bh_stats_{r}.csv", g19, f"bh_stats_{r}.csv")
    stats = DS.main_stats_buildheight_merge(bhlist=[f"bh_stats_{r}" for r in REGIONS], savepath=str(tmp_path), savename="bh_stats_globe")
    assert stats.dtype == np.float64 and np.array_equal(stats, np.sum(regions, axis=0)) and np.array_equal(stats, DS.HeightStats.merge(regions))
    for suffix in (".txt", ".csv"):
        _same_file(tmp_path / ("bh_stats_globe" + suffix), g19, "bh_stats_globe" + suffix)
    # an empty histogram: the rate column is 0 / 0 -- written as empty fields, read back as NaN, as pandas does
    DS.HeightStats().save(str(tmp_path), "empty")
    back = pd.read_csv(tmp_path / "empty.csv", header=0, index_col=0)
    assert not back["number"].values.any() and np.isnan(back["rate"].values).all()


def test_hierweight_of_the_merged_histogram_is_the_reference_value(g19):
    from srbh_amd import loader_math as LM
    merged = DS.HeightStats.merge([DO.label_histogram(g19[f"labels_{r}"]) for r in REGIONS])
    assert np.allclose(LM.hierweight(merged, tuple(g19["hir"])), g19["hierweight_globe"], rtol=1e-12, atol=0)


def test_oracle_known_answers():
    row, n = DO.band_row(np.array([[1, 2], [3, 4]], dtype=np.uint16))
    assert n == 4 and row.tolist() == [1.0, 4.0, 2.5, 1.25 ** 0.5]
    row, n = DO.band_row(np.array([np.nan, -3.0, 7.0, 7.0], dtype=np.float32), nodata=7.0)
    assert n == 1 and row.tolist() == [-3.0, -3.0, -3.0, 0.0]
    row, n = DO.band_row(np.full((3, 3), 9, dtype=np.int16), nodata=9)
    assert n == 0 and np.isnan(row).all()
    x = np.array([65534, 65535] * 8, dtype=np.uint16)           # the variance a one-pass sum of squares cannot see
    e = DO.band_exact(x)
    assert e["mean"] == 65534.5 and e["var"] == 0.25
    assert DO.label_histogram(np.array([[0, 0, 255], [3, 0, 3]])).tolist() == [3, 0, 0, 2] + [0] * 251 + [1]


def test_entry_points_are_declared_exported_and_refuse_bad_arguments():
    from srbh_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "srbh.h")).read()
    names = ("srbh_band_stats", "srbh_label_hist", "srbh_label_hist_ws_bytes")
    protos = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, protos), f"{name} is not declared in srbh.h"
        assert name in _lib.SIGNATURES
    assert "ComputeStatistics" in hdr and "project's own" in hdr
    assert "srbh_stats.hip" in _lib.SOURCES
    _lib.build()
    L = _lib.lib()
    for name in names:
        assert hasattr(L, name)
    # nothing reaches a device: every call returns SRBH_ERR_ARG first
    p = C.c_void_p(4096)       # never dereferenced
    ok, neg = (C.c_long * 3)(6 * 64, 64, 8), (C.c_long * 3)(6 * 64, 64, -8)
    nd = C.byref(C.c_double(0.0))
    assert L.srbh_band_stats(None, 0, ok, 1, 6, 8, 8, None, p, p, None) == -1
    assert L.srbh_band_stats(p, 0, None, 1, 6, 8, 8, None, p, p, None) == -1
    assert L.srbh_band_stats(p, 0, ok, 1, 6, 8, 8, nd, None, p, None) == -1
    assert L.srbh_band_stats(p, 0, ok, 1, 6, 8, 8, nd, p, None, None) == -1
    assert L.srbh_band_stats(p, 3, ok, 1, 6, 8, 8, None, p, p, None) == -1              # unknown type code
    assert L.srbh_band_stats(p, -1, ok, 1, 6, 8, 8, None, p, p, None) == -1
    for bad in ((0, 6, 8, 8), (1, 0, 8, 8), (1, 6, 0, 8), (1, 6, 8, -1)):
        assert L.srbh_band_stats(p, 1, ok, *bad, None, p, p, None) == -1
    assert L.srbh_band_stats(p, 2, neg, 1, 6, 8, 8, None, p, p, None) == -1             # negative stride
    assert L.srbh_band_stats(p, 2, ok, 1 << 20, 1 << 12, 8, 8, None, p, p, None) == -1  # 2^32 workgroups
    assert b"srbh_band_stats" in L.srbh_last_error()
    assert L.srbh_label_hist(None, 256, 1, 256, p, p, None) == -1
    assert L.srbh_label_hist(p, 256, 1, 256, None, p, None) == -1
    assert L.srbh_label_hist(p, 256, 1, 256, p, None, None) == -1
    assert L.srbh_label_hist(p, 256, 0, 256, p, p, None) == -1
    assert L.srbh_label_hist(p, 256, 1, 0, p, p, None) == -1
    assert L.srbh_label_hist(p, -256, 1, 256, p, p, None) == -1
    assert b"srbh_label_hist" in L.srbh_last_error()
    # one slot of 256 32-bit counters per 65536 labels of an image
    assert L.srbh_label_hist_ws_bytes(1, 1) == 1024 and L.srbh_label_hist_ws_bytes(3, 65536) == 3 * 1024
    assert L.srbh_label_hist_ws_bytes(3, 65537) == 6 * 1024 and L.srbh_label_hist_ws_bytes(1024, 256 * 256) == 1024 * 1024
    assert L.srbh_label_hist_ws_bytes(0, 256) == 0 and L.srbh_label_hist_ws_bytes(1, 0) == 0


def test_reference_names_are_exported_and_the_dropin_path_resolves(tmp_path):
    import srbh_amd
    for name in ("cal_mean_std", "cal_min_max", "main_stats_merge", "main_stats_buildheight_merge"):
        assert getattr(srbh_amd, name) is getattr(DS, name)
    with pytest.raises(AttributeError):
        srbh_amd.no_such_name
    code = ("import sys; sys.path.insert(0, %r);"
            "from stats_dataset_globe import cal_mean_std, cal_min_max, main_stats_merge, main_stats_buildheight_merge;"
            "import srbh_amd.dataset_stats as m;"
            "assert cal_mean_std is m.cal_mean_std and cal_min_max is m.cal_min_max and main_stats_merge is m.main_stats_merge;"
            "assert main_stats_buildheight_merge is m.main_stats_buildheight_merge;"
            "assert not ({'cv2', 'osgeo', 'pandas', 'matplotlib', 'rasterio'} & set(sys.modules)); print('ok')") % os.path.join(PKG, "dropin")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(tmp_path))
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr


def test_cpu_tensors_raise_and_bad_arguments_raise_value_error():
    x = torch.zeros(2, 6, 8, 8, dtype=torch.uint16)
    for fn, arg in ((DS.band_stats, x), (DS.label_histogram, torch.zeros(2, 8, 8, dtype=torch.uint8)),
                    (DS.DatasetStats(6).add, x), (DS.HeightStats().add, torch.zeros(2, 64, dtype=torch.uint8))):
        with pytest.raises(RuntimeError, match="GPU only"):
            fn(arg)
    for bad in (x[0], x.to(torch.float64), x.to(torch.uint8), torch.zeros(2, 0, 8, 8), torch.zeros(0, 2, 8, 8), np.zeros((1, 1, 2, 2), np.float32)):
        with pytest.raises(ValueError, match="band_stats"):
            DS.band_stats(bad)
    for bad in ("zero", float("nan"), [1, 2]):
        with pytest.raises(ValueError, match="nodata"):
            DS.band_stats(x, nodata=bad)
    with pytest.raises(RuntimeError, match="GPU only"):
        DS.band_stats(x, nodata=0)                     # a good nodata: only the device is missing
    lab = torch.zeros(2, 8, 8, dtype=torch.uint8)
    for bad in (lab[0, 0], lab.to(torch.int64), lab.float(), torch.zeros(2, 0, dtype=torch.uint8), [[0, 1]]):
        with pytest.raises(ValueError, match="label_histogram"):
            DS.label_histogram(bad)
    with pytest.raises(ValueError, match="nband"):
        DS.DatasetStats(0)
    ds = DS.DatasetStats(2)
    with pytest.raises(ValueError, match="2 bands"):
        ds.add(x)                                      # 6 bands into a 2-band table
    assert len(ds) == 0 and ds.table().shape == (2, 0, 4)
    with pytest.raises(ValueError, match="no image"):
        ds.save(".", "never_written")
    with pytest.raises(ValueError, match="merge"):
        DS.DatasetStats.merge([np.zeros((2, 3, 4)), np.zeros((3, 3, 4))])
    with pytest.raises(ValueError, match="merge"):
        DS.DatasetStats.merge([])
    with pytest.raises(ValueError, match="256 bins"):
        DS.HeightStats.merge([np.zeros(255)])
    assert DS.HeightStats().counts().tolist() == [0] * 256
