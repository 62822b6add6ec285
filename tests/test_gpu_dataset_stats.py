"""GPU: srbh_band_stats and srbh_label_hist (csrc/srbh_stats.hip) through srbh_amd.dataset_stats, every (image, band) against the exact
rational oracle tests/dataset_stats_oracle.py, and end to end into the files and constants the loaders read.

Required of every band: min, max and count exact; the mean of an integer type bit-equal to float64(integer sum) / count; the mean of
float32 within n u mean|x|; the variance std^2 within 2 [(n + 2) u var + (n u)^2 (mean^2 + var)], u = 2^-53 (corrected two-pass, Chan,
Golub & LeVeque 1983).  Errors are formed in exact rationals.  Two inputs are there for what they catch: 64 x 64 uint16 drawn from
{65534, 65535} (a one-pass float64 sum of squares misses the bound 2.6e5 times over, fp32 accumulation 1e12 times) and 64 x 64 float32
1000 + 1e-3 * rand (9e7 and 1e11)."""
import io
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from srbh_amd import dataset_stats as DS
from srbh_amd import loader_math as LM
from tests import dataset_stats_oracle as DO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1), (5, 7), (8, 8), (64, 64), (96, 80)]           # 96 x 80: more than 16 values per lane, the two-walk form
NC = [(1, 1), (3, 2), (1, 6), (3, 6), (3, 1)]
KINDS = ["u16", "i16", "f32"]
WORST = {"var": 0.0, "mean": 0.0}


def _images(kind, shape, seed):
    rs = np.random.RandomState(seed)
    if kind == "u16":
        x = rs.randint(0, 9000, size=shape).astype(np.uint16)
        x.reshape(-1)[::7] = 65535                                   # both ends of the type in every band
        x.reshape(-1)[3::11] = 0
        return x
    if kind == "i16":
        x = rs.randint(-32768, 32768, size=shape).astype(np.int16)   # both signs
        x.reshape(-1)[::13], x.reshape(-1)[5::17] = -32768, 32767
        return x
    return (rs.rand(*shape) * 40 - 32).astype(np.float32)            # "decibel" bands


def _check(images, stats, count, nodata=None, what=""):
    """every (image, band) of `images` (numpy) against the oracle; -> the worst fraction of the variance bound"""
    stats, count = stats.cpu().numpy(), count.cpu().numpy()
    n_img, n_band = images.shape[:2]
    assert stats.shape == (n_img, n_band, 4) and stats.dtype == np.float64 and count.shape == (n_img, n_band) and count.dtype == np.int64
    worst = 0.0
    for i in range(n_img):
        for b in range(n_band):
            e, got, tag = DO.band_exact(images[i, b], nodata), stats[i, b], (what, i, b)
            assert int(count[i, b]) == e["count"], tag
            if e["count"] == 0:
                assert np.isnan(got).all(), tag
                continue
            n = e["count"]
            assert got[0] == e["min"] and got[1] == e["max"], (tag, got, e["min"], e["max"])
            mean_err = abs(Fraction(float(got[2])) - e["mean"])
            if images.dtype.kind in "iu":
                s = int(DO.valid_values(images[i, b], nodata).astype(np.int64).sum())
                assert got[2] == np.float64(s) / np.float64(n), (tag, got[2])      # (|s| < 2^53: float64(s) is exact)
            else:
                mean_bound = DO.U * math.fsum(abs(float(v)) for v in DO.valid_values(images[i, b], nodata))     # n u mean|x|
                assert mean_err <= Fraction(mean_bound), (tag, float(mean_err), mean_bound)
                if mean_bound:
                    WORST["mean"] = max(WORST["mean"], float(mean_err) / mean_bound)
            var_err = abs(Fraction(float(got[3])) ** 2 - e["var"])
            bound = DO.variance_bound(n, float(e["mean"]), float(e["var"]))
            print(f"{what} image {i} band {b}: n {n} var {float(e['var']):.6g} |var err| {float(var_err):.3e} bound {bound:.3e}")
            assert got[3] >= 0.0 and var_err <= Fraction(bound), (tag, float(var_err), bound)
            if bound:
                worst = max(worst, float(var_err) / bound)
    WORST["var"] = max(WORST["var"], worst)
    return worst


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("si", range(len(SHAPES)), ids=[f"{h}x{w}" for h, w in SHAPES])
def test_band_stats_against_the_exact_oracle(kind, si):
    (h, w), (n, c) = SHAPES[si], NC[(si + KINDS.index(kind)) % len(NC)]
    x = _images(kind, (n, c, h, w), 100 + 10 * si + KINDS.index(kind))
    stats, count = DS.band_stats(torch.from_numpy(x).to(DEV))
    _check(x, stats, count, what=f"{kind} {n}x{c}x{h}x{w}")
    assert int(count.min()) == h * w


def test_every_n_and_c_at_one_shape():
    for n in (1, 3):
        for c in (1, 2, 6):
            x = _images("u16", (n, c, 8, 8), 7 * n + c)
            _check(x, *DS.band_stats(torch.from_numpy(x).to(DEV)), what=f"u16 {n}x{c}x8x8")


def test_the_two_inputs_a_one_pass_or_fp32_kernel_fails():
    rs = np.random.RandomState(3)
    top = (65534 + rs.randint(0, 2, size=(3, 2, 64, 64))).astype(np.uint16)
    near = (1000.0 + 1e-3 * rs.rand(3, 2, 64, 64)).astype(np.float32)
    for what, x in (("u16 {65534, 65535}", top), ("f32 1000 + 1e-3 rand", near)):
        frac = _check(x, *DS.band_stats(torch.from_numpy(x).to(DEV)), what=what)
        print(f"{what}: worst fraction of the variance bound {frac:.4f}")
    big = (1000.0 + 1e-3 * rs.rand(1, 1, 96, 80)).astype(np.float32)      # and through the two-walk form
    _check(big, *DS.band_stats(torch.from_numpy(big).to(DEV)), what="f32 1000 + 1e-3 rand, 96x80")


@pytest.mark.parametrize("kind,value", [("u16", 65535), ("u16", 0), ("i16", -32768), ("f32", 0.1), ("f32", -27.3125)])
def test_constant_image_has_std_exactly_zero(kind, value):
    dtype = {"u16": np.uint16, "i16": np.int16, "f32": np.float32}[kind]
    for h, w in ((64, 64), (96, 80), (5, 7)):
        x = np.full((2, 2, h, w), value, dtype=dtype)
        stats, count = DS.band_stats(torch.from_numpy(x).to(DEV))
        s = stats.cpu().numpy()
        c = np.float64(dtype(value))
        assert np.array_equal(s, np.broadcast_to(np.array([c, c, c, 0.0]), s.shape)), (kind, value, h, w, s[0, 0])
        assert int(count.min()) == h * w == int(count.max())


def test_nan_pixels_nodata_and_an_all_nodata_band():
    rs = np.random.RandomState(5)
    f = _images("f32", (3, 2, 64, 64), 50)
    f[rs.rand(*f.shape) < 0.1] = np.nan
    f[0, 1] = np.nan                                           # a band of NaNs only
    f[1, 0, 1:] = np.nan
    f[1, 0, 0, 1:] = np.nan
    f[1, 0, 0, 0] = -12.5                                      # one valid pixel
    stats, count = DS.band_stats(torch.from_numpy(f).to(DEV))
    _check(f, stats, count, what="f32 with NaN")
    assert int(count[0, 1]) == 0 and bool(stats[0, 1].isnan().all()) and int(count[1, 0]) == 1
    assert stats[1, 0].tolist() == [float(f[1, 0, 0, 0])] * 3 + [0.0]
    f[2, 1][rs.rand(64, 64) < 0.2] = -9999.0
    _check(f, *DS.band_stats(torch.from_numpy(f).to(DEV), nodata=-9999.0), nodata=-9999.0, what="f32 with NaN and nodata")
    for kind, nodata in (("u16", 0), ("u16", 65535), ("i16", -32768)):
        for h, w in ((64, 64), (96, 80), (5, 7)):
            x = _images(kind, (3, 2, h, w), 60)
            x[1, 1] = nodata                                   # all nodata
            stats, count = DS.band_stats(torch.from_numpy(x).to(DEV), nodata=nodata)
            _check(x, stats, count, nodata=nodata, what=f"{kind} {h}x{w} nodata {nodata}")
            assert int(count[1, 1]) == 0 and bool(stats[1, 1].isnan().all()) and 0 < int(count[0, 0]) < h * w
            # without the nodata value the band is a constant one
            assert DS.band_stats(torch.from_numpy(x).to(DEV))[0][1, 1].tolist() == [float(nodata)] * 3 + [0.0]
            ds = DS.DatasetStats(2)
            with pytest.raises(ValueError, match="no valid pixel"):
                ds.add(torch.from_numpy(x).to(DEV), nodata=nodata)
            assert len(ds) == 0
            ds.add(torch.from_numpy(x).to(DEV))
            assert len(ds) == 3 and ds.table().shape == (2, 3, 4)


def _same_bits(a, b):
    return all(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y)
               for x, y in zip(a, b))


@pytest.mark.parametrize("kind", KINDS)
def test_views_are_read_in_place_with_the_bits_of_the_contiguous_copy(kind):
    """a band cut (16-byte loads), a crop whose row stride is odd and whose base is unaligned (element loads), a crop with aligned rows
    (16-byte loads, a group per row segment): each against its contiguous copy, bit for bit, and against the oracle"""
    for h, w in ((64, 64), (96, 80), (8, 8)):
        full = _images(kind, (3, 8, h, w), 70)
        dev = torch.from_numpy(full).to(DEV)
        cut = dev[:, :6]
        assert not cut.is_contiguous() and cut.data_ptr() == dev.data_ptr()
        got = DS.band_stats(cut)
        _check(full[:, :6], *got, what=f"{kind} band cut {h}x{w}")
        assert _same_bits(got, DS.band_stats(torch.from_numpy(np.ascontiguousarray(full[:, :6])).to(DEV)))
        assert _same_bits(got, tuple(t[:, :6] for t in DS.band_stats(dev)))

        raster = _images(kind, (6, h + 9, w + 13), 71)            # odd row stride: w + 13
        rdev = torch.from_numpy(raster).to(DEV)
        crop, crop_np = rdev[None, :, 3:3 + h, 5:5 + w], np.ascontiguousarray(raster[None, :, 3:3 + h, 5:5 + w])
        assert crop.stride(2) % 2 == 1 and not crop.is_contiguous()
        got = DS.band_stats(crop)
        _check(crop_np, *got, what=f"{kind} crop {h}x{w}")
        assert _same_bits(got, DS.band_stats(torch.from_numpy(crop_np).to(DEV)))

        wide = _images(kind, (6, h + 8, w + 16), 72)              # rows start on 16-byte boundaries: groups are loaded whole
        wdev = torch.from_numpy(wide).to(DEV)
        crop, crop_np = wdev[None, :, 8:8 + h, 8:8 + w], np.ascontiguousarray(wide[None, :, 8:8 + h, 8:8 + w])
        assert crop.data_ptr() % 16 == 0 and not crop.is_contiguous()
        got = DS.band_stats(crop)
        _check(crop_np, *got, what=f"{kind} aligned crop {h}x{w}")
        assert _same_bits(got, DS.band_stats(torch.from_numpy(crop_np).to(DEV)))
        # and a contiguous batch whose base is not 16-byte aligned
        flat = torch.from_numpy(np.concatenate([np.zeros(1, full.dtype), full.reshape(-1)])).to(DEV)
        off = flat[1:].view(full.shape)
        assert off.data_ptr() % 16 != 0
        assert _same_bits(DS.band_stats(off), DS.band_stats(dev))


@pytest.mark.parametrize("kind", KINDS)
def test_an_images_numbers_depend_on_that_image_alone(kind):
    for h, w in ((64, 64), (96, 80), (5, 7)):
        x = _images(kind, (3, 2, h, w), 80)
        dev = torch.from_numpy(x).to(DEV)
        batch = DS.band_stats(dev)
        assert _same_bits(batch, DS.band_stats(dev))                                   # twice in a row
        for i in range(3):
            alone = DS.band_stats(torch.from_numpy(x[i:i + 1].copy()).to(DEV))
            assert _same_bits(alone, tuple(t[i:i + 1] for t in batch)), (kind, h, w, i)
        one_band = DS.band_stats(dev[:, 1:2])
        assert _same_bits(one_band, tuple(t[:, 1:2] for t in batch))


def test_image_offsets_beyond_2_to_the_31_elements():
    """the second image of each view starts 2^31 elements behind the first: offsets are 64-bit (the storage is allocated, not filled)"""
    x = _images("i16", (2, 1, 64, 64), 85)
    big = torch.empty(2 ** 31 + 4096, dtype=torch.int16, device=DEV)
    view = big.as_strided((2, 1, 64, 64), (2 ** 31, 4096, 64, 1))
    view.copy_(torch.from_numpy(x).to(DEV))
    got = DS.band_stats(view)
    _check(x, *got, what="i16 image stride 2^31")
    assert _same_bits(got, DS.band_stats(torch.from_numpy(x).to(DEV)))
    del big, view
    lab = _labels((2, 256, 256), 86)
    bigl = torch.empty(2 ** 31 + 65536, dtype=torch.uint8, device=DEV)
    lview = bigl.as_strided((2, 256, 256), (2 ** 31, 256, 1))
    lview.copy_(torch.from_numpy(lab).to(DEV))
    assert np.array_equal(DS.label_histogram(lview).cpu().numpy(), DO.label_histogram(lab))


# ---- label histogram ------------------------------------------------------------------------------------------------------------------
def _labels(shape, seed):
    rs = np.random.RandomState(seed)
    lab = np.zeros(shape, dtype=np.uint8)                       # mostly 0, a tail up to 255
    built = rs.rand(*shape) < 0.3
    lab[built] = np.minimum(255, rs.geometric(0.05, size=int(built.sum()))).astype(np.uint8)
    return lab


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("h,w", [(7, 9), (16, 16), (256, 256)])
def test_label_histogram_equals_bincount(n, h, w):
    lab = _labels((n, h, w), 90 + n)
    got = DS.label_histogram(torch.from_numpy(lab).to(DEV))
    assert got.dtype == torch.int64 and got.shape == (256,) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), DO.label_histogram(lab))
    assert np.array_equal(DS.label_histogram(torch.from_numpy(lab.reshape(n, -1)).to(DEV)).cpu().numpy(), DO.label_histogram(lab))


def test_label_histogram_hot_bins_all_values_slices_and_workspace():
    for shape in ((3, 256, 256), (3, 7, 9), (1, 300, 300)):      # 300 x 300: two workgroups per image, the second one ragged
        zero = torch.zeros(shape, dtype=torch.uint8, device=DEV)
        want = [0] * 256
        want[0] = int(np.prod(shape))
        assert DS.label_histogram(zero).tolist() == want
        assert DS.label_histogram(zero + 7).tolist() == [0] * 7 + [want[0]] + [0] * 248      # another hot bin
    every = np.arange(3 * 256 * 256, dtype=np.int64).reshape(3, 256, 256)
    every = ((every * 37 + every // 256) % 256).astype(np.uint8)                       # all 256 values, neighbours differ
    assert len(np.unique(every)) == 256
    assert np.array_equal(DS.label_histogram(torch.from_numpy(every).to(DEV)).cpu().numpy(), DO.label_histogram(every))
    runs = np.repeat(np.arange(256, dtype=np.uint8), 24)[None].repeat(2, 0)            # runs that straddle the 16-label groups
    assert np.array_equal(DS.label_histogram(torch.from_numpy(runs).to(DEV)).cpu().numpy(), DO.label_histogram(runs))
    for h, w in ((16, 16), (7, 9), (256, 256)):                                        # 7 x 9: the slice's images are not 16-byte aligned
        lab = _labels((6, h, w), 95)
        dev = torch.from_numpy(lab).to(DEV)
        for view, ref in ((dev[::2], lab[::2]), (dev[1::3], lab[1::3]), (dev[4:], lab[4:])):
            assert np.array_equal(DS.label_histogram(view).cpu().numpy(), DO.label_histogram(ref))
    lab = _labels((3, 300, 300), 96)
    dev = torch.from_numpy(lab).to(DEV)
    ws = torch.full((6 * 256,), float("nan"), dtype=torch.float32, device=DEV)         # the workspace needs no initialisation
    assert np.array_equal(DS.label_histogram(dev, workspace=ws).cpu().numpy(), DO.label_histogram(lab))
    assert not bool(ws.isnan().any())                                                  # every slot was written
    with pytest.raises(ValueError, match="workspace"):
        DS.label_histogram(dev, workspace=ws[:100])
    hs = DS.HeightStats()
    hs.add(dev).add(dev[:1])
    assert np.array_equal(hs.counts(), DO.label_histogram(lab) + DO.label_histogram(lab[:1])) and hs.counts().dtype == np.int64


# ---- closing the loop: from device tiles to the files and constants the loaders read -------------------------------------------------------
REGIONS = ("china", "usa", "eu")


@pytest.fixture(scope="module")
def g19(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g19_dataset_stats.npz")))


def test_dataset_stats_over_the_fixture_tiles_gives_the_stored_files(g19, tmp_path):
    for sensor, nband in (("s2", 6), ("s1", 2)):
        for r in REGIONS:
            tiles = g19[f"{sensor}_{r}"]
            ds = DS.DatasetStats(nband)
            ds.add(torch.from_numpy(tiles[:3]).to(DEV)).add(torch.from_numpy(tiles[3:]).to(DEV))       # two batches
            ds.save(str(tmp_path), sensor + r)
            with open(tmp_path / f"{sensor}{r}_minmax.txt", "rb") as f:
                assert f.read() == g19[f"file_{sensor}{r}_minmax.txt"].tobytes(), (sensor, r)
            want = np.load(io.BytesIO(g19[f"file_{sensor}{r}.npy"].tobytes()))
            got = np.load(tmp_path / f"{sensor}{r}.npy")
            assert np.array_equal(got[:, :, :2], want[:, :, :2]) and np.allclose(got, want, rtol=1e-13, atol=0)
            assert np.allclose(np.loadtxt(tmp_path / f"{sensor}{r}_meanstd.txt"),
                               np.loadtxt(io.BytesIO(g19[f"file_{sensor}{r}_meanstd.txt"].tobytes())), rtol=1e-12, atol=0)
        DS.main_stats_merge(s1list=[sensor + r for r in REGIONS], subdir=sensor + "globe", nband=nband, resroot=str(tmp_path))
        with open(tmp_path / f"{sensor}globe_minmax.txt", "rb") as f:
            assert f.read() == g19[f"file_{sensor}globe_minmax.txt"].tobytes(), sensor
        # the constants a loader reads back from the file normalise a batch to the same bits as the stored ones
        mine, stored = np.loadtxt(tmp_path / f"{sensor}globe_minmax.txt"), np.loadtxt(io.BytesIO(g19[f"file_{sensor}globe_minmax.txt"].tobytes()))
        raw = torch.from_numpy(g19[f"{sensor}_china"].astype(np.float32)).to(DEV)
        a, b = LM.normalize_tiles(raw, mine[0], mine[1], (0, 1)), LM.normalize_tiles(raw, stored[0], stored[1], (0, 1))
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and 0.0 < float(a.mean()) < 1.0


def test_height_stats_over_the_fixture_labels_gives_the_stored_files_and_weights(g19, tmp_path):
    regions = []
    for r in REGIONS:
        hs = DS.HeightStats().add(torch.from_numpy(g19[f"labels_{r}"]).to(DEV))
        hs.save(str(tmp_path), f"bh_stats_{r}")
        regions.append(hs)
        for ext in (".txt", ".csv"):
            with open(tmp_path / f"bh_stats_{r}{ext}", "rb") as f:
                assert f.read() == g19[f"file_bh_stats_{r}{ext}"].tobytes(), (r, ext)
    DS.main_stats_buildheight_merge(bhlist=[f"bh_stats_{r}" for r in REGIONS], savepath=str(tmp_path), savename="bh_stats_globe")
    with open(tmp_path / "bh_stats_globe.txt", "rb") as f:
        assert f.read() == g19["file_bh_stats_globe.txt"].tobytes()
    globe = DS.HeightStats()
    for r in REGIONS:
        globe.add(torch.from_numpy(g19[f"labels_{r}"]).to(DEV))
    assert np.array_equal(globe.counts().astype(np.float64), DS.HeightStats.merge(regions))
    hir = tuple(int(v) for v in g19["hir"])
    assert np.allclose(LM.hierweight(globe.counts(), hir), g19["hierweight_globe"], rtol=1e-12, atol=0)


def test_worst_fractions_of_the_bounds():
    """runs last: what the tests above measured"""
    print(f"worst fraction of the variance bound {WORST['var']:.4f}, of the float32 mean bound {WORST['mean']:.4f}")
    assert WORST["var"] <= 1.0 and WORST["mean"] <= 1.0
