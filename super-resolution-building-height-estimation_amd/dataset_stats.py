"""Dataset statistics on the device: the three small text files every loader starts from (reference stats_dataset_globe.py).

``<s1dir>_minmax.txt`` / ``<s2dir>_minmax.txt`` feed ``normalize_tiles``, ``train_batch``, ``GridTiles`` and ``predict_city`` (reference
BH_loader.py:301-304); the 256-bin floor histogram ``bh_stats_<city>.txt`` feeds ``hierweight`` / ``LabelPrep`` (BH_loader.py:30-61).
The reference makes them on the host, one GeoTIFF at a time: GDAL ``ComputeStatistics`` per tile and band, ``np.unique`` per label
image.  Here the per-image pass is two libsrbh kernels over tensors that are already on the device (csrc/srbh_stats.hip):

* ``band_stats``       per image and band ``(min, max, mean, std)`` and the valid-pixel count, float64, bit-reproducible;
* ``label_histogram``  the exact 256-bin histogram of uint8 labels.

Everything behind the per-image table -- ``cal_mean_std``, ``cal_min_max`` (``np.percentile``'s interpolation is part of the contract),
the region merges and the files -- is the reference's arithmetic in numpy on the host, under the reference's names: given the same table,
the text files are byte-identical.  ``DatasetStats`` and ``HeightStats`` tie the two halves together.

``band_stats`` is this project's own statement of what GDAL's ``ComputeStatistics(False)`` is understood to return (an exact scan; NaN and
nodata pixels excluded; population std).  GDAL is not available where the project is built and tested; no GDAL result has been compared.
GPU only; reading GeoTIFFs, the plots of the reference and ``floor2height`` are out of scope."""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib

__all__ = ["band_stats", "label_histogram", "cal_mean_std", "cal_min_max", "DatasetStats", "HeightStats", "main_stats_merge",
           "main_stats_buildheight_merge"]

_TYPE_CODES = {torch.float32: 0, torch.uint16: 1, torch.int16: 2}       # include/srbh.h SRBH_GRID_F32 / _U16 / _I16
NBINS = 256


def _need_device(*tensors):
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError("srbh dataset statistics run on the GPU only (no CPU fallback)")


# ---- the two kernels ------------------------------------------------------------------------------------------------------------------
def band_stats(images, nodata=None):
    """images: (N, C, H, W) device tensor of float32, uint16 or int16, read in place through its strides (a batch, a band cut
    ``x[:, :6]`` and a crop ``raster[None, :, y0:y1, x0:x1]`` are not copied; only a column stride other than 1 is).
    -> ``(stats (N, C, 4) float64 {min, max, mean, std}, count (N, C) int64)`` on the device; no host synchronisation.
    Pixels that are NaN or equal to ``nodata`` do not count; a band without a valid pixel has count 0 and four NaNs."""
    if not isinstance(images, torch.Tensor) or images.dim() != 4:
        raise ValueError(f"band_stats: images must be an (N, C, H, W) tensor (got {getattr(images, 'shape', type(images))})")
    if images.dtype not in _TYPE_CODES:
        raise ValueError(f"band_stats: images must be float32, uint16 or int16 (got {images.dtype})")
    if min(images.shape) < 1:
        raise ValueError(f"band_stats: every dimension must be at least 1 (got {tuple(images.shape)})")
    nd = None
    if nodata is not None:
        try:
            nd = float(nodata)
        except (TypeError, ValueError):
            raise ValueError(f"band_stats: nodata must be a number or None (got {nodata!r})") from None
        if math.isnan(nd):
            raise ValueError("band_stats: nodata must not be NaN (NaN pixels are excluded anyway)")
    _need_device(images)
    x = images.detach()
    if x.shape[3] > 1 and x.stride(3) != 1:
        x = x.contiguous()
    n, c, h, w = x.shape
    stats = torch.empty((n, c, 4), dtype=torch.float64, device=x.device)
    count = torch.empty((n, c), dtype=torch.int64, device=x.device)
    strides = (C.c_long * 3)(*x.stride()[:3])
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().srbh_band_stats(x.data_ptr(), _TYPE_CODES[x.dtype], strides, n, c, h, w,
                                              None if nd is None else C.byref(C.c_double(nd)), stats.data_ptr(), count.data_ptr(),
                                              _lib.stream_ptr()), "srbh_band_stats")
    return stats, count


def _label_hist_into(labels, hist, ws=None):
    """the kernel call of label_histogram: `labels` (N, HW) uint8 with unit pixel stride, `hist` (256,) int64, `ws` uint8 workspace or None"""
    n, hw = labels.shape
    L = _lib.lib()
    need = L.srbh_label_hist_ws_bytes(n, hw)
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=labels.device)
    elif ws.numel() * ws.element_size() < need:
        raise ValueError(f"label_histogram: workspace of {ws.numel() * ws.element_size()} bytes, {need} needed")
    with torch.cuda.device(labels.device):
        _lib.check(L.srbh_label_hist(labels.data_ptr(), labels.stride(0), n, hw, hist.data_ptr(), ws.data_ptr(), _lib.stream_ptr()),
                   "srbh_label_hist")
    return hist


def label_histogram(labels, workspace=None):
    """labels: (N, ...) uint8 device tensor, one label image per leading index (a batch slice is read in place; an image that is not
    contiguous in itself is copied) -> (256,) int64 counts on the device, exact; no host synchronisation.  ``workspace``: optional
    device buffer of at least srbh_label_hist_ws_bytes bytes to reuse between calls (its content does not matter)."""
    if not isinstance(labels, torch.Tensor) or labels.dim() < 2:
        raise ValueError(f"label_histogram: labels must be an (N, ...) tensor (got {getattr(labels, 'shape', type(labels))})")
    if labels.dtype != torch.uint8:
        raise ValueError(f"label_histogram: labels must be uint8 (got {labels.dtype})")
    if min(labels.shape) < 1:
        raise ValueError(f"label_histogram: every dimension must be at least 1 (got {tuple(labels.shape)})")
    _need_device(labels)
    x = labels.detach()
    if not x[0].is_contiguous():
        x = x.contiguous()
    x = x.as_strided((x.shape[0], x[0].numel()), (x.stride(0), 1))
    return _label_hist_into(x, torch.empty(NBINS, dtype=torch.int64, device=x.device), workspace)


# ---- the reference's host arithmetic over the per-image tables (stats_dataset_globe.py:24-59) ---------------------------------------------
def cal_mean_std(stats_s1):
    """stats_s1: per band an (images, 4) float64 table {min, max, mean, std} -> (mean_all, std_all), lists of one float per band: the
    mean of the image means and sqrt(mean(std^2 + mean^2) - mean_all^2) (stats_dataset_globe.py:24-42, its expressions in its order)."""
    mean_all, std_all = [], []
    for table in stats_s1:
        imean, istd = table[:, 2], table[:, 3]
        second = (istd * istd + imean * imean).mean()
        m = imean.mean()
        mean_all.append(m)
        std_all.append(math.sqrt(second - m * m))
    return mean_all, std_all


def cal_min_max(stats_s1, tmin=2, tmax=98):
    """-> (min_all, max_all): per band np.percentile(image minima, tmin) and np.percentile(image maxima, tmax), the reference's 2 % linear
    stretch (stats_dataset_globe.py:45-59); np.percentile's default linear interpolation is part of the contract."""
    min_all, max_all = [], []
    for table in stats_s1:
        min_all.append(np.percentile(table[:, 0], tmin))
        max_all.append(np.percentile(table[:, 1], tmax))
    return min_all, max_all


def _save_summary(stats_s1, resroot, subdir):
    """<subdir>_meanstd.txt and <subdir>_minmax.txt as main_stats / main_stats_merge write them (stats_dataset_globe.py:94-101, :123-130)"""
    mean_all, std_all = cal_mean_std(stats_s1)
    min_all, max_all = cal_min_max(stats_s1, tmin=2, tmax=98)
    np.savetxt(os.path.join(resroot, subdir + "_meanstd.txt"), np.array([mean_all, std_all]))
    np.savetxt(os.path.join(resroot, subdir + "_minmax.txt"), np.array([min_all, max_all]))
    return (mean_all, std_all), (min_all, max_all)


class DatasetStats:
    """The per-image table of one image directory, filled a batch at a time from the device, and the files main_stats writes from it."""

    def __init__(self, nband):
        nband = int(nband)
        if nband < 1:
            raise ValueError(f"DatasetStats: nband must be at least 1 (got {nband})")
        self.nband = nband
        self._parts = []          # (n, nband, 4) float64 host arrays

    def add(self, images, nodata=None):
        """append the rows of a batch (N, nband, H, W).  Raises ValueError if a band of an image has no valid pixel (its row would be
        four NaNs) -- the ONE check of this module that needs the kernel's result on the host; the copy of the table that follows needs
        it anyway."""
        if isinstance(images, torch.Tensor) and images.dim() == 4 and images.shape[1] != self.nband:
            raise ValueError(f"DatasetStats.add: {self.nband} bands expected (got {tuple(images.shape)})")
        stats, count = band_stats(images, nodata)
        empty = (count == 0).nonzero().cpu()
        if len(empty):
            i, b = (int(v) for v in empty[0])
            raise ValueError(f"DatasetStats.add: band {b} of image {i} of this batch has no valid pixel ({len(empty)} such bands); nothing added")
        self._parts.append(stats.cpu().numpy())
        return self

    def __len__(self):
        return sum(len(p) for p in self._parts)

    def table(self):
        """(nband, num, 4) float64: the array of main_stats' .npy (band, image, {min, max, mean, std})"""
        if not self._parts:
            return np.zeros((self.nband, 0, 4))
        return np.ascontiguousarray(np.concatenate(self._parts, axis=0).transpose(1, 0, 2))

    def save(self, resroot, subdir):
        """write <subdir>.npy, <subdir>_meanstd.txt and <subdir>_minmax.txt into resroot, with main_stats' np.save / np.savetxt calls
        (stats_dataset_globe.py:91-101).  -> ((mean_all, std_all), (min_all, max_all))"""
        if not len(self):
            raise ValueError("DatasetStats.save: no image has been added")
        stats_s1 = list(self.table())
        np.save(os.path.join(resroot, subdir + ".npy"), stats_s1)
        return _save_summary(stats_s1, resroot, subdir)

    @classmethod
    def merge(cls, tables):
        """the region merge of main_stats_merge (stats_dataset_globe.py:108-119): (nband, num_i, 4) tables (arrays or DatasetStats)
        concatenated along the image axis, in the order given -> a DatasetStats holding all rows"""
        tables = [t.table() if isinstance(t, DatasetStats) else np.asarray(t, dtype=np.float64) for t in tables]
        if not tables or any(t.ndim != 3 or t.shape[2] != 4 or t.shape[0] != tables[0].shape[0] for t in tables):
            raise ValueError("DatasetStats.merge: tables must be (nband, num, 4) arrays with one band count")
        out = cls(tables[0].shape[0])
        out._parts = [np.ascontiguousarray(t.transpose(1, 0, 2)) for t in tables]
        return out


def main_stats_merge(s1list=("s1china_check", "s1usa_check", "s1eu_check"), subdir="s1_vvvhratio", nband=2, resroot="datastatsglobe"):
    """merge the <name>.npy tables of several regions in resroot and write <subdir>_meanstd.txt / <subdir>_minmax.txt
    (stats_dataset_globe.py:105-130, same signature)"""
    merged = DatasetStats.merge([np.load(os.path.join(resroot, name + ".npy")) for name in s1list])
    if merged.nband != nband:
        raise ValueError(f"main_stats_merge: the tables hold {merged.nband} bands, nband = {nband}")
    return _save_summary(list(merged.table()), resroot, subdir)


# ---- building-height histogram ----------------------------------------------------------------------------------------------------------
def _write_height_files(counts, savepath, savename):
    """<savename>.txt (np.savetxt of the float64 counts) and <savename>.csv with the columns ,height,number,rate that the reference writes
    through pandas (stats_dataset_globe.py:156-159): floats in their shortest round-trip form, one row per floor"""
    stats = np.asarray(counts, dtype=np.float64)
    base = os.path.join(savepath, savename)
    np.savetxt(base + ".txt", stats)
    with np.errstate(invalid="ignore"):
        rate = stats / stats.sum()
    with open(base + ".csv", "w", newline="") as f:
        f.write(",height,number,rate\n")
        for i in range(NBINS):
            r = "" if math.isnan(rate[i]) else repr(float(rate[i]))      # (an empty field is how a NaN is written and read back)
            f.write(f"{i},{i},{float(stats[i])!r},{r}\n")


def _read_height_csv(path):
    """the 'number' column of a <savename>.csv"""
    with open(path) as f:
        head = f.readline().rstrip("\n").split(",")
        col = head.index("number")
        return np.array([float(line.split(",")[col]) for line in f if line.strip()], dtype=np.float64)


class HeightStats:
    """The floor histogram of a region's height labels, accumulated in int64 on the device (main_stats_buildingheight,
    stats_dataset_globe.py:148-159, without its plot)."""

    def __init__(self, device="cuda"):
        self.device = device
        self._counts = None

    def add(self, labels):
        """add a batch of uint8 label images (N, ...); no host synchronisation"""
        h = label_histogram(labels)
        self._counts = h if self._counts is None else self._counts + h.to(self._counts.device)
        return self

    def counts(self):
        """(256,) int64 numpy array: pixels per floor value (what hierweight takes as `stats`)"""
        if self._counts is None:
            return np.zeros(NBINS, dtype=np.int64)
        return self._counts.cpu().numpy()

    def save(self, savepath, savename):
        """write <savename>.txt -- byte-identical to the reference's np.savetxt of its float64 counts -- and <savename>.csv (columns
        height, number, rate; read back by pd.read_csv(path, header=0, index_col=0) with equal values)"""
        _write_height_files(self.counts(), savepath, savename)

    @staticmethod
    def merge(counts):
        """the sum of several regions' histograms, float64 as main_stats_buildheight_merge forms it (stats_dataset_globe.py:182-187)"""
        stats = np.zeros((NBINS,))
        for c in counts:
            c = c.counts() if isinstance(c, HeightStats) else np.asarray(c)
            if c.shape != (NBINS,):
                raise ValueError(f"HeightStats.merge: histograms must have {NBINS} bins (got {c.shape})")
            stats = stats + np.array(c, dtype=np.float64)
        return stats


def main_stats_buildheight_merge(bhlist=("bh_stats_china", "bh_stats_bhusa", "bh_stats_bheu"), savepath="datastatsglobe",
                                 savename="bh_stats_globe"):
    """sum the 'number' columns of <name>.csv for every name of bhlist and write <savename>.txt / .csv into savepath
    (stats_dataset_globe.py:179-193, same signature; the plot is left out)"""
    stats = HeightStats.merge([_read_height_csv(os.path.join(savepath, name + ".csv")) for name in bhlist])
    _write_height_files(stats, savepath, savename)
    return stats
