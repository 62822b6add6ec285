"""Polygon zones over a city's predicted rasters: the reference's "mean and std of building height in each urban center".

The reference publishes that table (datasetglobe/urbanarea_meanstd.xls, README "Testing on 301 urban centers"); an urban centre is a
polygon (``urban_centers.shp``), and its ``zonal_stats`` (demo_preprocess_height_v2.py:450-570) does one ``gdal.RasterizeLayer`` into a
scratch raster, one window read and one ``numpy.ma`` sum per feature.  Here, over ``harness.predict_city``'s ``(height, class)``:

* ``zone_edges``         polygons (rings of float64 vertices, in pixels or through a GDAL geotransform) -> the int32 fixed-point edge table;
* ``zone_items``         the work list: each zone's bounding box cut into bands of about ``item_pixels`` pixels (host, numpy);
* ``zone_sums``          per zone ``[count, n, sum, sumsq, max]``, every zone in ONE libsrbh call (csrc/srbh_zones.hip), exact integers;
* ``zone_histogram``     per zone the selected pixels counted by ``min(v // bin_width, nbins - 1)``;
* ``zone_heights`` / ``zonal_fields`` / ``urban_centre_table``  the reference's numbers from those integers.

THE RULE (this project's own; include/srbh.h states it in full).  Coordinates are raster pixels -- the raster spans [0, W] x [0, H] and
pixel (x, y) has its centre at (x + 1/2, y + 1/2) -- quantised to int32 fixed point with 8 fractional bits: ``X = rint(256 * p)`` in
float64 (256 * p is exact, rint rounds half to even), and this quantisation is part of the definition.  |X|, |Y| <= 2^29.  A pixel is in
a zone iff the number of the zone's edges that cross its row (``min(Y0, Y1) <= 256 y + 128 < max(Y0, Y1)``) strictly right of its centre
is odd: even-odd over all rings of all parts, so holes and multipolygons need no flag, and where two parts overlap the overlap is
outside.  A centre on a left or top boundary is in, on a right or bottom boundary out.  It is modelled on ``RasterizeLayer`` without
ALL_TOUCHED on the value raster's own grid; no result of GDAL is compared, and the sub-pixel shift of the reference's per-feature scratch
grid (anchored at the polygon's own xmin, ymax) is not reproduced.

A pixel is SELECTED as in city_summary -- inside the raster, ``value > value_threshold`` and (no mask or ``mask > mask_threshold``) --
and in the zone.  Raster units throughout.  GPU only.  Reading shapefiles, reprojection, GeoTIFFs and the .xls are out of scope; a
burned label raster is ``city_burn``'s."""
import numpy as np
import torch

from . import _lib
from .city_grid import _on_device, _workspace
from .city_summary import _NAMES, _abi, _bins, _rasters, heights_from_sums

__all__ = ["Zones", "zone_edges", "zone_items", "zone_sums", "zone_histogram", "zone_heights", "zonal_fields", "urban_centre_table"]

FRACTION_BITS = 8
COORD_MAX = 2 ** 29
ITEM_PIXELS = 65536


class Zones:
    """the host tables of Z zones: ``edges`` (E, 4) int32 (X0, Y0, X1, Y1) without horizontal edges, ``edge_off`` (Z + 1,) int32 and
    ``bbox`` (Z, 4) int64 (Xmin, Ymin, Xmax, Ymax) of each zone's edges in fixed point (all zero for a zone without edges)"""

    def __init__(self, edges, edge_off, bbox):
        self.edges, self.edge_off, self.bbox = edges, edge_off, bbox
        self._device_tables = {}                                         # (zone_sums' uploaded tables; the arrays above are not to be changed)

    def __len__(self):
        return len(self.edge_off) - 1


def _quantise(ring, geotransform, where):
    ring = np.asarray(ring, dtype=np.float64)
    if ring.ndim != 2 or ring.shape[1] != 2:
        raise ValueError(f"zone_edges: {where} must be an (n, 2) array of vertices (got {ring.shape})")
    if geotransform is not None:
        x0, dx, _, y0, _, dy = geotransform
        ring = (ring - (x0, y0)) / (dx, dy)
    if not np.isfinite(ring).all():
        raise ValueError(f"zone_edges: {where} holds a vertex that is not finite")
    q = np.rint(ring * float(1 << FRACTION_BITS))                        # (exact product; rint rounds half to even)
    if q.size and np.abs(q).max() > COORD_MAX:
        raise ValueError(f"zone_edges: {where} holds a vertex beyond +-2^{29 - FRACTION_BITS} pixels (the fixed-point limit 2^29)")
    return q.astype(np.int64)


def zone_edges(polygons, geotransform=None):
    """-> ``Zones``.  ``polygons``: a list of zones; a zone is a list of rings; a ring is an (n, 2) float64 array of (x, y) vertices -- a
    multipolygon is simply all its rings, exterior or hole.  Without ``geotransform`` the vertices are raster pixels; with a GDAL
    geotransform ``(x0, dx, 0, y0, 0, dy)`` map coordinates become pixels by ``(X - x0) / dx``, ``(Y - y0) / dy`` (a rotated transform is
    refused).  Rings are closed if they are not; a ring with fewer than 3 distinct vertices contributes nothing; horizontal edges are
    dropped.  Coordinates are quantised to ``rint(256 p)``; one beyond +-2^29 raises."""
    if geotransform is not None:
        geotransform = tuple(float(g) for g in geotransform)
        if len(geotransform) != 6 or geotransform[2] != 0 or geotransform[4] != 0:
            raise ValueError(f"zone_edges: a rotated or malformed geotransform {geotransform} (terms 2 and 4 must be 0)")
        if geotransform[1] == 0 or geotransform[5] == 0 or not np.isfinite(geotransform).all():
            raise ValueError(f"zone_edges: geotransform {geotransform} has no pixel size")
    edges, off, bbox = [], [0], []
    for zi, zone in enumerate(polygons):
        mine = []
        for ri, ring in enumerate(zone):
            q = _quantise(ring, geotransform, f"ring {ri} of zone {zi}")
            if len(np.unique(q, axis=0)) < 3:
                continue
            nxt = np.roll(q, -1, axis=0)                                 # (the closing segment; of a closed ring it is a point)
            e = np.concatenate([q, nxt], axis=1)
            mine.append(e[e[:, 1] != e[:, 3]])
        mine = np.concatenate(mine) if mine else np.zeros((0, 4), dtype=np.int64)
        edges.append(mine)
        off.append(off[-1] + len(mine))
        bbox.append((mine[:, [0, 2]].min(), mine[:, [1, 3]].min(), mine[:, [0, 2]].max(), mine[:, [1, 3]].max()) if len(mine) else (0, 0, 0, 0))
    if off[-1] >= 2 ** 31:
        raise ValueError("zone_edges: more than 2^31 - 1 edges")
    edges = np.concatenate(edges) if edges else np.zeros((0, 4), dtype=np.int64)
    return Zones(edges.astype(np.int32).reshape(-1, 4), np.array(off, dtype=np.int32), np.array(bbox, dtype=np.int64).reshape(-1, 4))


def zone_items(zones, H, W, item_pixels=ITEM_PIXELS):
    """-> (items (NI, 5) int32 rows (zone, xoff, yoff, xcount, ycount), item_off (Z + 1,) int32): per zone the rows y with ``Ymin <= 256 y
    + 128 < Ymax`` and the columns ``floor(Xmin / 256) .. ceil(Xmax / 256)``, both clipped to the H x W raster, cut into bands of whole
    rows that hold about ``item_pixels`` pixels each (at least one row).  A zone with nothing inside the raster has no item.  Host only."""
    if not isinstance(zones, Zones):
        raise TypeError("zone_items: zones must come from zone_edges")
    H, W, item_pixels = int(H), int(W), int(item_pixels)
    if H < 1 or W < 1 or item_pixels < 1:
        raise ValueError(f"zone_items: H={H}, W={W}, item_pixels={item_pixels} must be positive")
    items, off = [], [0]
    for z, (xmin, ymin, xmax, ymax) in enumerate(zones.bbox.tolist()):
        y0, y1 = max((ymin + 127) >> 8, 0), min((ymax + 127) >> 8, H)
        x0, x1 = max(xmin >> 8, 0), min(-((-xmax) >> 8), W)
        if y1 > y0 and x1 > x0:
            rows, width = y1 - y0, x1 - x0
            bands = -(-rows // max(1, item_pixels // width))
            cuts = [y0 + (rows * b) // bands for b in range(bands + 1)]
            items += [(z, x0, cuts[b], width, cuts[b + 1] - cuts[b]) for b in range(bands)]
        off.append(len(items))
    if len(items) >= 2 ** 31:
        raise ValueError(f"zone_items: {len(items)} items; raise item_pixels")
    return np.array(items, dtype=np.int32).reshape(-1, 5), np.array(off, dtype=np.int32)


# ---- the kernels ----------------------------------------------------------------------------------------------------------------------------
def _tables(zones, H, W, item_pixels, device):
    """-> (device pointers of edges, edge_off, items, item_off; Z, E, NI).  The four tables go into one pinned host buffer (edges first:
    16-byte aligned) and are uploaded by ONE non-blocking copy; the device buffer is kept on ``zones`` per raster size, band size, device
    and stream, so that the next call (urban_centre_table makes three) builds and uploads nothing."""
    key = (H, W, item_pixels, device.index, _lib.stream_ptr().value)
    hit = zones._device_tables.get(key)
    if hit is None:
        items, item_off = zone_items(zones, H, W, item_pixels)
        parts = [zones.edges.reshape(-1), zones.edge_off, items.reshape(-1), item_off]
        host = torch.empty(sum(p.size for p in parts) + 4, dtype=torch.int32).pin_memory()
        at, offs = 0, []
        for p in parts:
            host[at:at + p.size] = torch.from_numpy(np.ascontiguousarray(p, dtype=np.int32))
            offs.append(at)
            at += p.size
        dev = host.to(device, non_blocking=True)
        if len(zones._device_tables) >= 8:                              # (a few raster sizes at most; never an unbounded store)
            zones._device_tables.clear()
        hit = zones._device_tables[key] = (dev, [dev.data_ptr() + 4 * o for o in offs], len(zones), len(zones.edges), len(items))
    return hit[1:]


def _check_zones(fn, zones, item_pixels):
    """the zone arguments of an entry (here and in city_zone_compare), judged without a device -> item_pixels as int"""
    if isinstance(item_pixels, bool) or not isinstance(item_pixels, (int, np.integer)) or item_pixels < 1:
        raise ValueError(f"{fn}: item_pixels={item_pixels!r} must be an integer >= 1")
    if not isinstance(zones, Zones):
        raise TypeError(f"{fn}: zones must come from zone_edges")
    if len(zones) < 1:
        raise ValueError(f"{fn}: no zones")
    return int(item_pixels)


def _prepare(fn, value, zones, mask, value_threshold, mask_threshold, item_pixels):
    """the argument path of both entries: everything that needs no device first -> (the eight leading ABI arguments, the table
    arguments, vthr, mthr, the device)"""
    H, W, vthr, mthr = _rasters(fn, value, mask, value_threshold, mask_threshold)
    item_pixels = _check_zones(fn, zones, item_pixels)
    value, rs_v, mask, rs_m = _on_device(fn, _NAMES, value, mask)
    with torch.cuda.device(value.device):
        ptrs, Z, E, NI = _tables(zones, H, W, item_pixels, value.device)
    return _abi(value, rs_v, mask, rs_m, H, W), (ptrs[0], ptrs[1], Z, E, ptrs[2], ptrs[3], NI), vthr, mthr, value.device


def zone_sums(value, zones, mask=None, value_threshold=0, mask_threshold=0, item_pixels=ITEM_PIXELS, workspace=None):
    """-> device (Z, 5) int64 ``[count, n, sum, sumsq, max]`` per zone, one srbh_zone_sums call on the current stream, no synchronisation.
    ``count`` = the zone's pixels inside the raster, the others over its selected pixels (0 when n == 0): window_sums' row, and
    ``heights_from_sums`` applies unchanged.  A zone without edges or wholly outside the raster gives zeros.  ``workspace``: optional
    device buffer to reuse between calls (srbh_zone_sums_ws_bytes(number of items) bytes; its content does not matter)."""
    fn = "zone_sums"
    abi, tab, vthr, mthr, device = _prepare(fn, value, zones, mask, value_threshold, mask_threshold, item_pixels)
    Z, E, NI = tab[2], tab[3], tab[6]
    out = torch.empty((Z, 5), dtype=torch.int64, device=device)
    if E == 0 or NI == 0:                                                 # nothing of any zone lies inside the raster
        return out.zero_()
    ws = _workspace(fn, workspace, _lib.lib().srbh_zone_sums_ws_bytes(NI), device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().srbh_zone_sums(*abi, *tab, vthr, mthr, out.data_ptr(), ws.data_ptr(), _lib.stream_ptr()), "srbh_zone_sums")
    return out


def zone_histogram(value, zones, bin_width=1, nbins=256, mask=None, value_threshold=0, mask_threshold=0, item_pixels=ITEM_PIXELS,
                   workspace=None):
    """-> device (Z, nbins) int64: per zone its selected pixels counted by ``min(value // bin_width, nbins - 1)``, exact.
    ``zone_histogram(height, zones, 10, 256, build)`` is each urban centre's height histogram in the 256-bin layout of bh_stats_*.txt,
    ``zone_histogram(build, zones, 1, 7, value_threshold=-1)`` its class counts."""
    fn = "zone_histogram"
    bin_width, nbins = _bins(fn, bin_width, nbins)
    abi, tab, vthr, mthr, device = _prepare(fn, value, zones, mask, value_threshold, mask_threshold, item_pixels)
    Z, E, NI = tab[2], tab[3], tab[6]
    hist = torch.empty((Z, nbins), dtype=torch.int64, device=device)
    if E == 0 or NI == 0:
        return hist.zero_()
    ws = _workspace(fn, workspace, _lib.lib().srbh_zone_hist_ws_bytes(NI, nbins), device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().srbh_zone_hist(*abi, *tab, vthr, mthr, bin_width, nbins, hist.data_ptr(), ws.data_ptr(), _lib.stream_ptr()),
                   "srbh_zone_hist")
    return hist


# ---- the reference's numbers ------------------------------------------------------------------------------------------------------------------
def zone_heights(height, zones, build=None):
    """The per-zone table over a predicted city: ``heights_from_sums`` of ``zone_sums(height, zones, build)`` -- n, count, fraction, mean,
    std (population), max over the zone's pixels with height > 0 and, with ``build``, class > 0.  One call and one device-to-host copy of
    Z x 5 int64.  Raster units (predict_city's height is round(10 h))."""
    return heights_from_sums(zone_sums(height, zones, build).cpu().numpy())


def zonal_fields(value, zones):
    """The two fields the reference's zonal_stats writes per feature: ``sum`` = the zone's pixels with value > 0, ``count`` = the zone's
    pixels inside the raster.  numpy int64."""
    s = zone_sums(value, zones).cpu().numpy()
    return {"sum": s[:, 1].copy(), "count": s[:, 0].copy()}


def _centre_table(height, build, zones, bin_width, nbins, num_class, more=None):
    """urban_centre_table's calls, then ``more()``'s device (Z, k) table where one is asked for; ONE torch.cat and ONE device-to-host
    copy for everything -> (urban_centre_table's dict, the k columns of ``more`` as a numpy array)"""
    parts = [zone_sums(height, zones, build), zone_histogram(height, zones, bin_width, nbins, build)]
    if build is not None:
        parts.append(zone_histogram(build, zones, 1, num_class, value_threshold=-1))
    if more is not None:
        parts.append(more())
    flat = torch.cat(parts, dim=1).cpu().numpy()
    end = flat.shape[1] - (0 if more is None else parts[-1].shape[1])
    out = heights_from_sums(flat[:, :5])
    out["hist"] = flat[:, 5:5 + nbins].copy()
    out["class_counts"] = None if build is None else flat[:, 5 + nbins:end].copy()
    return out, flat[:, end:]


def urban_centre_table(height, build, zones, bin_width=10, nbins=256, num_class=7):
    """The urbanarea_meanstd row of each zone: dict of numpy arrays with one entry per zone -- ``mean``, ``std``, ``max``, ``n``,
    ``count``, ``fraction`` as zone_heights gives them, ``hist`` (Z, nbins) int64 (the zone's height histogram,
    zone_histogram(height, zones, bin_width, nbins, build)) and ``class_counts`` (Z, num_class) int64 (every pixel of the zone by class,
    the last class open; None without ``build``).  Three calls, one read-back."""
    return _centre_table(height, build, zones, bin_width, nbins, num_class)[0]
