"""Building footprints burned into a raster on the device: the label raster the validation entries consume.

The reference makes its reference height rasters and its training labels with ``shp_to_tiff`` / ``shp2tif``
(demo_preprocess_height_v2.py:27-119, ``main_shp2tif``): one ``gdal.RasterizeLayer(..., options=["ATTRIBUTE=<field>"])`` that paints
every building footprint, in feature order, with its attribute value.  Here:

* ``feature_edges``  millions of small rings as ONE vertex array and two offset arrays -> ``city_zones.Zones`` (equal to ``zone_edges``
  of the same polygons, without a Python loop per feature);
* ``burn_tiles``     the work list: per 64 x 64 tile of the raster the features whose pixel box meets it, ascending (host, numpy);
* ``burn``           features + one value each -> a uint16 / uint8 device raster, ONE libsrbh call (csrc/srbh_burn.hip), exact;
* ``label_raster``   heights in metres -> the ``ref_u16`` of ``city_validation`` / ``cell_errors`` / ``urban_centre_validation``, in
  ``predict_city``'s units (``round_half_even(10 h)``);
* ``zone_raster``    ``index + 1`` burned over a background of 0: the zone-id raster.

THE RULE (this project's own, like city_zones'; include/srbh.h states it in full).  Feature ``f`` is a zone in city_zones' sense: all
edges of all its rings, int32 fixed point with 8 fractional bits, even-odd over its own edges, the pixel centre decides, a centre on a
left or top boundary is in, on a right or bottom boundary out.  ``merge="last"`` (GDAL's replace): a pixel takes the value of the LARGEST
``f`` whose zone holds it -- a value of 0 burns like any other; ``merge="max"``: the largest value among the containing features.  A
pixel in no feature gets ``init``, or, with ``keep``, is not written.  Overlap of two parts of ONE feature is outside.  Integers only:
bit-equal between runs.  No result of GDAL is compared.

GPU only.  Reading shapefiles, reprojection, GeoTIFFs, ALL_TOUCHED, GDAL's additive merge and float or int16 rasters are out of scope."""
import numpy as np
import torch

from . import _lib
from .city_grid import _on_device
from .city_zones import COORD_MAX, FRACTION_BITS, Zones

__all__ = ["feature_edges", "burn_tiles", "burn", "label_raster", "zone_raster", "MERGES", "TILE"]

MERGES = {"last": 0, "max": 1}                                           # include/srbh.h SRBH_BURN_*
TILE = 64                                                                # srbh_burn_tile()
_TYPES = {torch.uint16: 1, torch.uint8: 3}                               # include/srbh.h SRBH_GRID_*
_TOP = {torch.uint16: 65535, torch.uint8: 255}


# ---- the edge table, flat -----------------------------------------------------------------------------------------------------------------
def _offsets(fn, name, off, end):
    off = np.asarray(off)
    if off.ndim != 1 or len(off) < 1 or off.dtype.kind not in "iu":
        raise ValueError(f"{fn}: {name} must be a 1-d integer array of at least one offset")
    off = off.astype(np.int64)
    if off[0] != 0 or off[-1] != end or (np.diff(off) < 0).any():
        raise ValueError(f"{fn}: {name} must ascend from 0 to {end}")
    return off


def feature_edges(vertices, ring_off, feature_off, geotransform=None):
    """-> ``Zones``, with arrays EQUAL to ``zone_edges`` of the same polygons.  ``vertices``: (n, 2) float64 (x, y) of every ring, one
    after the other; ``ring_off`` (R + 1,): ring r is ``vertices[ring_off[r]:ring_off[r + 1]]``; ``feature_off`` (F + 1,): feature f owns
    the rings ``feature_off[f] .. feature_off[f + 1]`` (exteriors, holes and parts alike).  ``geotransform`` as in ``zone_edges``.  Rings
    are closed if they are not; a ring with fewer than 3 distinct quantised vertices contributes nothing; horizontal edges are dropped.
    numpy throughout: no Python loop per feature."""
    fn = "feature_edges"
    v = np.asarray(vertices, dtype=np.float64)
    if v.ndim != 2 or v.shape[1] != 2:
        raise ValueError(f"{fn}: vertices must be an (n, 2) array (got {v.shape})")
    ring_off = _offsets(fn, "ring_off", ring_off, len(v))
    feature_off = _offsets(fn, "feature_off", feature_off, len(ring_off) - 1)
    if geotransform is not None:
        geotransform = tuple(float(g) for g in geotransform)
        if len(geotransform) != 6 or geotransform[2] != 0 or geotransform[4] != 0:
            raise ValueError(f"{fn}: a rotated or malformed geotransform {geotransform} (terms 2 and 4 must be 0)")
        if geotransform[1] == 0 or geotransform[5] == 0 or not np.isfinite(geotransform).all():
            raise ValueError(f"{fn}: geotransform {geotransform} has no pixel size")
        x0, dx, _, y0, _, dy = geotransform
        v = (v - (x0, y0)) / (dx, dy)
    if not np.isfinite(v).all():
        raise ValueError(f"{fn}: a vertex is not finite")
    q = np.rint(v * float(1 << FRACTION_BITS))                           # (exact product; rint rounds half to even)
    if q.size and np.abs(q).max() > COORD_MAX:
        raise ValueError(f"{fn}: a vertex beyond +-2^{29 - FRACTION_BITS} pixels (the fixed-point limit 2^29)")
    q = q.astype(np.int64)
    n, R, F = len(q), len(ring_off) - 1, len(feature_off) - 1
    counts = np.diff(ring_off)
    ring_of = np.repeat(np.arange(R), counts)                            # the ring of each vertex
    # the distinct vertices of each ring: sort by (ring, x, y) and count the changes
    order = np.lexsort((q[:, 1], q[:, 0], ring_of))
    s, sr = q[order], ring_of[order]
    new = np.ones(n, dtype=bool)
    new[1:] = (sr[1:] != sr[:-1]) | (s[1:] != s[:-1]).any(axis=1)
    live = np.bincount(sr[new], minlength=R) >= 3                        # per ring
    # vertex i -> the next vertex of its ring (the last one closes the ring; of a closed ring that segment is a point)
    nxt = np.arange(1, n + 1)
    last = ring_off[1:][counts > 0] - 1
    nxt[last] = ring_off[:-1][counts > 0]
    e = np.concatenate([q, q[nxt]], axis=1) if n else np.zeros((0, 4), dtype=np.int64)
    use = live[ring_of] & (e[:, 1] != e[:, 3])
    e = e[use]
    feat_of_ring = np.repeat(np.arange(F), np.diff(feature_off))
    per = np.bincount(feat_of_ring[ring_of[use]], minlength=F)           # edges per feature
    if per.sum() >= 2 ** 31:
        raise ValueError(f"{fn}: more than 2^31 - 1 edges")
    off = np.zeros(F + 1, dtype=np.int64)
    np.cumsum(per, out=off[1:])
    bbox = np.zeros((F, 4), dtype=np.int64)
    some = per > 0
    if some.any():
        at = off[:-1][some]                                              # (strictly ascending and < E: reduceat's segments are the features')
        xs, ys = e[:, [0, 2]], e[:, [1, 3]]
        bbox[some, 0] = np.minimum.reduceat(xs.min(axis=1), at)
        bbox[some, 1] = np.minimum.reduceat(ys.min(axis=1), at)
        bbox[some, 2] = np.maximum.reduceat(xs.max(axis=1), at)
        bbox[some, 3] = np.maximum.reduceat(ys.max(axis=1), at)
    return Zones(e.astype(np.int32).reshape(-1, 4), off.astype(np.int32), bbox)


# ---- the work list --------------------------------------------------------------------------------------------------------------------------
def _shape(fn, H, W):
    if any(isinstance(s, bool) or not isinstance(s, (int, np.integer)) for s in (H, W)) or H < 1 or W < 1:
        raise ValueError(f"{fn}: H={H!r}, W={W!r} must be positive integers")
    H, W = int(H), int(W)
    if H * W >= 2 ** 31:
        raise ValueError(f"{fn}: a raster of {H} x {W} pixels; H * W must stay below 2^31")
    return H, W


def burn_tiles(zones, H, W):
    """-> (boxes (Z, 4) int32, tile_off (NT + 1,) int32, tile_feat (NF,) int32).  ``boxes``: per feature (x0, y0, x1, y1), half open, in
    pixels -- the rows y with ``Ymin <= 256 y + 128 < Ymax`` and the columns ``floor(Xmin / 256) .. ceil(Xmax / 256)``, clipped to the
    raster, exactly ``zone_items``' rows and columns; all zero for a feature with nothing inside.  The raster is cut into ``TILE`` x
    ``TILE`` tiles anchored at pixel (0, 0), NT = ceil(H / 64) * ceil(W / 64) in row-major order; tile t lists the features whose box meets
    it, ``tile_feat[tile_off[t]:tile_off[t + 1]]``, ascending.  A feature wholly outside the raster is in no list.  Host only."""
    fn = "burn_tiles"
    if not isinstance(zones, Zones):
        raise TypeError(f"{fn}: zones must come from zone_edges or feature_edges")
    H, W = _shape(fn, H, W)
    bb = zones.bbox.astype(np.int64).reshape(-1, 4)
    x0, x1 = np.maximum(bb[:, 0] >> 8, 0), np.minimum(-((-bb[:, 2]) >> 8), W)
    y0, y1 = np.maximum((bb[:, 1] + 127) >> 8, 0), np.minimum((bb[:, 3] + 127) >> 8, H)
    some = (x1 > x0) & (y1 > y0)
    boxes = np.where(some[:, None], np.stack([x0, y0, x1, y1], axis=1), 0).astype(np.int32).reshape(-1, 4)
    tiles_x, tiles_y = -(-W // TILE), -(-H // TILE)
    NT = tiles_x * tiles_y
    feat = np.nonzero(some)[0]
    tx0, ty0 = x0[feat] // TILE, y0[feat] // TILE
    nx, ny = (x1[feat] - 1) // TILE - tx0 + 1, (y1[feat] - 1) // TILE - ty0 + 1
    pairs = nx * ny
    NF = int(pairs.sum())
    if NF >= 2 ** 31:
        raise ValueError(f"{fn}: {NF} (feature, tile) pairs; the list is indexed in 32 bits")
    start = np.cumsum(pairs) - pairs
    which = np.repeat(np.arange(len(feat)), pairs)                       # the feature (its rank among those inside) of each pair
    local = np.arange(NF) - start[which]
    tile = (ty0[which] + local // nx[which]) * tiles_x + tx0[which] + local % nx[which]
    order = np.argsort(tile, kind="stable")                              # stable: each tile's list keeps the ascending feature order
    tile_off = np.zeros(NT + 1, dtype=np.int64)
    np.cumsum(np.bincount(tile, minlength=NT), out=tile_off[1:])
    return boxes, tile_off.astype(np.int32), feat[which[order]].astype(np.int32)


def _tables(zones, H, W, device):
    """-> (device pointers of edges, edge_off, boxes, tile_off, tile_feat; NT, NF).  The five tables go into one pinned host buffer (edges
    first: 16-byte aligned) and are uploaded by ONE non-blocking copy; the device buffer is kept on ``zones`` per raster size, device and
    stream, next to zone_sums' tables, so that the next call builds and uploads nothing."""
    key = ("burn", H, W, device.index, _lib.stream_ptr().value)
    hit = zones._device_tables.get(key)
    if hit is None:
        boxes, tile_off, tile_feat = burn_tiles(zones, H, W)
        parts = [zones.edges.reshape(-1), zones.edge_off, boxes.reshape(-1), tile_off, tile_feat]
        host = torch.empty(sum(p.size for p in parts) + 4, dtype=torch.int32).pin_memory()
        at, offs = 0, []
        for p in parts:
            host[at:at + p.size] = torch.from_numpy(np.ascontiguousarray(p, dtype=np.int32))
            offs.append(at)
            at += p.size
        dev = host.to(device, non_blocking=True)
        if len(zones._device_tables) >= 8:                              # (a few raster sizes at most; never an unbounded store)
            zones._device_tables.clear()
        hit = zones._device_tables[key] = (dev, [dev.data_ptr() + 4 * o for o in offs], len(tile_off) - 1, len(tile_feat))
    return hit[1:]


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------------
def _values(fn, values, Z, top):
    v = np.asarray(values)
    if v.dtype.kind not in "iu" or v.ndim != 1:
        raise ValueError(f"{fn}: values must be a 1-d array of integers (got {v.dtype} {v.shape})")
    if len(v) != Z:
        raise ValueError(f"{fn}: {len(v)} values for {Z} features")
    if len(v) and (v.min() < 0 or v.max() > top):
        raise ValueError(f"{fn}: a value outside 0..{top}")
    return np.ascontiguousarray(v, dtype=np.int32)


def burn(zones, values, H=None, W=None, dtype=torch.uint16, init=0, merge="last", out=None, keep=False):
    """-> the device raster (H, W) of ``dtype`` (torch.uint16 or torch.uint8): one srbh_burn call on the current stream, no
    synchronisation after the launch.  The values (4 bytes per feature) are uploaded first by a plain copy from pageable memory, which
    holds the host until it is done; the tables are uploaded once (pinned, non-blocking) and kept on ``zones``.  ``zones``: the features (``zone_edges`` / ``feature_edges``); ``values``: one integer per feature, 0..65535
    (0..255 for uint8).  ``merge``: ``"last"`` (the largest feature index wins) or ``"max"`` (the largest value wins).  A pixel in no
    feature gets ``init``.  ``out``: an existing device raster, or an interior view of one, written in place and returned (H, W and dtype
    are then its own); with ``keep=True``, which requires it, pixels in no feature keep its contents."""
    fn = "burn"
    if not isinstance(zones, Zones):
        raise TypeError(f"{fn}: zones must come from zone_edges or feature_edges")
    if len(zones) < 1:
        raise ValueError(f"{fn}: no features")
    if not isinstance(merge, str) or merge not in MERGES:
        raise ValueError(f"{fn}: merge={merge!r} is none of {tuple(MERGES)}")
    if out is not None:
        if not (torch.is_tensor(out) and out.dim() == 2):
            raise ValueError(f"{fn}: out must be an (H, W) tensor (got {getattr(out, 'shape', type(out))})")
        if (H is not None and H != out.shape[0]) or (W is not None and W != out.shape[1]):
            raise ValueError(f"{fn}: H={H}, W={W} do not match out's {tuple(out.shape)}")
        if out.shape[1] > 1 and out.stride(1) != 1:
            raise ValueError(f"{fn}: out has stride {out.stride(1)} along W; it must be 1 (a band or a crop is fine, a transpose is not)")
        if out.shape[0] > 1 and out.stride(0) < out.shape[1]:
            raise ValueError(f"{fn}: out's rows overlap (row stride {out.stride(0)} below W={out.shape[1]})")
        H, W, dtype = out.shape[0], out.shape[1], out.dtype
    elif keep:
        raise ValueError(f"{fn}: keep=True needs the raster to keep: pass out")
    if dtype not in _TYPES:
        raise TypeError(f"{fn}: the raster is {dtype}; uint16 or uint8 (float and int16 rasters are out of scope)")
    H, W = _shape(fn, H, W)
    top = _TOP[dtype]
    if isinstance(init, bool) or not isinstance(init, (int, np.integer)) or not 0 <= init <= top:
        raise ValueError(f"{fn}: init={init!r} must be an integer in 0..{top}")
    vals = _values(fn, values, len(zones), top)
    # ---- everything above needs no device ----
    if out is None:
        if not torch.cuda.is_available():
            raise RuntimeError(f"{fn} (libsrbh): needs a ROCm device -- there is no CPU path")
        out = torch.empty((H, W), dtype=dtype, device=torch.device("cuda", torch.cuda.current_device()))
    out, rs = _on_device(fn, ("out", None), out, None)[:2]
    if len(zones.edges) == 0:                                            # no feature has an edge: nothing to launch
        if not keep:                                                     # (through int16: the fill of every torch build)
            (out.view(torch.int16).fill_(int(init) - 65536 if init >= 32768 else int(init)) if dtype == torch.uint16 else out.fill_(int(init)))
        return out
    with torch.cuda.device(out.device):
        ptrs, NT, NF = _tables(zones, H, W, out.device)
        dvals = torch.from_numpy(vals).to(out.device)                   # (pageable: blocks the host; they change from call to call)
        _lib.check(_lib.lib().srbh_burn(out.data_ptr(), _TYPES[dtype], rs, H, W, ptrs[0], ptrs[1], dvals.data_ptr(), ptrs[2], len(zones),
                                        len(zones.edges), ptrs[3], ptrs[4], NT, NF, MERGES[merge], int(bool(keep)), int(init),
                                        _lib.stream_ptr()), "srbh_burn")
    return out


def label_raster(zones, heights, H, W, scale=10):
    """-> device (H, W) uint16: the reference height raster of ``city_validation`` / ``cell_errors`` / ``urban_centre_validation`` in
    ``predict_city``'s units.  ``heights``: one height per feature, in metres; a feature burns ``round_half_even(scale * h)`` clamped to
    0..65535 (0.05 -> 0, 0.15 -> 2 at scale 10), later features over earlier ones, 0 where there is no building.  A NaN or negative
    height is refused."""
    fn = "label_raster"
    h = np.asarray(heights, dtype=np.float64)
    if h.ndim != 1:
        raise ValueError(f"{fn}: heights must be 1-d (got {h.shape})")
    if not isinstance(scale, (int, float, np.integer, np.floating)) or isinstance(scale, bool) or not np.isfinite(scale) or scale <= 0:
        raise ValueError(f"{fn}: scale={scale!r} must be a positive number")
    if np.isnan(h).any() or (h < 0).any():
        raise ValueError(f"{fn}: a height that is NaN or negative")
    v = np.minimum(np.rint(float(scale) * h), 65535.0).astype(np.int64)   # (rint rounds half to even)
    return burn(zones, v, H, W, torch.uint16, 0, "last")


def zone_raster(zones, H, W):
    """-> device (H, W) uint16: ``index + 1`` of the last zone that holds the pixel, 0 where none does.  Z <= 65535."""
    if isinstance(zones, Zones) and len(zones) > 65535:
        raise ValueError(f"zone_raster: {len(zones)} zones; a uint16 raster numbers 65535 at most")
    return burn(zones, np.arange(1, (len(zones) if isinstance(zones, Zones) else 0) + 1, dtype=np.int64), H, W, torch.uint16, 0, "last")
