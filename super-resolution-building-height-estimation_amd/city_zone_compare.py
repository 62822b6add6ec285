"""Urban-centre validation: how good a predicted city is against a reference height raster on the same grid, PER POLYGON ZONE.

The paper reports per urban centre; ``city_zones`` gives a centre's own table (mean and std of building height in each polygon) and
``city_compare`` the agreement with a reference raster per rectangular window, per height class or per block.  Here the two meet, over
``harness.predict_city``'s ``(height uint16, class uint8)``, a reference height raster on the same grid and ``city_zones.zone_edges``'
``Zones``:

* ``zone_pair_sums``           per zone ``[count, n, sd, sad, sdd, sp, sr, spp, srr, spr]``, every zone in ONE libsrbh call
  (csrc/srbh_zone_compare.hip), exact integers;
* ``zone_errors``              ``city_compare.errors_from_sums`` of that table: n, count, fraction, me, mae, rmse, the means, Pearson r, r2;
* ``urban_centre_validation``  ``city_zones.urban_centre_table``'s per-centre arrays extended by the error measures, one read-back.

THE RULE is the conjunction of the two modules' rules, each unchanged.  A pixel enters the nine sums when it is IN THE ZONE (city_zones:
vertices quantised to int32 fixed point with 8 fractional bits, even-odd over all rings, the pixel's centre decides, a centre on a left or
top boundary is in) and COMPARED (city_compare: inside the raster, the pair test of ``mode`` -- with ``P := p > pred_threshold`` and
``R := r > ref_threshold``: ``"any"`` P or R, ``"both"`` P and R, ``"ref"`` R, ``"pred"`` P -- and no mask or ``mask >
mask_threshold``).  ``count`` is the zone's pixels inside the raster, as ``zone_sums`` gives it: no test of the comparison applies to
it.  ``d = pred - ref``, signed.  Raster units throughout.

GPU only.  A per-zone ``class_sums`` (a HeightMetric per centre), a reference raster of another resolution and warping, int16 and float
rasters, shapefiles and GeoTIFFs are out of scope."""
import torch

from . import _lib
from .city_compare import _abi, _device_rasters, _rasters, errors_from_sums
from .city_grid import _workspace
from .city_zones import ITEM_PIXELS, _centre_table, _check_zones, _tables

__all__ = ["zone_pair_sums", "zone_errors", "urban_centre_validation"]

_ERROR_NAMES = ("me", "mae", "rmse", "mean_pred", "mean_ref", "r", "r2")


def zone_pair_sums(pred, ref, zones, mask=None, mode="any", pred_threshold=0, ref_threshold=0, mask_threshold=0, item_pixels=ITEM_PIXELS,
                   workspace=None):
    """-> device (Z, 10) int64 ``[count, n, sd, sad, sdd, sp, sr, spp, srr, spr]`` per zone, one srbh_zone_pair_sums call on the current
    stream, no synchronisation.  ``pred`` / ``ref`` / ``mask``: (H, W) device tensors of uint16 or uint8, read in place (stride 1 along
    W, any row stride).  ``zones``: city_zones.zone_edges' tables; the uploaded tables are city_zones' own, so a call after ``zone_sums``
    on the same ``Zones`` uploads nothing.  ``count`` = the zone's pixels inside the raster, ``n`` = the compared ones; the other eight
    are pair_sums' over those.  A zone without edges or wholly outside the raster gives zeros.  ``workspace``: optional device buffer to
    reuse between calls (srbh_zone_pair_ws_bytes(number of items) bytes; its content does not matter)."""
    fn = "zone_pair_sums"
    H, W, mode, pthr, rthr, mthr = _rasters(fn, pred, ref, mask, mode, pred_threshold, ref_threshold, mask_threshold)
    item_pixels = _check_zones(fn, zones, item_pixels)
    _workspace(fn, workspace)                                            # (before a device is asked for)
    pred, rs_p, ref, rs_r, mask, rs_m = _device_rasters(fn, pred, ref, mask)
    device = pred.device
    with torch.cuda.device(device):
        ptrs, Z, E, NI = _tables(zones, H, W, item_pixels, device)
    out = torch.empty((Z, 10), dtype=torch.int64, device=device)
    if E == 0 or NI == 0:                                                 # nothing of any zone lies inside the raster
        return out.zero_()
    ws = _workspace(fn, workspace, _lib.lib().srbh_zone_pair_ws_bytes(NI), device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().srbh_zone_pair_sums(*_abi(pred, rs_p, ref, rs_r, mask, rs_m, H, W), ptrs[0], ptrs[1], Z, E, ptrs[2], ptrs[3],
                                                  NI, mode, pthr, rthr, mthr, out.data_ptr(), ws.data_ptr(), _lib.stream_ptr()),
                   "srbh_zone_pair_sums")
    return out


def zone_errors(pred, ref, zones, build=None, **kw):
    """The per-zone agreement table of a predicted city and a reference height raster: errors_from_sums of zone_pair_sums(pred, ref,
    zones, build, **kw) -- by default the zone's pixels where either height is > 0 and, with ``build``, class > 0.  One call and one
    device-to-host copy of Z x 10 int64.  Raster units."""
    return errors_from_sums(zone_pair_sums(pred, ref, zones, build, **kw).cpu().numpy())


def urban_centre_validation(height, ref, build, zones, bin_width=10, nbins=256, num_class=7):
    """The urbanarea_meanstd row of each zone with its agreement against ``ref``: city_zones.urban_centre_table's dict of per-centre
    arrays (``mean``, ``std``, ``max``, ``n``, ``count``, ``fraction``, ``hist``, ``class_counts``) extended by ``me``, ``mae``,
    ``rmse``, ``mean_pred``, ``mean_ref``, ``r``, ``r2`` and ``n_compared`` -- zone_errors' numbers under cell_errors' defaults (the
    pixels where either height is > 0 and, with ``build``, class > 0).  Four calls (three without ``build``) on one set of uploaded
    tables, ONE torch.cat and ONE device-to-host copy for everything."""
    out, sums = _centre_table(height, build, zones, bin_width, nbins, num_class, lambda: zone_pair_sums(height, ref, zones, build))
    err = errors_from_sums(sums)
    for name in _ERROR_NAMES:
        out[name] = err[name]
    out["n_compared"] = err["n"]
    return out
