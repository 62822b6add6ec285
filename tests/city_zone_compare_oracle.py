"""The pair sums per polygon zone in numpy int64 and Python integers, one zone at a time: what srbh_zone_pair_sums must return.  A helper
of tests/test_city_zone_compare_cpu.py and tests/test_gpu_city_zone_compare.py, not a test.  Written from the definition include/srbh.h
states, not from the kernel: tests/city_zones_oracle.py's ``zone_mask`` gives the membership (pinned there against a Fraction crossing
count), tests/city_compare_oracle.py's ``_compared`` the pair test, and the ten sums are taken over ``mask & compared``.

``mistake`` turns ONE rule into a plausible wrong one; tests/test_city_zone_compare_cpu.py asserts that each of them changes the result
on the GPU tests' own inputs:
  'zone_or'        the zone's bits ORed with the selection instead of ANDed
  'mask_on_count'  the third raster's test applied to count
  'r_minus_p'      d = r - p
  'or_in_both'     "both" implemented as "any"
  'corner'         the pixel's centre taken at its corner"""
import numpy as np

from tests import city_compare_oracle as CO
from tests import city_zones_oracle as ZO

MISTAKES = ("zone_or", "mask_on_count", "r_minus_p", "or_in_both", "corner")


def zone_row(pred, ref, zm, mask=None, mode="any", pthr=0, rthr=0, mthr=0, mistake=None):
    """the ten integers of one zone whose membership is the (H, W) bool ``zm``"""
    p, r = pred.astype(np.int64), ref.astype(np.int64)
    m = None if mask is None else mask.astype(np.int64)
    compared = CO._compared(p, r, m, mode, pthr, rthr, mthr, mistake)
    sel = (zm | compared) if mistake == "zone_or" else (zm & compared)
    count = int(zm.sum())
    if mistake == "mask_on_count" and m is not None:
        count = int((zm & (m > mthr)).sum())
    return CO._ten(p, r, sel, count, mistake)


def zone_pair_sums(pred, ref, polygons, mask=None, mode="any", pthr=0, rthr=0, mthr=0, mistake=None, masks=None, geotransform=None):
    """(Z, 10) int64 [count, n, sd, sad, sdd, sp, sr, spp, srr, spr].  ``masks``: the zones' memberships where the caller has them
    already (ZO.masks of the same polygons)"""
    H, W = pred.shape
    if masks is None:
        masks = ZO.masks(polygons, H, W, "corner" if mistake == "corner" else None, geotransform)
    rows = [zone_row(pred, ref, zm, mask, mode, pthr, rthr, mthr, mistake) for zm in masks]
    return np.array(rows, dtype=np.int64).reshape(-1, 10)


def urban_centre_validation(height, ref, build, polygons, bin_width=10, nbins=256, num_class=7):
    """ZO.urban_centre_table's dict extended by CO.errors of the zones' rows under cell_errors' defaults"""
    out = ZO.urban_centre_table(height, build, polygons, bin_width, nbins, num_class)
    err = CO.errors(zone_pair_sums(height, ref, polygons, build))
    for k in ("me", "mae", "rmse", "mean_pred", "mean_ref", "r", "r2"):
        out[k] = err[k]
    out["n_compared"] = err["n"]
    return out


# ---- the inputs of the GPU tests ----------------------------------------------------------------------------------------------------------------
H0, W0 = ZO.H0, ZO.W0
NAMED = {**ZO.rule_zones(), **ZO.clip_zones()}
NAMES = list(NAMED)
POLYS = list(NAMED.values()) + ZO.fan()


def window_zones(pos):
    """integer rectangles (xoff, yoff, xcount, ycount) as zones"""
    return [[ZO.rect(x, y, x + w, y + h)] for x, y, w, h in np.asarray(pos).tolist()]


def threshold_rasters():
    """131 x 70 rasters of the values next to every threshold the tests use"""
    rs = np.random.RandomState(5)
    v = np.array(CO.THRESHOLD_VALUES, dtype=np.uint16)
    p, r = v[rs.randint(0, len(v), size=(H0, W0))], v[rs.randint(0, len(v), size=(H0, W0))]
    m = np.array((0, 1, 6, 7, 254, 255), dtype=np.uint8)[rs.randint(0, 6, size=(H0, W0))]
    return p, r, m


def long_case(H, W):
    """(polygons, pred, ref, mask) of an elongated raster: a pentagon that reaches outside, a zone of two parts (one across the column
    8192 or the row 2047), and the whole raster"""
    if W > H:
        polys = [[ZO.ring((-5, -1), (W + 10, 0.2), (W - 9.5, H + 0.5), (W / 2 + 0.25, H / 2), (10, H - 0.1))],
                 [ZO.rect(8191.5, 0, 8192.5, H), ZO.ring((100.5, 0.5), (W - 100.5, 0.5), (W / 3, H - 0.5))], [ZO.rect(0, 0, W, H)]]
    else:
        polys = [[ZO.ring((-1, -5), (0.2, H + 10), (W + 0.5, H - 9.5), (W / 2, H / 2 + 0.25), (W - 0.1, 10))],
                 [ZO.ring((0.5, 100.5), (2.5, 2047.5), (0.5, H - 100.5))], [ZO.rect(0, 0, W, H)]]
    tp, tr = (np.uint8, np.uint16) if W == 70000 or W == 3000 else (np.uint16, np.uint8)
    p, r, m = CO.triple(tp, tr, np.uint8, H, W, seed=6)
    return polys, p, r, m
