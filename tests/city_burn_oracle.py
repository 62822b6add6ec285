"""Footprints burned into a raster in numpy, one feature at a time: what srbh_burn must store.  A helper of tests/test_city_burn_cpu.py and
tests/test_gpu_city_burn.py, not a test.  Written from the definition include/srbh.h states, not from the kernel: per feature the mask of
tests/city_zones_oracle.zone_mask (which the CPU test pins against a fractions.Fraction crossing count on overlapping features), painted
in feature order for "last" and through numpy.maximum for "max".  GDAL cannot be run where this project is built: no result of it is
compared.

``rule`` names a MISTAKE for the tests that show the comparison is not blind: 'first' (the first feature wins), 'last_as_max' ("last"
done as "max"), 'or_rings' (a feature's rings ORed instead of even-odd), 'init_under_keep' (init written under keep), 'corner' (the centre
taken at the pixel's corner), 'zero_skips' (a value of 0 treated as "no burn")."""
import numpy as np

from tests import city_zones_oracle as ZO

H0, W0 = ZO.H0, ZO.W0
MISTAKES = ("first", "last_as_max", "or_rings", "init_under_keep", "corner", "zero_skips")


def shifted(polygons, dx, dy=0.0):
    """the polygons moved by whole pixels (exact in float64 for the coordinates used here)"""
    return [[np.asarray(r, dtype=np.float64).reshape(-1, 2) - (dx, dy) for r in zone] for zone in polygons]


def feature_masks(polygons, H, W, rule=None):
    """one (H, W) bool mask per feature"""
    zrule = "corner" if rule == "corner" else None
    out = []
    for zone in polygons:
        if rule == "or_rings":
            m = np.zeros((H, W), dtype=bool)
            for ring in zone:
                m |= ZO.zone_mask(ZO.zone_edge_list([ring]), H, W)
        else:
            m = ZO.zone_mask(ZO.zone_edge_list(zone), H, W, zrule)
        out.append(m)
    return out


def paint(masks, values, H, W, dtype, init=0, merge="last", base=None, rule=None):
    """the raster: ``base`` is the raster kept under keep (None: no keep, pixels in no feature get init)"""
    values = [int(v) for v in values]
    assert len(values) == len(masks) and all(0 <= v <= np.iinfo(dtype).max for v in values)
    out = np.zeros((H, W), dtype=np.int64)
    burned = np.zeros((H, W), dtype=bool)
    if rule == "last_as_max" and merge == "last":
        merge = "max"
    order = range(len(masks))
    if rule == "first":
        order = reversed(order)
    for f in order:
        m = masks[f]
        if rule == "zero_skips" and values[f] == 0:
            continue
        if merge == "last":
            out[m] = values[f]
        else:
            out[m] = np.where(burned[m], np.maximum(out[m], values[f]), values[f])
        burned |= m
    back = np.full((H, W), init, dtype=np.int64) if base is None or rule == "init_under_keep" else base.astype(np.int64)
    return np.where(burned, out, back).astype(dtype)


def burn(polygons, values, H, W, dtype, init=0, merge="last", base=None, rule=None):
    return paint(feature_masks(polygons, H, W, rule), values, H, W, dtype, init, merge, base, rule)


def cover(masks):
    """(H, W) int: how many features hold each pixel"""
    return sum(m.astype(np.int64) for m in masks)


# ---- the inputs of the GPU test (here, so that the CPU test can show that no mistaken rule passes them and that they hold the cases) ----------
def values_for(n, dtype, seed, kind="distinct"):
    """'distinct': a random permutation of 1..n folded into the type (distinct for n <= the type's maximum); 'cycle': 0, 1, the type's
    maximum and a random value in turn"""
    rs = np.random.RandomState(seed)
    top = int(np.iinfo(dtype).max)
    if kind == "distinct":
        return (1 + rs.permutation(n) % top).tolist()
    rnd = rs.randint(0, top + 1, size=n)
    return [(0, 1, top, int(rnd[i]))[i % 4] for i in range(n)]


def seam_zones():
    """features across the tile seams x = 63|64, 127|128 and y = 63|64 of the 70 x 131 raster, three and more deep, a later 0 among them"""
    return [[ZO.rect(60.5, 58.5, 67.5, 68.5)], [ZO.ring((61, 60), (70, 62.5), (62, 69))], [ZO.rect(62.5, 61.5, 66.5, 66.5)],
            [ZO.rect(124.5, 60.5, 130.5, 67.5)], [ZO.ring((120, 55), (131, 64), (122, 70))], [ZO.rect(126.5, 62.5, 129.5, 65.5)],
            [ZO.rect(63.5, 63.5, 64.5, 64.5)], [ZO.rect(0, 63, 131, 65), ZO.rect(20.5, 63, 40.5, 65)], [ZO.rect(127, 0, 129, 70)]]


SEAM_VALUES = {np.uint16: [700, 65535, 0, 9, 300, 0, 5, 77, 2], np.uint8: [200, 255, 0, 9, 30, 0, 5, 77, 2]}


def dense_zones(n=2000, seed=11):
    """n small triangles and quadrilaterals inside the first tile, many deep"""
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        c = rs.uniform(2, 62, size=2)
        pts = c + rs.uniform(-6, 6, size=(3 + i % 2, 2))
        grid = (256.0, 2.0, 1.0)[i % 3]
        out.append([np.round(np.clip(pts, 0, 64) * grid) / grid])
    return out


def cases(dtype):
    """name -> (polygons, values) on the H0 x W0 raster"""
    rule, clip, small, fan, dense = (list(ZO.rule_zones().values()), list(ZO.clip_zones().values()), ZO.small_zones(301), ZO.fan(),
                                     dense_zones())
    whole = ("everything", "beyond everything", "triangle at the limit")      # first, or "last" would show nothing but the last of them
    clip = [ZO.clip_zones()[k] for k in whole] + [z for k, z in ZO.clip_zones().items() if k not in whole]
    vr = values_for(len(rule), dtype, 21)
    return {
        "rule": (rule, vr), "rule reversed": (rule[::-1], vr[::-1]),
        "clip": (clip, values_for(len(clip), dtype, 22)),
        "empty features": ([[], rule[0], [], [ZO.ring((5, 5), (9, 9))], rule[4], []], values_for(6, dtype, 23)),
        "one": ([rule[3]], [7]),
        "small": (small, values_for(len(small), dtype, 24, "cycle")),
        "dense": (dense, values_for(len(dense), dtype, 25, "cycle")),
        "fan": (fan, values_for(8, dtype, 26)),
        "seams": (seam_zones(), SEAM_VALUES[dtype]),
    }
