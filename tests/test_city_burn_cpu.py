"""CPU: the host half of the burn -- the oracle tests/city_burn_oracle.py against a fractions.Fraction crossing count pixel by pixel on
overlapping features, city_burn.feature_edges against city_zones.zone_edges (arrays equal), burn_tiles (a pair is listed iff the feature's
pixel box meets the tile, ascending lists, boxes equal to zone_items' rows and columns), label_raster's rounding, the ABI declarations,
the refusals of the Python layer, and -- so that the GPU comparison is not blind -- that each of six mistaken rules changes the oracle's
raster on the GPU test's own inputs, and that those inputs hold the cases they are there for.  No kernel is launched here."""
import os

import numpy as np
import pytest
import torch

from srbh_amd import _lib
from srbh_amd import city_burn as CB
from srbh_amd import city_zones as CZ
from tests import city_burn_oracle as BO
from tests import city_zones_oracle as ZO

H0, W0 = BO.H0, BO.W0


# ---- the oracle itself ----------------------------------------------------------------------------------------------------------------------
def test_oracle_equals_the_fraction_crossing_count_on_overlapping_features():
    rs = np.random.RandomState(1)
    H, W = 9, 11
    deep = pixels = 0
    for i in range(21):
        grid = (256.0, 2.0, 1.0)[i % 3]
        polys = []
        for k in range(5):
            zone = [np.round(rs.uniform(-2, 13, size=(3 + rs.randint(0, 3), 2)) * grid) / grid for _ in range(1 + (k == 2))]
            polys.append(zone)
        values = rs.randint(0, 4, size=5).tolist()
        masks = [ZO.fraction_mask(ZO.zone_edge_list(z), H, W)[0] for z in polys]
        for merge in ("last", "max"):
            got = BO.burn(polys, values, H, W, np.uint8, 9, merge)
            for y in range(H):
                for x in range(W):
                    inside = [f for f in range(5) if masks[f][y, x]]
                    want = 9 if not inside else (values[inside[-1]] if merge == "last" else max(values[f] for f in inside))
                    assert got[y, x] == want, (i, merge, y, x)
        deep += int((BO.cover(masks) >= 3).sum())
        pixels += H * W
    assert pixels > 2000 and deep > 100, (pixels, deep)
    base = rs.randint(0, 256, size=(H, W)).astype(np.uint8)
    kept, last = BO.burn(polys, values, H, W, np.uint8, 9, "last", base), BO.burn(polys, values, H, W, np.uint8, 9, "last")
    none = BO.cover(masks) == 0
    assert none.any() and np.array_equal(kept[none], base[none]) and (last[none] == 9).all() and np.array_equal(kept[~none], last[~none])


# ---- feature_edges == zone_edges ----------------------------------------------------------------------------------------------------------------
def flat(polygons):
    rings = [np.asarray(r, dtype=np.float64).reshape(-1, 2) for z in polygons for r in z]
    vertices = np.concatenate(rings) if rings else np.zeros((0, 2))
    ring_off = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int64)
    feature_off = np.concatenate([[0], np.cumsum([len(z) for z in polygons])]).astype(np.int64)
    return vertices, ring_off, feature_off


def same_zones(a, b):
    return (a.edges.dtype == b.edges.dtype == np.int32 and a.edge_off.dtype == b.edge_off.dtype == np.int32 and a.bbox.dtype == b.bbox.dtype
            and a.edges.shape == b.edges.shape and np.array_equal(a.edges, b.edges) and np.array_equal(a.edge_off, b.edge_off)
            and np.array_equal(a.bbox, b.bbox))


@pytest.mark.parametrize("name", ["rule", "clip", "small", "closing and degenerate", "empty list of rings"])
def test_feature_edges_equals_zone_edges(name):
    t = 1 / 512
    tri = np.array([(0.0 + t, 0.0), (1.0 + t, 3.0 + 3 * t), (2 / 256 + t, 5.0)])
    polys = {"rule": list(ZO.rule_zones().values()), "clip": list(ZO.clip_zones().values()), "small": ZO.small_zones(301),
             "closing and degenerate": [[tri], [np.concatenate([tri, tri[:1]])], [], [ZO.ring((1, 1), (5, 5))],
                                        [ZO.ring((1, 1), (5, 5), (1, 1 + 1 / 1024), (5, 5))],
                                        [ZO.rect(0, 0, 2, 2), ZO.ring((7, 7), (7, 7), (7, 7)), ZO.ring((3, 3), (4, 5), (5, 3))], [ZO.rect(1, 1, 4, 3)]],
             "empty list of rings": [[], []]}[name]
    want, got = CZ.zone_edges(polys), CB.feature_edges(*flat(polys))
    assert isinstance(got, CZ.Zones) and len(got) == len(polys) and same_zones(got, want)
    if name == "clip":
        assert np.abs(got.edges).max() == 2 ** 29
    if name == "closing and degenerate":
        assert got.edge_off.tolist() == [0, 3, 6, 6, 6, 6, 10, 12]


def test_feature_edges_geotransform_and_refusals():
    gt = (500000.0, 2.5, 0.0, 4100000.0, 0.0, -2.5)                      # north up: dy < 0
    px = [[ZO.ring((3.25, 1.5), (40.5, 7), (12, 33.125))], [ZO.rect(5, 5, 9, 8), ZO.rect(6, 6, 7, 7)]]
    world = [[np.stack([gt[0] + r[:, 0] * gt[1], gt[3] + r[:, 1] * gt[5]], axis=1) for r in z] for z in px]
    a = CB.feature_edges(*flat(world), geotransform=gt)
    assert same_zones(a, CZ.zone_edges(world, gt)) and same_zones(a, CZ.zone_edges(px)) and a.edges[:, 1].min() == 384
    v, ro, fo = flat(px)
    for bad in ((0, 1, 0.1, 0, 0, -1), (0, 1, 0, 0, -0.2, -1), (0, 1, 0, 0, 0), (0, 0, 0, 0, 0, -1)):
        with pytest.raises(ValueError, match="geotransform"):
            CB.feature_edges(v, ro, fo, bad)
    lim = float(2 ** 21)
    assert CB.feature_edges(*flat([[ZO.ring((-lim, 0), (lim, 1), (0, lim))]])).edges.max() == 2 ** 29
    for bad in (ZO.ring((0, 0), (lim + 1 / 256, 1), (0, 5)), ZO.ring((0, 0), (np.nan, 1), (0, 5)), ZO.ring((0, 0), (np.inf, 1), (0, 5))):
        with pytest.raises(ValueError, match="feature_edges"):
            CB.feature_edges(*flat([[bad]]))
    for args in ((np.zeros((4, 3)), [0, 4], [0, 1]), (v, ro[:-1], fo), (v, ro, fo[1:]), (v, ro[::-1].copy(), fo), (v, ro.astype(np.float64), fo),
                 (v, ro, [0, 5])):
        with pytest.raises(ValueError, match="feature_edges"):
            CB.feature_edges(*args)


# ---- burn_tiles ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(H0, W0), (64, 128), (3, 700), (200, 5)])
def test_burn_tiles_lists_a_pair_iff_the_box_meets_the_tile(H, W):
    polys = list(ZO.rule_zones().values()) + list(ZO.clip_zones(H, W).values()) + ZO.small_zones(60, H, W) + BO.seam_zones()
    names = list(ZO.rule_zones()) + list(ZO.clip_zones(H, W))
    z = CZ.zone_edges(polys)
    boxes, tile_off, tile_feat = CB.burn_tiles(z, H, W)
    T = CB.TILE
    tiles_x, tiles_y = -(-W // T), -(-H // T)
    assert boxes.dtype == tile_off.dtype == tile_feat.dtype == np.int32 and boxes.shape == (len(polys), 4)
    assert len(tile_off) == tiles_x * tiles_y + 1 and tile_off[0] == 0 and tile_off[-1] == len(tile_feat) and (np.diff(tile_off) >= 0).all()
    items, item_off = CZ.zone_items(z, H, W, 2 ** 40)                     # one item per zone that has anything inside
    for f in range(len(polys)):
        mine = items[item_off[f]:item_off[f + 1]]
        want = [0, 0, 0, 0] if len(mine) == 0 else [mine[0, 1], mine[0, 2], mine[0, 1] + mine[0, 3], mine[0, 2] + mine[0, 4]]
        assert boxes[f].tolist() == want, f
    for t in range(tiles_x * tiles_y):
        ty, tx = divmod(t, tiles_x)
        mine = tile_feat[tile_off[t]:tile_off[t + 1]].tolist()
        assert all(a < b for a, b in zip(mine, mine[1:])), t              # strictly ascending
        want = [f for f, (x0, y0, x1, y1) in enumerate(boxes.tolist())
                if x1 > x0 and y1 > y0 and x0 < (tx + 1) * T and x1 > tx * T and y0 < (ty + 1) * T and y1 > ty * T]
        assert mine == want, t
    listed = set(tile_feat.tolist())
    for k, name in enumerate(names):
        if name.startswith("wholly") or name in ("empty", "degenerate ring only"):
            assert k not in listed and boxes[k].tolist() == [0] * 4, name
    assert len(listed) > 20
    # every pixel of a feature lies inside its box
    for f, m in enumerate(BO.feature_masks(polys[:14], H, W)):
        ys, xs = np.nonzero(m)
        if len(ys):
            x0, y0, x1, y1 = boxes[f].tolist()
            assert xs.min() >= x0 and xs.max() < x1 and ys.min() >= y0 and ys.max() < y1, f


def test_burn_tiles_refusals():
    z = CZ.zone_edges([[ZO.rect(1, 1, 5, 5)]])
    with pytest.raises(TypeError, match="burn_tiles"):
        CB.burn_tiles([[ZO.rect(1, 1, 5, 5)]], 8, 9)
    for H, W in ((0, 9), (8, -1), (2 ** 16, 2 ** 15), (8.0, 9)):
        with pytest.raises(ValueError, match="burn_tiles"):
            CB.burn_tiles(z, H, W)
    # 2^31 pairs are refused before anything of that size is made: 2^13 features over all 2^18 tiles of a 32768 x 32768 raster
    big = CZ.Zones(np.zeros((0, 4), np.int32), np.zeros(8193, np.int32), np.tile(np.array([[0, 0, 2 ** 23, 2 ** 23]], np.int64), (8192, 1)))
    with pytest.raises(ValueError, match="pairs"):
        CB.burn_tiles(big, 32768, 32768)


# ---- label_raster's rounding, without a device ---------------------------------------------------------------------------------------------------
def test_label_raster_rounds_half_to_even_and_clamps(monkeypatch):
    seen = {}

    def fake(zones, values, H, W, dtype, init, merge):
        seen.update(values=np.asarray(values).tolist(), dtype=dtype, init=init, merge=merge, shape=(H, W))
        return "raster"

    monkeypatch.setattr(CB, "burn", fake)
    z = CZ.zone_edges([[ZO.rect(1, 1, 5, 5)]] * 9)
    assert CB.label_raster(z, [0.05, 0.15, 0.25, 12.34, 0.0, 6553.5, 6553.6, 1e9, np.inf], 8, 9) == "raster"
    assert seen["values"] == [0, 2, 2, 123, 0, 65535, 65535, 65535, 65535]
    assert seen["dtype"] == torch.uint16 and seen["init"] == 0 and seen["merge"] == "last" and seen["shape"] == (8, 9)
    CB.label_raster(z, [1.5] * 9, 8, 9, scale=1)
    assert seen["values"] == [2] * 9
    for bad in ([np.nan] + [1.0] * 8, [-0.01] + [1.0] * 8, [[1.0] * 9]):
        with pytest.raises(ValueError, match="label_raster"):
            CB.label_raster(z, bad, 8, 9)
    for scale in (0, -1, np.nan, "10"):
        with pytest.raises(ValueError, match="scale"):
            CB.label_raster(z, [1.0] * 9, 8, 9, scale=scale)


# ---- the ABI and the Python refusals ---------------------------------------------------------------------------------------------------------------
def test_abi_declarations():
    assert "srbh_burn.hip" in _lib.SOURCES and os.path.exists(os.path.join(_lib.CSRC, "srbh_burn.hip"))
    header = open(os.path.join(_lib.INCLUDE, "srbh.h")).read()
    for name in ("srbh_burn_tile", "srbh_burn"):
        assert name + "(" in header and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["srbh_burn"][1]) == 19 and _lib.SIGNATURES["srbh_burn_tile"][1] == []
    assert "#define SRBH_BURN_LAST 0" in header and "#define SRBH_BURN_MAX 1" in header and CB.MERGES == {"last": 0, "max": 1}
    assert CB.TILE == 64 and "64: the tile side" in header
    import srbh_amd.city_burn as mod                                    # the alias package resolves the new module
    assert mod.burn is CB.burn and set(mod.__all__) >= {"feature_edges", "burn_tiles", "burn", "label_raster", "zone_raster"}


def test_python_layer_refusals_need_no_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device was asked for before the arguments were judged")

    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(torch.cuda, "current_device", no_device)
    monkeypatch.setattr(torch, "empty", no_device)
    z = CZ.zone_edges([[ZO.rect(1, 1, 5, 5)], [ZO.rect(2, 2, 6, 6)]])
    host8, host16 = torch.zeros((8, 9), dtype=torch.uint8), torch.zeros((8, 9), dtype=torch.uint16)
    with pytest.raises(TypeError, match="burn"):
        CB.burn([[ZO.rect(1, 1, 5, 5)]], [1], 8, 9)
    with pytest.raises(ValueError, match="no features"):
        CB.burn(CZ.zone_edges([]), [], 8, 9)
    for values in ([1], [1, 2, 3], [1.0, 2.0], [-1, 2], [1, 65536], [[1, 2]], [True, False]):
        with pytest.raises(ValueError, match="value"):
            CB.burn(z, values, 8, 9)
    with pytest.raises(ValueError, match="value"):
        CB.burn(z, [1, 256], 8, 9, dtype=torch.uint8)
    with pytest.raises(ValueError, match="value"):
        CB.burn(z, [1, 256], out=host8)
    for kw in (dict(merge="add"), dict(merge=0), dict(init=-1), dict(init=65536), dict(init=1.0), dict(init=True), dict(keep=True),
               dict(H=0), dict(W=-2), dict(H=None), dict(H=2 ** 16, W=2 ** 15)):
        with pytest.raises(ValueError, match="burn"):
            CB.burn(z, [1, 2], **{"H": 8, "W": 9, **kw})
    with pytest.raises(ValueError, match="init"):
        CB.burn(z, [1, 2], 8, 9, dtype=torch.uint8, init=256)
    for dtype in (torch.int16, torch.float32, torch.int32):
        with pytest.raises(TypeError, match="burn"):
            CB.burn(z, [1, 2], 8, 9, dtype=dtype)
    with pytest.raises(TypeError, match="burn"):
        CB.burn(z, [1, 2], out=host16.to(torch.int16))
    for out, kw in ((host16.t(), {}), (host16, dict(H=9)), (host16, dict(W=8)), (torch.zeros(9, dtype=torch.uint16), {}),
                    (host16[:1].expand(8, 9), {}), (np.zeros((8, 9), np.uint16), {})):
        with pytest.raises(ValueError, match="burn"):
            CB.burn(z, [1, 2], out=out, **kw)
    with pytest.raises(ValueError, match="65535"):
        CB.zone_raster(CZ.Zones(np.zeros((0, 4), np.int32), np.zeros(65537, np.int32), np.zeros((65536, 4), np.int64)), 8, 9)
    monkeypatch.undo()
    # sound arguments reach the device question last: a host raster is refused there, and only there
    with pytest.raises(RuntimeError, match="no CPU"):
        CB.burn(z, [1, 2], out=host16)
    with pytest.raises(RuntimeError, match="no CPU"):
        CB.burn(z, [1, 2], out=host8, keep=True, merge="max", init=255)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU"):
            CB.burn(z, [1, 2], 8, 9)
        with pytest.raises(RuntimeError, match="no CPU"):
            CB.label_raster(z, [1.0, 2.5], 8, 9)
        with pytest.raises(RuntimeError, match="no CPU"):
            CB.zone_raster(z, 8, 9)


# ---- the comparison is not blind ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_inputs():
    """per type the GPU test's cases with their masks, computed once"""
    masks = {name: BO.feature_masks(polys, H0, W0) for name, (polys, _) in BO.cases(np.uint16).items()}      # (the polygons are the same)
    return {dtype: {name: (polys, values, masks[name]) for name, (polys, values) in BO.cases(dtype).items()} for dtype in (np.uint16, np.uint8)}


@pytest.mark.parametrize("mistake", BO.MISTAKES)
def test_a_mistaken_rule_changes_the_gpu_tests_rasters(gpu_inputs, mistake):
    rs = np.random.RandomState(5)
    for dtype, cases in gpu_inputs.items():
        base = rs.randint(0, np.iinfo(dtype).max + 1, size=(H0, W0)).astype(dtype)
        changed = []
        for name, (polys, values, masks) in cases.items():
            if name == "dense":
                continue
            keep = mistake == "init_under_keep"
            right = BO.paint(masks, values, H0, W0, dtype, 7, "last", base if keep else None)
            wrong_masks = BO.feature_masks(polys, H0, W0, mistake) if mistake in ("or_rings", "corner") else masks
            wrong = BO.paint(wrong_masks, values, H0, W0, dtype, 7, "last", base if keep else None, mistake)
            if not np.array_equal(right, wrong):
                changed.append(name)
        assert changed, (mistake, dtype)
        want = {"first": {"rule", "rule reversed", "small", "seams"}, "last_as_max": {"rule", "small", "seams"}, "or_rings": {"rule"},
                "init_under_keep": {"rule", "one", "small"}, "corner": {"rule", "fan", "clip"}, "zero_skips": {"small", "seams"}}[mistake]
        assert want <= set(changed), (mistake, dtype, changed)


def test_the_gpu_inputs_hold_the_cases(gpu_inputs):
    for dtype, cases in gpu_inputs.items():
        deep = later_zero = 0
        for name, (polys, values, masks) in cases.items():
            deep += int((BO.cover(masks) >= 3).sum())
            # a later 0 over an earlier non-zero: where the last feature's value is 0 and an earlier one's is not
            last = np.full((H0, W0), -1, dtype=np.int64)
            nonzero_before = np.zeros((H0, W0), dtype=bool)
            for m, v in zip(masks, values):
                if v == 0:
                    later_zero += int((m & nonzero_before).sum())
                else:
                    nonzero_before |= m
                last[m] = v
        assert deep > 500 and later_zero > 50, (dtype, deep, later_zero)

        def straddles(axis, seam):
            """features with a pixel on both sides of the seam in one row (axis 1) or column (axis 0)"""
            n = 0
            for name, (polys, values, masks) in cases.items():
                for m in masks:
                    a, b = (m[:, seam - 1], m[:, seam]) if axis == 1 else (m[seam - 1, :], m[seam, :])
                    n += bool((a & b).any())
            return n

        assert straddles(1, 64) >= 5 and straddles(1, 128) >= 5 and straddles(0, 64) >= 5, dtype
    rule, rev = gpu_inputs[np.uint16]["rule"], gpu_inputs[np.uint16]["rule reversed"]
    assert not np.array_equal(BO.paint(rule[2], rule[1], H0, W0, np.uint16), BO.paint(rev[2], rev[1], H0, W0, np.uint16))
    fan = gpu_inputs[np.uint16]["fan"]
    assert (BO.cover(fan[2]) == 1).all()                                 # disjoint and covering: "last" == "max", zone_raster non-zero
    assert np.array_equal(BO.paint(fan[2], fan[1], H0, W0, np.uint16), BO.paint(fan[2], fan[1], H0, W0, np.uint16, merge="max"))
    dense = gpu_inputs[np.uint16]["dense"]
    assert len(dense[0]) == 2000 and BO.cover(dense[2]).max() >= 12 and not BO.cover(dense[2])[:, 64:].any() and not BO.cover(dense[2])[64:].any()
