"""CPU: the host half of the polygon zones -- the oracle tests/city_zones_oracle.py against a fractions.Fraction crossing count pixel by
pixel, city_zones.zone_edges (quantisation ties, closing, degenerate rings, geotransforms, refusals) and zone_items (every in-range row in
exactly one item, nothing outside the raster) against the oracle's edge list, the partition property of the rule, zone_heights on
hand-made sums, the refusals of the Python layer, and -- so that the GPU comparison is not blind -- that each of three mistaken rules
changes the oracle's result on the GPU test's own zones.  No kernel is launched here."""
import numpy as np
import pytest
import torch

from srbh_amd import city_zones as CZ
from tests import city_summary_oracle as SO
from tests import city_zones_oracle as ZO

H0, W0 = ZO.H0, ZO.W0


def raster(dtype, H, W, seed, zeros=0.5):
    rs = np.random.RandomState(seed)
    a = rs.randint(0, np.iinfo(dtype).max + 1, size=(H, W)).astype(dtype)
    a[rs.rand(H, W) < zeros] = 0
    return a


# ---- the oracle itself ----------------------------------------------------------------------------------------------------------------------
def test_oracle_equals_the_fraction_crossing_count_pixel_by_pixel():
    rs = np.random.RandomState(1)
    pixels = on_edge = on_vertex = 0
    for i in range(150):
        H, W = 7 + i % 3, 9 - i % 2
        grid = (256.0, 2.0, 1.0)[i % 3]
        zone = []
        for _ in range(1 + (i % 4 == 0)):
            pts = rs.uniform(-2, max(H, W) + 2, size=(3 + rs.randint(0, 4), 2))
            zone.append(np.round(pts * grid) / grid)
        edges = ZO.zone_edge_list(zone)
        want, e, v = ZO.fraction_mask(edges, H, W)
        assert np.array_equal(ZO.zone_mask(edges, H, W), want), i
        pixels, on_edge, on_vertex = pixels + H * W, on_edge + e, on_vertex + v
    assert pixels > 9000 and on_edge > 20 and on_vertex > 100, (pixels, on_edge, on_vertex)


def test_boundary_ownership():
    """a centre on a left or top boundary is in, on a right or bottom boundary out; zones sharing an edge neither share nor miss a pixel"""
    m = ZO.masks([[ZO.rect(2.5, 1.5, 6.5, 4.5)]], 8, 9)[0]
    assert np.array_equal(np.argwhere(m), [(y, x) for y in (1, 2, 3) for x in (2, 3, 4, 5)])
    a, b = ZO.masks([[ZO.ring((1.5, 0.5), (6.5, 5.5), (1.5, 5.5))], [ZO.ring((1.5, 0.5), (6.5, 0.5), (6.5, 5.5))]], 8, 9)
    whole = ZO.masks([[ZO.rect(1.5, 0.5, 6.5, 5.5)]], 8, 9)[0]
    assert not (a & b).any() and np.array_equal(a | b, whole) and whole.sum() == 25 and a.sum() > 0 and b.sum() > 0


# ---- zone_edges -----------------------------------------------------------------------------------------------------------------------------
def edge_set(z, k):
    return sorted(map(tuple, z.edges[z.edge_off[k]:z.edge_off[k + 1]].tolist()))


def test_zone_edges_quantisation_closing_and_degenerate_rings():
    t = 1 / 512                                                          # a tie of the quantisation: half a unit
    tri = np.array([(0.0 + t, 0.0), (1.0 + t, 3.0 + 3 * t), (2 / 256 + t, 5.0)])
    z = CZ.zone_edges([[tri]])
    assert z.edges.dtype == np.int32 and z.edge_off.tolist() == [0, 3] and len(z) == 1
    assert edge_set(z, 0) == sorted([(0, 0, 256, 770), (256, 770, 2, 1280), (2, 1280, 0, 0)])          # 0.5 -> 0, 256.5 -> 256, 769.5 -> 770, 2.5 -> 2
    assert z.bbox.tolist() == [[0, 0, 256, 1280]]
    closed = np.concatenate([tri, tri[:1]])
    assert edge_set(CZ.zone_edges([[closed]]), 0) == edge_set(z, 0)
    # horizontal edges dropped; rings with fewer than 3 distinct vertices (after quantisation) contribute nothing; an empty zone stays
    z = CZ.zone_edges([[ZO.rect(1, 1, 4, 3)], [], [ZO.ring((1, 1), (5, 5))], [ZO.ring((1, 1), (5, 5), (1, 1 + 1 / 1024), (5, 5))],
                       [ZO.rect(0, 0, 2, 2), ZO.ring((7, 7), (7, 7), (7, 7)), ZO.ring((3, 3), (4, 5), (5, 3))]])
    assert z.edge_off.tolist() == [0, 2, 2, 2, 2, 6] and len(z) == 5
    assert edge_set(z, 0) == [(256, 768, 256, 256), (1024, 256, 1024, 768)] and z.bbox[1:4].tolist() == [[0] * 4] * 3
    polys = list(ZO.rule_zones().values()) + list(ZO.clip_zones().values()) + ZO.fan() + ZO.small_zones(30)
    z = CZ.zone_edges(polys)
    for k, zone in enumerate(polys):
        assert edge_set(z, k) == sorted(ZO.zone_edge_list(zone)), k
    assert np.abs(z.edges).max() == 2 ** 29


def test_zone_edges_geotransform_and_refusals():
    gt = (500000.0, 2.5, 0.0, 4100000.0, 0.0, -2.5)                      # north up: dy < 0
    px = ZO.ring((3.25, 1.5), (40.5, 7), (12, 33.125))
    world = np.stack([gt[0] + px[:, 0] * gt[1], gt[3] + px[:, 1] * gt[5]], axis=1)
    a, b = CZ.zone_edges([[world]], gt), CZ.zone_edges([[px]])
    assert np.array_equal(a.edges, b.edges) and np.array_equal(a.bbox, b.bbox) and a.edges[:, 1].min() == 384
    assert sorted(ZO.zone_edge_list([world], gt)) == edge_set(a, 0)
    for bad in ((0, 1, 0.1, 0, 0, -1), (0, 1, 0, 0, -0.2, -1), (0, 1, 0, 0, 0), (0, 0, 0, 0, 0, -1)):
        with pytest.raises(ValueError, match="geotransform"):
            CZ.zone_edges([[px]], bad)
    lim = float(2 ** 21)
    assert CZ.zone_edges([[ZO.ring((-lim, 0), (lim, 1), (0, lim))]]).edges.max() == 2 ** 29
    for bad in (ZO.ring((0, 0), (lim + 1 / 256, 1), (0, 5)), ZO.ring((0, -lim - 1), (1, 1), (0, 5)), ZO.ring((0, 0), (np.nan, 1), (0, 5)),
                ZO.ring((0, 0), (np.inf, 1), (0, 5))):
        with pytest.raises(ValueError, match="zone_edges"):
            CZ.zone_edges([[bad]])
    with pytest.raises(ValueError, match=r"\(n, 2\)"):
        CZ.zone_edges([[np.zeros((4, 3))]])


# ---- zone_items -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("item_pixels", [1, 64, 1000, 65536, 2 ** 40])
def test_zone_items_cover_every_row_once_and_stay_inside(item_pixels):
    polys = list(ZO.rule_zones().values()) + list(ZO.clip_zones().values()) + ZO.fan()
    z = CZ.zone_edges(polys)
    items, off = CZ.zone_items(z, H0, W0, item_pixels)
    assert items.dtype == np.int32 and off.dtype == np.int32 and off[0] == 0 and off[-1] == len(items) and len(off) == len(polys) + 1
    assert (items[:, 1] >= 0).all() and (items[:, 2] >= 0).all() and (items[:, 3] > 0).all() and (items[:, 4] > 0).all()
    assert (items[:, 1] + items[:, 3] <= W0).all() and (items[:, 2] + items[:, 4] <= H0).all()
    names = list(ZO.rule_zones()) + list(ZO.clip_zones())
    for k, zone in enumerate(polys):
        mine = items[off[k]:off[k + 1]]
        assert (mine[:, 0] == k).all()
        m = ZO.zone_mask(ZO.zone_edge_list(zone), H0, W0)
        covered = np.zeros((H0, W0), dtype=np.int64)
        for _, x, y, w, h in mine.tolist():
            covered[y:y + h, x:x + w] += 1
        assert covered.max(initial=0) <= 1 and (covered[m] == 1).all(), k                     # every pixel of the zone in exactly one item
        xmin, ymin, xmax, ymax = z.bbox[k].tolist()
        rows = [y for y in range(H0) if ymin <= 256 * y + 128 < ymax] if z.edge_off[k + 1] > z.edge_off[k] else []
        cols = range(max(xmin // 256, 0), min(-(-xmax // 256), W0))
        assert covered.sum() == len(rows) * len(cols) and all(covered[y, x] == 1 for y in rows for x in cols), k
        if k < len(names) and (names[k].startswith("wholly") or names[k] in ("empty", "degenerate ring only")):
            assert len(mine) == 0, names[k]
        if item_pixels == 1:
            assert (mine[:, 4] == 1).all()
        if item_pixels == 2 ** 40:
            assert len(mine) <= 1
    if item_pixels == 1000:
        k = names.index("everything")
        sizes = items[off[k]:off[k + 1], 3] * items[off[k]:off[k + 1], 4]
        assert len(sizes) == 10 and sizes.min() == 7 * W0 and sizes.max() == 7 * W0                # 70 rows in bands of 1000 // 131 = 7
    with pytest.raises(ValueError, match="zone_items"):
        CZ.zone_items(z, H0, W0, 0)
    with pytest.raises(TypeError, match="zone_items"):
        CZ.zone_items(polys, H0, W0)


# ---- the partition property -------------------------------------------------------------------------------------------------------------------
def test_a_fan_of_triangles_partitions_the_raster():
    v, m = raster(np.uint16, H0, W0, 2), raster(np.uint8, H0, W0, 3, zeros=0.3)
    zm = ZO.masks(ZO.fan(), H0, W0)
    assert len(zm) == 8 and all(a.any() for a in zm) and np.array_equal(sum(a.astype(np.int64) for a in zm), np.ones((H0, W0), dtype=np.int64))
    s = ZO.zone_sums(v, ZO.fan(), m)
    whole = SO.window_sums(v, [(0, 0, W0, H0)], m)[0]
    assert s[:, 0].sum() == H0 * W0 and np.array_equal(s[:, :4].sum(axis=0), whole[:4]) and s[:, 4].max() == whole[4] and whole[1] > 0
    h = ZO.zone_hist(v, ZO.fan(), 10, 256, m)
    assert np.array_equal(h.sum(axis=0), SO.value_hist(v, 10, 256, m))


# ---- the comparison is not blind --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["closed", "ge", "corner"])
def test_a_mistaken_rule_changes_the_gpu_tests_zones(rule):
    polys = {**ZO.rule_zones(), **ZO.clip_zones()}
    v = (1 + np.arange(H0 * W0) * 7 % 65521).astype(np.uint16).reshape(H0, W0)      # (a shifted zone of the same size shows in the sums)
    right, wrong = ZO.zone_sums(v, list(polys.values())), ZO.zone_sums(v, list(polys.values()), rule=rule)
    changed = [name for name, a, b in zip(polys, right, wrong) if not np.array_equal(a, b)]
    assert changed, rule
    assert "rectangle on centres" in changed and "diamond through centres" in changed, changed
    fan_right, fan_wrong = ZO.zone_sums(v, ZO.fan()), ZO.zone_sums(v, ZO.fan(), rule=rule)
    assert not np.array_equal(fan_right, fan_wrong), rule


# ---- the host numbers ---------------------------------------------------------------------------------------------------------------------------
def test_zone_heights_numbers_from_hand_made_sums():
    from srbh_amd.city_summary import heights_from_sums
    sums = np.array([[10, 4, 10, 30, 4], [7, 0, 0, 0, 0], [0, 0, 0, 0, 0], [3, 3, 3 * 65535, 3 * 65535 ** 2, 65535]], dtype=np.int64)
    t, ref = heights_from_sums(sums), SO.heights(sums)
    assert t["n"].tolist() == [4, 0, 0, 3] and t["count"].tolist() == [10, 7, 0, 3] and t["max"].tolist() == [4, 0, 0, 65535]
    assert t["mean"][0] == 2.5 and t["std"][0] == np.sqrt(1.25) and t["fraction"][0] == 0.4 and t["std"][3] == 0.0
    assert np.isnan(t["mean"][1:3]).all() and t["fraction"][1] == 0 and np.isnan(t["fraction"][2])
    for k in ref:
        assert SO.same_bits(t[k], ref[k]) if t[k].dtype == np.float64 else np.array_equal(t[k], ref[k]), k


def test_python_layer_refusals_need_no_device():
    z = CZ.zone_edges([[ZO.rect(1, 1, 5, 5)]])
    v, m = torch.zeros((8, 9), dtype=torch.uint8), torch.zeros((8, 9), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU"):
        CZ.zone_sums(v, z)
    with pytest.raises(RuntimeError, match="no CPU"):
        CZ.zone_histogram(v, z, 10, 7, m)
    with pytest.raises(TypeError, match="zone_sums"):
        CZ.zone_sums(v.to(torch.int16), z)
    with pytest.raises(TypeError, match="zone_sums"):
        CZ.zone_sums(v, [[ZO.rect(1, 1, 5, 5)]])
    with pytest.raises(ValueError, match="zone_sums"):
        CZ.zone_sums(v, CZ.zone_edges([]))
    with pytest.raises(ValueError, match="zone_sums"):
        CZ.zone_sums(v, z, torch.zeros((8, 8), dtype=torch.uint8))
    with pytest.raises(ValueError, match="threshold"):
        CZ.zone_sums(v, z, value_threshold=65536)
    with pytest.raises(ValueError, match="item_pixels"):
        CZ.zone_sums(v, z, item_pixels=0)
    for kw in (dict(bin_width=0), dict(bin_width=65536), dict(nbins=0), dict(nbins=4097), dict(nbins=2.0)):
        with pytest.raises(ValueError, match="zone_histogram"):
            CZ.zone_histogram(v, z, **kw)
    import srbh_amd.city_zones as mod                                   # the alias package resolves the new module
    assert mod.zone_sums is CZ.zone_sums and set(mod.__all__) >= {"zone_edges", "zone_items", "zone_sums", "zone_histogram", "zone_heights",
                                                                   "zonal_fields", "urban_centre_table"}
