"""GPU: footprints burned into a raster (srbh_burn; city_burn.burn / label_raster / zone_raster) against the oracle
tests/city_burn_oracle.py, which tests/test_city_burn_cpu.py pins against a Fraction crossing count, shows not to be blind to six mistaken
rules on the very inputs used here, and shows to hold the cases they are there for (pixels three features deep, a later 0 over an earlier
non-zero, features across every tile seam).

Every pixel is compared EXACTLY.  The rasters are 131 x 70 -- two tile rows with a ragged 6, three tile columns with a ragged 3 -- and lie
in guard buffers of the type's LARGEST value: contiguous with a 16-byte-aligned base (the vector-store path wherever a lane's run is
aligned) and as interior views with three strides and unaligned bases (the element path); a store that left the raster shows as a broken
guard, not as a fault.  Hostile device tables are bounded by the kernel's checks by construction: nothing here provokes anything."""
import numpy as np
import pytest
import torch

from srbh_amd import _lib
from srbh_amd import city_burn as CB
from srbh_amd import city_compare as CC
from srbh_amd import city_summary as CS
from srbh_amd import city_zones as CZ
from srbh_amd.metrics import HeightMetric
from tests import city_burn_oracle as BO
from tests import city_compare_oracle as CO
from tests import city_zones_oracle as ZO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, U16, I16, U8 = 0, 1, 2, 3                           # include/srbh.h SRBH_GRID_*
H0, W0 = BO.H0, BO.W0
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
ERR_ARG = -1
TYPES = [np.uint16, np.uint8]
HOWS = ["aligned", 0, 1, 2]
BO_TORCH = {np.uint16: torch.uint16, np.uint8: torch.uint8}
MARGINS = [(1, 3, 1, 2), (2, 5, 3, 1), (1, 1, 0, 8)]     # top, left, bottom, right of the interior views: three strides, odd bases


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).to(DEV).view(torch.uint16)
    return torch.from_numpy(a).to(DEV)


def host(t):
    t = t.contiguous()
    if t.dtype == torch.uint16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


class Frame:
    """an H x W raster inside a device buffer whose every other element is the type's largest value; the raster itself starts out as
    ``base``, or as that value too"""

    def __init__(self, dtype, H, W, how, base=None):
        self.top, self.shape = np.iinfo(dtype).max, (H, W)
        if how == "aligned":
            pad = 64
            buf = np.full(pad + H * W + pad, self.top, dtype=dtype)
            self.inner = np.zeros(buf.shape, dtype=bool)
            self.inner[pad:pad + H * W] = True
            if base is not None:
                buf[pad:pad + H * W] = base.reshape(-1)
            self.buf = dev(buf)
            self.view = self.buf[pad:pad + H * W].view(H, W)
            assert self.view.is_contiguous() and self.view.data_ptr() % 16 == 0
        else:
            t, l, b, r = MARGINS[how]
            buf = np.full((H + t + b, W + l + r), self.top, dtype=dtype)
            self.inner = np.zeros(buf.shape, dtype=bool)
            self.inner[t:t + H, l:l + W] = True
            if base is not None:
                buf[t:t + H, l:l + W] = base
            self.buf = dev(buf)
            self.view = self.buf[t:t + H, l:l + W]
            assert self.view.stride(0) == W + l + r and (H == 1 or not self.view.is_contiguous())

    def read(self):
        """-> the raster; the guard must be intact"""
        a = host(self.buf)
        assert (a[~self.inner] == self.top).all(), "a store left the raster"
        return a[self.inner].reshape(self.shape)


def burn_into(zones, values, dtype, how, H=H0, W=W0, base=None, **kw):
    fr = Frame(dtype, H, W, how, base)
    got = CB.burn(zones, values, out=fr.view, **kw)
    assert got.data_ptr() == fr.view.data_ptr() and got.dtype == fr.view.dtype and tuple(got.shape) == (H, W)
    return fr.read()


@pytest.fixture(scope="module")
def ref():
    """name -> (zones, masks, {dtype: values}) of the oracle module's cases, computed once and left unchanged"""
    per = {t: BO.cases(t) for t in TYPES}
    return {name: (CZ.zone_edges(polys), BO.feature_masks(polys, H0, W0), {t: per[t][name][1] for t in TYPES})
            for name, (polys, _) in per[np.uint16].items()}


# ---- alignment and ragged edges ----------------------------------------------------------------------------------------------------------------
def edge_rects(H, W):
    """xoff 0..17 x widths 1..40 x 1, 3 and H rows; the same flush with the right edge"""
    out = []
    for xoff in range(18):
        for i, w in enumerate(range(1 + xoff % 3, 41, 3)):
            for h, y in ((1, (xoff * 7 + w) % H), (3, (xoff * 5 + w) % (H - 2)), (H, 0)):
                out.append((xoff, y, w, h))
                out.append((W - w - (xoff + i) % 3, y, w, h))
    return out


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("how", HOWS)
def test_integer_rectangles_equal_slice_assignments(dtype, how):
    """each rectangle is one feature; in feature order, "last" is a sequence of slice assignments"""
    rects = edge_rects(H0, W0)
    assert {r[0] for r in rects} >= set(range(18)) and {r[2] for r in rects} >= set(range(1, 41)) and {r[3] for r in rects} == {1, 3, H0}
    top = int(np.iinfo(dtype).max)
    values = [(i * 37 + 1) % (top + 1) for i in range(len(rects))]
    zones = CZ.zone_edges([[ZO.rect(x, y, x + w, y + h)] for x, y, w, h in rects])
    want = np.full((H0, W0), 7, dtype=dtype)
    for (x, y, w, h), v in zip(rects, values):
        want[y:y + h, x:x + w] = v
    assert np.array_equal(burn_into(zones, values, dtype, how, init=7), want)
    for k in (0, 5, 400, len(rects) - 1, len(rects) - 2):                  # alone: Z = 1
        x, y, w, h = rects[k]
        one = np.full((H0, W0), 0, dtype=dtype)
        one[y:y + h, x:x + w] = values[k]
        assert np.array_equal(burn_into(CZ.zone_edges([[ZO.rect(x, y, x + w, y + h)]]), [values[k]], dtype, how), one), k


# ---- rules, ordering, merge, init ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("merge", ["last", "max"])
def test_every_case_equals_the_oracle(ref, dtype, how, merge):
    init = 7 if merge == "last" else int(np.iinfo(dtype).max)
    got = {}
    for name, (zones, masks, values) in ref.items():
        want = BO.paint(masks, values[dtype], H0, W0, dtype, init, merge)
        got[name] = burn_into(zones, values[dtype], dtype, how, init=init, merge=merge)
        bad = np.argwhere(got[name] != want)
        assert len(bad) == 0, (name, len(bad), bad[:5].tolist())
    assert not np.array_equal(got["rule"], got["rule reversed"]) or merge == "max"
    if merge == "max":
        assert np.array_equal(got["rule"], got["rule reversed"])              # independent of the order
    assert (got["fan"] != init).all() or init in ref["fan"][2][dtype]


@pytest.mark.parametrize("dtype", TYPES)
def test_last_equals_max_on_disjoint_features_and_zone_raster(ref, dtype):
    zones, masks, values = ref["fan"]
    a, b = CB.burn(zones, values[dtype], H0, W0, dtype=BO_TORCH[dtype]), CB.burn(zones, values[dtype], H0, W0, dtype=BO_TORCH[dtype], merge="max")
    assert a.is_cuda and a.dtype == BO_TORCH[dtype] and tuple(a.shape) == (H0, W0) and torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert np.array_equal(host(a), BO.paint(masks, values[dtype], H0, W0, dtype))
    ids = CB.zone_raster(zones, H0, W0)
    assert ids.dtype == torch.uint16 and np.array_equal(host(ids), BO.paint(masks, range(1, 9), H0, W0, np.uint16))
    assert (host(ids) != 0).all()
    hist = CS.value_histogram(ids, 1, 16).cpu().numpy()
    count = CZ.zone_sums(ids, zones).cpu().numpy()[:, 0]
    assert np.array_equal(hist[1:9], count) and hist[0] == 0 and hist[9:].sum() == 0 and count.sum() == H0 * W0


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("how", HOWS)
def test_keep_over_a_prefilled_raster(ref, dtype, how):
    rs = np.random.RandomState(31)
    base = rs.randint(0, int(np.iinfo(dtype).max) + 1, size=(H0, W0)).astype(dtype)
    for name in ("rule", "clip", "small", "one", "empty features", "seams"):
        zones, masks, values = ref[name]
        for merge in ("last", "max"):
            want = BO.paint(masks, values[dtype], H0, W0, dtype, 5, merge, base)
            got = burn_into(zones, values[dtype], dtype, how, base=base, keep=True, merge=merge, init=5)
            assert np.array_equal(got, want), (name, merge)
        none = BO.cover(masks) == 0
        assert name == "clip" or (none.any() and np.array_equal(want[none], base[none]))
    # features wholly outside: NF = 0, every tile is empty -- init everywhere, or nothing under keep
    polys = [ZO.clip_zones()[k] for k in ("wholly left", "wholly below", "wholly right")]
    zones = CZ.zone_edges(polys)
    assert len(CB.burn_tiles(zones, H0, W0)[2]) == 0 and len(zones.edges) > 0
    assert np.array_equal(burn_into(zones, [1, 2, 3], dtype, how, base=base, keep=True), base)
    assert (burn_into(zones, [1, 2, 3], dtype, how, base=base, init=9) == 9).all()
    # no feature has an edge: nothing is launched
    nothing = CZ.zone_edges([[], [ZO.ring((5, 5), (9, 9))]])
    assert (burn_into(nothing, [1, 2], dtype, how, base=base, init=4) == 4).all()
    assert np.array_equal(burn_into(nothing, [1, 2], dtype, how, base=base, keep=True), base)


# ---- extreme shapes -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,dtype,how", [(3, 70000, np.uint16, "aligned"), (3, 70000, np.uint8, 1), (5000, 3, np.uint16, 0),
                                           (5000, 3, np.uint8, "aligned")])
def test_long_and_tall_rasters(H, W, dtype, how):
    """3 x 70000: 1094 tile columns, every row 16-byte aligned; 5000 x 3: 79 tile rows of one ragged column"""
    if W > H:
        polys = [[ZO.ring((-5, -1), (W + 10, 0.2), (W - 9.5, H + 0.5), (W / 2 + 0.25, H / 2), (10, H - 0.1))],
                 [ZO.rect(8191.5, 0, 8192.5, H), ZO.ring((100.5, 0.5), (W - 100.5, 0.5), (W / 3, H - 0.5))],
                 [ZO.rect(63.5, 1, 64.5, 2)], [ZO.rect(W - 70.5, 0, W - 0.5, 2)], [ZO.rect(30000, 1, 30100, 3)]]
    else:
        polys = [[ZO.ring((-1, -5), (0.2, H + 10), (W + 0.5, H - 9.5), (W / 2, H / 2 + 0.25), (W - 0.1, 10))],
                 [ZO.ring((0.5, 100.5), (2.5, 2047.5), (0.5, H - 100.5))], [ZO.rect(1, 63.5, 2, 64.5)], [ZO.rect(0, H - 70.5, 2, H - 0.5)],
                 [ZO.rect(1, 3000, 3, 3100)]]
    values = [300 % 256, 0, 255, 17, 1]
    masks = BO.feature_masks(polys, H, W)
    assert all(m.any() for m in masks) and (BO.cover(masks) == 0).any() and (BO.cover(masks) >= 2).any()
    zones = CZ.zone_edges(polys)
    for merge in ("last", "max"):
        assert np.array_equal(burn_into(zones, values, dtype, how, H, W, init=9, merge=merge), BO.paint(masks, values, H, W, dtype, 9, merge)), merge


@pytest.mark.parametrize("how", ["aligned", 1])
def test_columns_from_2_to_the_21_never_burn(how):
    """a raster 148 columns wider than the fixed-point range: features reach X = 2^29 exactly; the oracle judges the first and the last
    400 columns, everything between is the value of the rectangle that spans the range"""
    big, H, W, n = float(2 ** 21), 3, 2 ** 21 + 148, 400
    polys = [[ZO.rect(0, 0, big, 3)], [ZO.ring((big - 200, 0), (big, 1.5), (big - 200, 3))],
             [ZO.rect(big - 50.5, 0, big, 2)], [ZO.rect(2.5, 0, 9.5, 3)], [ZO.rect(big - 9, 1, big, 3), ZO.rect(big - 4, 1, big, 3)]]
    values = [3, 200, 0, 77, 255]
    zones = CZ.zone_edges(polys)
    assert zones.edges.max() == 2 ** 29 and -(-W // 64) == 32771
    fr = Frame(np.uint8, H, W, how)
    CB.burn(zones, values, out=fr.view, init=9)
    got = fr.read()
    first = BO.burn(polys, values, H, n, np.uint8, 9)
    last = BO.burn(BO.shifted(polys, W - n), values, H, n, np.uint8, 9)
    assert np.array_equal(got[:, :n], first) and np.array_equal(got[:, W - n:], last)
    assert (got[:, n:W - n] == 3).all() and (last[:, n - 148:] == 9).all() and (last[:, :n - 148] != 9).all() and len(np.unique(last)) >= 4
    assert (got[:, 2 ** 21:] == 9).all() and (got[:, 2 ** 21 - 1] != 9).all()


# ---- hostile tables and refusals --------------------------------------------------------------------------------------------------------------------
def type_code(t):
    return U16 if t.dtype == torch.uint16 else U8


class Tables:
    """device tables for the C ABI, each in a buffer of its own (edges 16-byte aligned)"""
    NAMES = ("edges", "edge_off", "values", "boxes", "tile_off", "tile_feat")

    def __init__(self, zones, values, H, W, **change):
        boxes, tile_off, tile_feat = CB.burn_tiles(zones, H, W)
        a = dict(edges=zones.edges, edge_off=zones.edge_off, values=values, boxes=boxes, tile_off=tile_off, tile_feat=tile_feat)
        a.update(change)
        self.np = {k: np.ascontiguousarray(np.asarray(v, dtype=np.int64).astype(np.int32)) for k, v in a.items()}
        self.t = {k: torch.from_numpy(np.concatenate([v.reshape(-1), np.zeros(4, np.int32)])).to(DEV) for k, v in self.np.items()}
        self.Z, self.E = len(self.np["edge_off"]) - 1, len(self.np["edges"])
        self.NT, self.NF = len(self.np["tile_off"]) - 1, len(self.np["tile_feat"])

    def call(self, out, H, W, merge=0, keep=0, init=0, **k):
        p = {n: self.t[n].data_ptr() for n in self.NAMES}
        p.update({n: k[n] for n in self.NAMES if n in k})
        return _lib.lib().srbh_burn((k["out_ptr"] if "out_ptr" in k else out.data_ptr()), k.get("type", type_code(out)), k.get("rs", out.stride(0)), H, W, p["edges"],
                                    p["edge_off"], p["values"], p["boxes"], k.get("Z", self.Z), k.get("E", self.E), p["tile_off"],
                                    p["tile_feat"], k.get("NT", self.NT), k.get("NF", self.NF), merge, keep, init, _lib.stream_ptr())


@pytest.mark.parametrize("dtype,how", [(np.uint16, 0), (np.uint8, "aligned"), (np.uint16, "aligned"), (np.uint8, 2)])
def test_hostile_device_tables_stay_inside(dtype, how):
    """wrong tables may give wrong pixels in the tiles and of the features they name; they reach nothing outside the tables and out"""
    polys = list(ZO.rule_zones().values()) + BO.seam_zones()
    Z = len(polys)
    values = BO.values_for(Z, dtype, 41)
    z = CZ.zone_edges(polys)
    masks = BO.feature_masks(polys, H0, W0)
    boxes, tile_off, tile_feat = CB.burn_tiles(z, H0, W0)
    NT, NF, E = len(tile_off) - 1, len(tile_feat), len(z.edges)
    assert NT == 6 and (np.diff(tile_off) > 2).all()
    big = 2 ** 30

    def run(tab, **kw):
        fr = Frame(dtype, H0, W0, how)
        _lib.check(tab.call(fr.view, H0, W0, init=7, **kw), "srbh_burn")
        return fr.read()

    # (a) hostility that changes nothing: feature indices -1 / Z / INT_MAX / INT_MIN in every tile's list, edges beyond the coordinate
    # limit inside feature 0, an absurdly large box
    lists = [tile_feat[tile_off[t]:tile_off[t + 1]].tolist() for t in range(NT)]
    hostile = [[-1] + l[:1] + [Z, INT_MAX] + l[1:] + [INT_MIN, Z + 1] for l in lists]
    off_a = np.concatenate([[0], np.cumsum([len(l) for l in hostile])])
    e0 = z.edge_off[1]
    edges_a = np.concatenate([z.edges[:e0], [[-big, -big, big, big], [5, INT_MAX, 9, INT_MIN]], z.edges[e0:]])
    edge_off_a = z.edge_off.astype(np.int64).copy()
    edge_off_a[1:] += 2
    boxes_a = boxes.copy()
    boxes_a[10] = (INT_MIN, INT_MIN, INT_MAX, INT_MAX)
    tab = Tables(z, values, H0, W0, edges=edges_a, edge_off=edge_off_a, boxes=boxes_a, tile_off=off_a, tile_feat=np.concatenate(hostile))
    want = BO.paint(masks, values, H0, W0, dtype, 7)
    assert np.array_equal(run(tab), want)
    assert np.array_equal(run(tab, merge=1), BO.paint(masks, values, H0, W0, dtype, 7, "max"))
    # (b) features 2 and 3 lose their edges to a range beyond E, 5 and 6 to one below 0, 10 to a box no rectangle meets
    edge_off_b = z.edge_off.astype(np.int64).copy()
    edge_off_b[3], edge_off_b[6] = E + 1000, -7
    boxes_b = boxes.copy()
    boxes_b[10] = (INT_MAX, INT_MAX, INT_MIN, INT_MIN)
    gone = (2, 3, 5, 6, 10)
    tab = Tables(z, values, H0, W0, edge_off=edge_off_b, boxes=boxes_b)
    some = [np.zeros_like(m) if f in gone else m for f, m in enumerate(masks)]
    assert all(masks[f].any() for f in gone)
    assert np.array_equal(run(tab), BO.paint(some, values, H0, W0, dtype, 7))
    # (c) tile 1's range descends, tile 5's ends beyond NF: both are empty; tile 2 then starts inside tile 1's list (unsound: any pixels,
    # inside the raster); tiles 0, 3 and 4 are sound and at their oracle values
    off_c = tile_off.astype(np.int64).copy()
    off_c[2], off_c[6] = off_c[1] - 1, NF + 5
    tab = Tables(z, values, H0, W0, tile_off=off_c)
    got = run(tab)
    assert np.array_equal(got[:64, :64], want[:64, :64]) and np.array_equal(got[64:, :128], want[64:, :128])
    assert (got[:64, 64:128] == 7).all() and (got[64:, 128:] == 7).all() and (want[:64, 64:128] != 7).any() and (want[64:, 128:] != 7).any()
    # the sound tables next to them are unchanged by all this
    assert np.array_equal(run(Tables(z, values, H0, W0)), want)


def test_two_calls_are_bit_equal_and_build_the_tables_once(ref):
    zones, masks, values = ref["small"]
    zones._device_tables.clear()
    a = CB.burn(zones, values[np.uint16], H0, W0)
    torch.cuda.synchronize()
    key = [k for k in zones._device_tables if k[0] == "burn"]
    buf = zones._device_tables[key[0]][0]
    b = CB.burn(zones, values[np.uint16], H0, W0)
    assert len(key) == 1 and [k for k in zones._device_tables if k[0] == "burn"] == key and zones._device_tables[key[0]][0] is buf
    assert a.data_ptr() != b.data_ptr() and np.array_equal(host(a), host(b)) and np.array_equal(host(a), BO.paint(masks, values[np.uint16], H0, W0, np.uint16))
    c = CB.burn(zones, values[np.uint8], H0, W0, dtype=torch.uint8)       # the type is not part of the tables
    assert len(zones._device_tables) == 1 and np.array_equal(host(c), BO.paint(masks, values[np.uint8], H0, W0, np.uint8))
    CZ.zone_sums(a, zones)                                                # zone_sums' tables live next to them
    assert len(zones._device_tables) == 2


def test_c_abi_refusals_write_nothing(ref):
    zones, masks, values = ref["rule"]
    tab = Tables(zones, values[np.uint16], H0, W0)
    nan = torch.full((H0 * W0 * 2 // 8 + 2,), float("nan"), dtype=torch.float64, device=DEV)
    out = nan.view(torch.uint16)[:H0 * W0].view(H0, W0)
    p = {n: tab.t[n].data_ptr() for n in Tables.NAMES}
    refused = [dict(out_ptr=None), *[{n: None} for n in Tables.NAMES], dict(type=I16), dict(type=F32), dict(type=4), dict(type=-1), dict(H=0), dict(W=0),
               dict(H=-3), dict(Z=0), dict(Z=-1), dict(E=0), dict(E=-5), dict(NF=-1), dict(H=2 ** 16, W=2 ** 15, rs=2 ** 15, NT=2 ** 19),
               dict(rs=W0 - 1), dict(out_ptr=out.data_ptr() + 1), dict(edges=p["edges"] + 4), dict(edge_off=p["edge_off"] + 2),
               dict(tile_feat=p["tile_feat"] + 1), dict(NT=tab.NT + 1), dict(NT=tab.NT - 1), dict(NT=0), dict(H=H0 + 64), dict(merge=-1),
               dict(merge=2), dict(init=-1), dict(init=65536), dict(type=U8, init=256)]
    for change in refused:
        kw = {k: v for k, v in change.items() if k not in ("H", "W", "merge", "init")}
        rc = tab.call(out, change.get("H", H0), change.get("W", W0), change.get("merge", 0), 0, change.get("init", 0), **kw)
        assert rc == ERR_ARG, change
        with pytest.raises(RuntimeError, match="srbh_burn"):
            _lib.check(rc, "srbh_burn")
    torch.cuda.synchronize()
    assert torch.isnan(nan).all()                                         # nothing was launched: the pattern stands
    assert tab.call(out, H0, W0, 0, 0, 65535) == 0 and tab.call(out, H0, W0, 1, 1, 0, NF=0) == 0        # NF = 0 is legal
    assert np.array_equal(host(out), BO.paint(masks, values[np.uint16], H0, W0, np.uint16, 65535)) and torch.isnan(nan[H0 * W0 * 2 // 8 + 1:]).all()
    assert _lib.lib().srbh_burn_tile() == CB.TILE == 64


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------
def test_label_raster_feeds_city_validation():
    rs = np.random.RandomState(16)
    H, W, n = 150, 200, 260
    gt = (431000.0, 2.5, 0.0, 4581000.0, 0.0, -2.5)
    rings, pix = [], []
    for i in range(n):                                                   # footprints: quadrilaterals of 3..14 pixels, some with a courtyard
        c = np.array([rs.uniform(0, W), rs.uniform(0, H)])
        half = rs.uniform(1.5, 7, size=2)
        quad = c + np.array([(-1, -1), (1, -1), (1, 1), (-1, 1)]) * half + rs.uniform(-1, 1, size=(4, 2))
        mine = [np.round(quad * 256) / 256] + ([c + np.array([(-1, -1), (1, -1), (1, 1), (-1, 1)]) * 0.4 * half] if i % 7 == 0 else [])
        pix.append(mine)
        rings.append([np.stack([gt[0] + r[:, 0] * gt[1], gt[3] + r[:, 1] * gt[5]], axis=1) for r in mine])
    pix = [[(np.asarray(r) - (gt[0], gt[3])) / (gt[1], gt[5]) for r in z] for z in rings]          # the pixels the geotransform gives back
    heights = np.round(rs.gamma(2.0, 6.0, size=n) * 20) / 20                                  # multiples of 0.05: ties of the rounding
    heights[-4:] = (0.05, 0.15, 0.0, 7000.0)                                                  # (the last feature is never painted over)
    flat_v = np.concatenate([r for z in rings for r in z])
    ring_off = np.concatenate([[0], np.cumsum([len(r) for z in rings for r in z])])
    feature_off = np.concatenate([[0], np.cumsum([len(z) for z in rings])])
    zones = CB.feature_edges(flat_v, ring_off, feature_off, gt)
    burned = CB.label_raster(zones, heights, H, W)
    ref = BO.burn(pix, [min(65535, int(round(10.0 * float(h)))) for h in heights], H, W, np.uint16)
    assert burned.dtype == torch.uint16 and np.array_equal(host(burned), ref) and 0.2 < (ref > 0).mean() < 0.9 and ref.max() == 65535
    height = np.clip(ref.astype(np.int32) + rs.randint(-40, 41, size=(H, W)), 0, 65535).astype(np.uint16)
    height[(ref == 0) & (rs.rand(H, W) < 0.9)] = 0
    build = CO.class_of(height, CC.DEFAULT_EDGES).astype(np.uint8)
    got = CC.city_validation(dev(height), burned, dev(build))
    rows, bad = CO.class_sums(height, ref, CC.DEFAULT_EDGES, build)
    stats, count, cm = CO.metric_tables(rows)
    assert got["bad"] == bad == 0
    hm = HeightMetric(7, device=DEV)
    hm.stats += torch.from_numpy(stats).to(DEV)
    hm.count += torch.from_numpy(count).to(DEV)
    assert torch.equal(got["height"].getAvgEach(), hm.getAvgEach()) and torch.equal(got["height"].getCount(), hm.getCount())
    assert CO.same_bits(got["height"].stats.cpu().numpy(), stats) and (stats[:, 0] > 0).sum() >= 4
    assert np.array_equal(got["seg"].getConfusionMatrix().cpu().numpy(), cm) and cm.sum() == H * W
    whole = CO.errors(CO.pair_sums(height, ref, [(0, 0, W, H)], None, "any", -1, -1))
    for k, v in whole.items():
        assert CO.same_bits(got["sums"][k].astype(np.float64), v.astype(np.float64)), k
