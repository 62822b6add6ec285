"""GPU: the urban-centre validation (srbh_zone_pair_sums; city_zone_compare.zone_pair_sums / zone_errors / urban_centre_validation)
against the oracle tests/city_zone_compare_oracle.py, which tests/test_city_zone_compare_cpu.py pins against a pixel loop and shows not
to be blind to five mistaken rules on the very inputs used here.

Every number the kernel returns is an integer and is compared EXACTLY; the floats of the host layer bit for bit.  The rasters are 131 x
70 interior views of larger buffers whose every other element is the LARGEST value, with strided rows, unaligned bases and three
different strides (a load or a predicate that left a raster shows as a wrong sum, not as a fault).  The shapes are the smallest at which
each piece can go wrong: the twelve element-size forms, every alignment of a rectangle's head and tail, scanlines through vertices,
holes and overlapping parts, zones partly and wholly outside, vertices at the fixed-point limit, more than 256 edges, rows wider than one
bitmap segment, bands of more rows than one batch, sums beyond 32 bits of either sign, hostile device tables."""
import numpy as np
import pytest
import torch

from srbh_amd import _lib
from srbh_amd import city_compare as CC
from srbh_amd import city_zone_compare as CZC
from srbh_amd import city_zones as CZ
from tests import city_compare_oracle as CO
from tests import city_zone_compare_oracle as ZCO
from tests import city_zones_oracle as ZO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U16, I16, U8, F32 = 1, 2, 3, 0                          # include/srbh.h SRBH_GRID_*
H0, W0 = ZCO.H0, ZCO.W0
INT_MAX = 2 ** 31 - 1
GARBAGE = -0x0123456789abcdef
ERR_ARG = -1
SIZES = [(tp, tr, tm) for tp in (np.uint16, np.uint8) for tr in (np.uint16, np.uint8) for tm in (None, np.uint8, np.uint16)]
NAMES, POLYS = ZCO.NAMES, ZCO.POLYS


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).to(DEV).view(torch.uint16)
    return torch.from_numpy(a).to(DEV)


def framed(a, top=1, left=3, bottom=1, right=2):
    """`a` as an interior view of a larger device buffer whose every other element is the type's largest value; the view starts at an
    odd element of the buffer"""
    H, W = a.shape
    buf = np.full((H + top + bottom, W + left + right), np.iinfo(a.dtype).max, dtype=a.dtype)
    buf[top:top + H, left:left + W] = a
    return dev(buf)[top:top + H, left:left + W]


def framed3(p, r, m):
    """the three rasters framed with three different row strides"""
    fp, fr, fm = framed(p), framed(r, 2, 5, 3, 1), None if m is None else framed(m, 1, 1, 2, 9)
    assert not fp.is_contiguous() and fp.stride(0) != fr.stride(0) and (fm is None or len({fp.stride(0), fr.stride(0), fm.stride(0)}) == 3)
    return fp, fr, fm


def sums(*a, **k):
    got = CZC.zone_pair_sums(*a, **k)
    assert got.dtype == torch.int64 and got.is_cuda and got.shape[1] == 10
    return got.cpu().numpy()


@pytest.fixture(scope="module")
def ref():
    """the zones of the rule, even-odd, clipping and partition rows and their masks, computed once"""
    return CZ.zone_edges(POLYS), ZO.masks(POLYS, H0, W0)


class Tables:
    """device tables for the C ABI, edges in a buffer of their own (16-byte aligned)"""

    def __init__(self, edges, edge_off, items, item_off):
        self.np = [np.ascontiguousarray(a, dtype=np.int32) for a in (edges, edge_off, items, item_off)]
        self.t = [torch.from_numpy(a.reshape(-1)).to(DEV) for a in self.np]
        self.Z, self.E, self.NI = len(edge_off) - 1, len(edges), len(items)

    def args(self, **k):
        p = [t.data_ptr() for t in self.t]
        return (k.get("edges", p[0]), k.get("edge_off", p[1]), k.get("Z", self.Z), k.get("E", self.E), k.get("items", p[2]),
                k.get("item_off", p[3]), k.get("NI", self.NI))


def type_code(t):
    return U16 if t.dtype == torch.uint16 else U8


def raw_sums(p, r, m, tab, out, ws, mode=0, pthr=0, rthr=0, mthr=0):
    H, W = p.shape
    return _lib.lib().srbh_zone_pair_sums(p.data_ptr(), type_code(p), p.stride(0), r.data_ptr(), type_code(r), r.stride(0),
                                          None if m is None else m.data_ptr(), 0 if m is None else type_code(m),
                                          0 if m is None else m.stride(0), H, W, *tab.args(), mode, pthr, rthr, mthr, out.data_ptr(),
                                          ws.data_ptr(), _lib.stream_ptr())


def nan_buffer(nbytes):
    return torch.full((nbytes // 8 + 2,), float("nan"), dtype=torch.float64, device=DEV)


# ---- element sizes, memory layout, the named zones ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tp,tr,tm", SIZES)
def test_named_zones_every_element_size_and_layout(ref, tp, tr, tm):
    zones, masks = ref
    p, r, m = CO.triple(tp, tr, tm)
    want = ZCO.zone_pair_sums(p, r, POLYS, m, masks=masks)
    fp, fr, fm = framed3(p, r, m)
    assert fp.data_ptr() % 16 != 0
    got = sums(fp, fr, zones, fm)
    for k, name in enumerate(NAMES):
        assert np.array_equal(got[k], want[k]), (name, got[k], want[k])
    assert np.array_equal(got, want)
    assert np.array_equal(sums(dev(p), dev(r), zones, None if m is None else dev(m)), want)     # contiguous, aligned bases
    row = dict(zip(NAMES, want.tolist()))
    whole = CO.pair_sums(p, r, [(0, 0, W0, H0)], m)[0].tolist()
    assert row["rectangle on centres"][0] == 30 * 15 and row["1000-gon"][0] > 2700 and row["hole"][0] == 40 * 18 - 16 * 8
    assert row["two overlapping parts"][0] == 15 * 15 + 16 * 15 - 2 * 8 * 8                   # the overlap is outside
    for name in ("empty", "degenerate ring only", "wholly left", "wholly below", "wholly right", "sliver without a centre"):
        assert row[name] == [0] * 10, name
    assert row["sliver with one column"][0] == 57
    assert row["triangle at the limit"] == whole and row["everything"] == whole and row["beyond everything"] == whole
    assert sum(0 < w[1] < w[0] for w in want.tolist()) > 15                                     # partial zones
    # the fan's partition equals the whole raster's pair_sums row, from the device
    dwhole = CC.pair_sums(dev(p), dev(r), [(0, 0, W0, H0)], None if m is None else dev(m)).cpu().numpy()[0]
    assert dwhole.tolist() == whole and np.array_equal(got[len(NAMES):].sum(axis=0), dwhole)


def test_integer_rectangles_equal_pair_sums_of_the_windows():
    p, r, m = CO.triple(np.uint16, np.uint8, np.uint8)
    pos = CO.edge_windows(H0, W0)
    assert set(pos[:, 0].tolist()) >= set(range(18)) and set(pos[:, 2].tolist()) >= set(range(1, 41)) and {1, 3, H0} <= set(pos[:, 3].tolist())
    zones = CZ.zone_edges(ZCO.window_zones(pos))
    fp, fr, fm = framed3(p, r, m)
    for mask, fmask in ((m, fm), (None, None)):
        want = CO.pair_sums(p, r, pos, mask)
        got = CZC.zone_pair_sums(fp, fr, zones, fmask)
        assert tuple(got.shape) == (len(pos), 10) and np.array_equal(got.cpu().numpy(), want)
        assert torch.equal(got, CC.pair_sums(fp, fr, pos, fmask))
    # the other raster fixing the groups: uint8 first
    assert np.array_equal(sums(fr, fp, zones, fm), CO.pair_sums(r, p, pos, m))


def test_small_zones_one_zone_and_empty_zones():
    p, r, m = CO.triple(np.uint16, np.uint16, np.uint8, seed=10)
    fp, fr, fm = framed3(p, r, m)
    small = ZO.small_zones(301)
    want = ZCO.zone_pair_sums(p, r, small, m)
    assert (want[:, 0] == 0).any() and (want[:, 1] > 0).sum() > 200 and ((want[:, 1] == 0) & (want[:, 0] > 0)).any()
    assert np.array_equal(sums(fp, fr, CZ.zone_edges(small), fm), want)
    for k in (0, 150, 300):
        assert np.array_equal(sums(fp, fr, CZ.zone_edges(small[k:k + 1]), fm), want[k:k + 1])
    assert sums(fp, fr, CZ.zone_edges([[], [ZO.rect(-9, -9, -1, -1)]]), fm).tolist() == [[0] * 10] * 2    # nothing to launch: zeros
    mixed = [[], small[7], [ZO.rect(-9, -9, -1, -1)], small[8], []]
    assert np.array_equal(sums(fp, fr, CZ.zone_edges(mixed), fm), ZCO.zone_pair_sums(p, r, mixed, m))


# ---- modes and thresholds -----------------------------------------------------------------------------------------------------------------------
def test_modes_and_thresholds(ref):
    zones, masks = ref
    p, r, m = ZCO.threshold_rasters()
    dp, dr, dm = dev(p), dev(r), dev(m)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    empty = partial = 0
    for mode in CO.MODES:
        for pthr in (-1, 0, 254, 65535):
            for rthr in (-1, 0, 254, 65535):
                want = ZCO.zone_pair_sums(p, r, POLYS, None, mode, pthr, rthr, masks=masks)
                got = sums(dp, dr, zones, mode=mode, pred_threshold=pthr, ref_threshold=rthr, workspace=ws)
                assert np.array_equal(got, want), (mode, pthr, rthr)
                for mthr in (-1, 0, 6, 255):
                    want = ZCO.zone_pair_sums(p, r, POLYS, m, mode, pthr, rthr, mthr, masks=masks)
                    got = sums(dp, dr, zones, dm, mode, pthr, rthr, mthr, workspace=ws)
                    assert np.array_equal(got, want), (mode, pthr, rthr, mthr)
                    big = want[want[:, 0] > 100]
                    empty += int((big[:, 1] == 0).all())
                    partial += int(((big[:, 1] > 0) & (big[:, 1] < big[:, 0])).any())
    assert empty >= 16 and partial >= 16
    everything = sums(dp, dr, zones, dm, "any", -1, -1, -1)
    assert np.array_equal(everything[:, 0], everything[:, 1])


# ---- segments, batches and bands ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(3, 70000), (5000, 3), (5, 1500), (40, 3000)])
def test_rows_wider_than_a_segment_and_bands_taller_than_a_batch(H, W):
    """3 x 70000: nine segments of 8192 columns; 5000 x 3: one item of 5000 one-word rows is three batches; 1500 and 3000 columns: rows of
    47 and 94 words.  However the items are cut, the fold gives the same sums."""
    polys, p, r, m = ZCO.long_case(H, W)
    zones, want = CZ.zone_edges(polys), ZCO.zone_pair_sums(p, r, polys, m)
    assert (want[:2, 0] > 0).all() and (want[:2, 0] < H * W).all() and want[2, 0] == H * W and (want[:, 1] > 0).all()
    fp, fr, fm = framed3(p, r, m)
    counts = set()
    for item_pixels in (64, 1000, 65536, 2 ** 30):
        counts.add(len(CZ.zone_items(zones, H, W, item_pixels)[0]))
        assert np.array_equal(sums(fp, fr, zones, fm, item_pixels=item_pixels), want), item_pixels
    assert len(counts) >= 2 and min(counts) == 3


def test_band_sizes_give_equal_bits(ref):
    zones, masks = ref
    p, r, m = CO.triple(np.uint8, np.uint16, np.uint16, seed=8)
    fp, fr, fm = framed3(p, r, m)
    want = ZCO.zone_pair_sums(p, r, POLYS, m, "both", masks=masks)
    for item_pixels in (1, 64, 1000, 2 ** 30):
        assert np.array_equal(sums(fp, fr, zones, fm, "both", item_pixels=item_pixels), want), item_pixels


# ---- overflow -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pv,rv", [(65535, 0), (0, 65535), (65535, 65535)])
def test_sums_beyond_32_bits_of_either_sign(pv, rv):
    N = 1024
    dp, dr = dev(np.full((N, N), pv, dtype=np.uint16)), dev(np.full((N, N), rv, dtype=np.uint16))
    zones = CZ.zone_edges([[ZO.rect(0, 0, N, N)]])
    n, d = N * N, pv - rv
    want = [n, n, n * d, n * abs(d), n * d * d, n * pv, n * rv, n * pv * pv, n * rv * rv, n * pv * rv]
    assert max(abs(w) for w in want) > 4.5e15 and (d >= 0 or want[2] < -2 ** 32)
    for item_pixels, items in ((2 ** 30, 1), (65536, 16)):
        assert len(CZ.zone_items(zones, N, N, item_pixels)[0]) == items
        assert sums(dp, dr, zones, item_pixels=item_pixels).tolist() == [want], item_pixels


# ---- identities ---------------------------------------------------------------------------------------------------------------------------------
def test_identities(ref):
    zones, masks = ref
    p, r, m = CO.triple(np.uint16, np.uint16, np.uint8, seed=20)
    dp, dr, dm = dev(p), dev(r), dev(m)
    same = sums(dp, dp, zones, dm)
    assert (same[:, 2:5] == 0).all() and np.array_equal(same[:, 5], same[:, 6]) and np.array_equal(same[:, 7], same[:, 9]) and (same[:, 1] > 0).any()
    for mode in ("any", "both"):
        a, b = sums(dp, dr, zones, dm, mode), sums(dr, dp, zones, dm, mode)
        assert np.array_equal(a[:, 2], -b[:, 2]) and (a[:, 2] != 0).any() and np.array_equal(a[:, [0, 1, 3, 4, 9]], b[:, [0, 1, 3, 4, 9]])
        assert np.array_equal(a[:, [5, 7]], b[:, [6, 8]])
    pred = sums(dp, dr, zones, dm, "pred", 0, 0, 0)
    assert np.array_equal(pred[:, [0, 1, 5, 7]], CZ.zone_sums(dp, zones, dm).cpu().numpy()[:, :4])
    fan = sums(dp, dr, zones, dm)[len(NAMES):]
    assert len(fan) == 8 and np.array_equal(fan.sum(axis=0), CC.pair_sums(dp, dr, [(0, 0, W0, H0)], dm).cpu().numpy()[0])


# ---- workspace, outputs, reuse ------------------------------------------------------------------------------------------------------------------
def test_nan_patterned_workspace_and_out_repeat_and_table_reuse(ref):
    _, masks = ref
    zones = CZ.zone_edges(POLYS)                                          # fresh: its table cache is this test's own
    p, r, m = CO.triple(np.uint16, np.uint8, np.uint8, seed=30)
    fp, fr, fm = framed3(p, r, m)
    want = ZCO.zone_pair_sums(p, r, POLYS, m, masks=masks)
    items, item_off = CZ.zone_items(zones, H0, W0, 1000)
    tab = Tables(zones.edges, zones.edge_off, items, item_off)
    need = _lib.lib().srbh_zone_pair_ws_bytes(tab.NI)
    assert need == tab.NI * 80 and tab.NI > tab.Z
    ws, out = nan_buffer(need), nan_buffer(tab.Z * 80)
    _lib.check(raw_sums(fp, fr, fm, tab, out, ws), "srbh_zone_pair_sums")
    first = out.view(torch.int64)[:tab.Z * 10].reshape(-1, 10).clone()
    assert np.array_equal(first.cpu().numpy(), want) and torch.isnan(out[tab.Z * 10:]).all() and torch.isnan(ws[tab.NI * 10:]).all()
    ws.fill_(float("nan"))
    _lib.check(raw_sums(fp, fr, fm, tab, out, ws), "srbh_zone_pair_sums")
    assert torch.equal(out.view(torch.int64)[:tab.Z * 10].reshape(-1, 10), first)
    assert len(zones._device_tables) == 0
    CZ.zone_sums(fp, zones, fm)
    assert len(zones._device_tables) == 1
    held = next(iter(zones._device_tables.values()))[0]
    a, b = CZC.zone_pair_sums(fp, fr, zones, fm, workspace=ws), CZC.zone_pair_sums(fp, fr, zones, fm)
    assert torch.equal(a, b) and torch.equal(a, first) and a.is_cuda
    assert len(zones._device_tables) == 1 and next(iter(zones._device_tables.values()))[0] is held       # nothing was uploaded again
    with pytest.raises(ValueError, match="workspace"):
        CZC.zone_pair_sums(fp, fr, zones, fm, workspace=torch.empty(16, dtype=torch.uint8, device=DEV))


# ---- hostile tables -----------------------------------------------------------------------------------------------------------------------------
def test_hostile_device_tables_stay_inside():
    """wrong tables may give wrong sums of the zones they name; they reach nothing outside the rasters, the tables, out and ws"""
    p, r, m = CO.triple(np.uint16, np.uint8, np.uint8, seed=12)
    fp, fr, fm = framed3(p, r, m)
    NAMED = ZCO.NAMED
    polys = [NAMED["1000-gon"], NAMED["hole"], NAMED["U"], NAMED["bow-tie"], NAMED["diamond through centres"]]
    z = CZ.zone_edges(polys)
    want = ZCO.zone_pair_sums(p, r, polys, m)
    big = 2 ** 30
    # zone 0: its own edges and two beyond the coordinate limit (they contribute nothing); zone 2's edge range ends beyond E; zone 3's
    # starts below 0
    edges = np.concatenate([z.edges[:z.edge_off[1]], [[-big, -big, big, big], [5, INT_MAX, 9, -INT_MAX - 1]], z.edges[z.edge_off[1]:]])
    edge_off = z.edge_off.astype(np.int64).copy()
    edge_off[1:] += 2
    E = len(edges)
    edge_off[3], edge_off[4] = E + 1000, -7                              # zones 2 and 3 broken; zone 4 then starts at -7: broken too
    items, item_off = CZ.zone_items(z, H0, W0, 1000)
    n0, n1 = item_off[1], item_off[2]
    mine = [items[:n0], [(0, W0, 0, 5, 5), (0, -INT_MAX, -INT_MAX, 100, 100), (0, 5, 5, -3, 5)],                # zone 0: + items outside
            [(1, -3, -3, INT_MAX, INT_MAX)],                                                                    # zone 1: one item, clipped
            [(2, 0, 0, W0, H0), (3, 0, 0, W0, H0), (4, 0, 0, W0, H0)],
            [(-1, 0, 0, W0, H0), (5, 0, 0, W0, H0), (INT_MAX, 0, 0, W0, H0), (-INT_MAX - 1, -INT_MAX - 1, -INT_MAX - 1, INT_MAX, INT_MAX)]]
    all_items = np.concatenate([np.array(a, dtype=np.int64).reshape(-1, 5) for a in mine])
    NI = len(all_items)
    item_off = [0, n0 + 3, n0 + 4, n0 + 5, n0 + 6, NI + 5]              # zone 4's item range ends beyond NI: zeros
    tab = Tables(edges, edge_off, all_items, item_off)
    assert tab.Z == 5 and tab.NI == NI and n1 > n0
    ws, out = nan_buffer(NI * 80), nan_buffer(5 * 80)
    _lib.check(raw_sums(fp, fr, fm, tab, out, ws), "srbh_zone_pair_sums")
    got = out.view(torch.int64)[:50].reshape(5, 10).cpu().numpy()
    assert np.array_equal(got[:2], want[:2]) and (got[2:] == 0).all() and (want[2:, 1] > 0).all()
    assert torch.isnan(out[50:]).all() and torch.isnan(ws[NI * 10:]).all()
    # the valid tables next to them are unchanged by all this
    assert np.array_equal(sums(fp, fr, z, fm), want)


# ---- host tables --------------------------------------------------------------------------------------------------------------------------------
def test_zone_errors_and_urban_centre_validation_through_a_geotransform():
    rs = np.random.RandomState(16)
    H, W = 140, 262
    build = np.zeros((H, W), dtype=np.uint8)
    for _ in range(40):
        x, y = rs.randint(0, W - 10), rs.randint(0, H - 10)
        build[y:y + rs.randint(3, 40), x:x + rs.randint(3, 40)] = rs.randint(1, 7)
    height = np.round(10 * rs.gamma(2.0, 6.0, size=(H, W))).astype(np.uint16)
    height[(build == 0) & (rs.rand(H, W) < 0.8)] = 0
    refh = np.clip(height.astype(np.int64) + rs.randint(-40, 41, size=(H, W)), 0, 65535).astype(np.uint16)
    refh[rs.rand(H, W) < 0.6] = 0
    gt = (431000.0, 2.5, 0.0, 4581000.0, 0.0, -2.5)
    centres = []
    for k in range(10):                                                  # blobs in map coordinates, some with a hole
        cx, cy, rad = rs.uniform(0, W), rs.uniform(0, H), rs.uniform(8, 60)
        a = np.sort(rs.uniform(0, 2 * np.pi, size=24))
        rr = rad * rs.uniform(0.6, 1.0, size=24)
        px = np.stack([cx + rr * np.cos(a), cy + rr * np.sin(a)], axis=1)
        rings = [px] + ([np.stack([cx + 0.3 * rad * np.cos(a), cy + 0.3 * rad * np.sin(a)], axis=1)] if k % 4 == 0 else [])
        centres.append([np.stack([gt[0] + q[:, 0] * gt[1], gt[3] + q[:, 1] * gt[5]], axis=1) for q in rings])
    centres.append([np.stack([gt[0] + np.array([1.0, 4.0, 2.0]) * 2.5, gt[3] - np.array([1.0, 1.5, 4.0]) * 2.5], axis=1)])
    height[0:6, 0:6] = 0
    refh[0:6, 0:6] = 0                                                    # the last centre compares nothing: NaN rows
    zones = CZ.zone_edges(centres, gt)
    pix = [[(np.asarray(q) - (gt[0], gt[3])) / (gt[1], gt[5]) for q in z] for z in centres]
    dh, dr, db = dev(height), dev(refh), dev(build)
    for b, d_b in ((build, db), (None, None)):
        ints = ZCO.zone_pair_sums(height, refh, pix, b)
        want = CO.errors(ints)
        assert np.array_equal(CZC.zone_pair_sums(dh, dr, zones, d_b).cpu().numpy(), ints)
        got, own = CZC.zone_errors(dh, dr, zones, d_b), CC.errors_from_sums(ints)
        assert set(got) == set(want) and np.isnan(want["rmse"]).any() and (want["n"] > 500).any()
        for k in ("n", "count"):
            assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), k
        for k in ("fraction", "me", "mae", "rmse", "mean_pred", "mean_ref", "r", "r2"):
            assert CO.same_bits(got[k], want[k]) and CO.same_bits(own[k], want[k]), k
        table, wtab, base = CZC.urban_centre_validation(dh, dr, d_b, zones), ZCO.urban_centre_validation(height, refh, b, pix), \
            CZ.urban_centre_table(dh, d_b, zones)
        assert set(table) == set(wtab) == set(base) | {"me", "mae", "rmse", "mean_pred", "mean_ref", "r", "r2", "n_compared"}
        for k in ("n", "count", "max", "hist", "n_compared") + (("class_counts",) if b is not None else ()):
            assert table[k].dtype == np.int64 and np.array_equal(table[k], wtab[k]), k
        assert b is not None or table["class_counts"] is None
        for k in ("fraction", "mean", "std", "me", "mae", "rmse", "mean_pred", "mean_ref", "r", "r2"):
            assert CO.same_bits(table[k], wtab[k]), k
        for k in ("n", "count", "max", "hist"):
            assert np.array_equal(table[k], base[k]), k
    modes = CZC.zone_errors(dh, dr, zones, db, mode="both", pred_threshold=30, ref_threshold=30)
    assert CO.same_bits(modes["rmse"], CO.errors(ZCO.zone_pair_sums(height, refh, pix, build, "both", 30, 30))["rmse"])


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_c_abi_refusals_launch_nothing():
    p, r, m = CO.triple(np.uint16, np.uint8, np.uint8, seed=17)
    dp, dr, dm = dev(p), dev(r), dev(m)
    polys = [ZCO.NAMED["hole"], ZCO.NAMED["U"]]
    z = CZ.zone_edges(polys)
    items, item_off = CZ.zone_items(z, H0, W0)
    tab = Tables(z.edges, z.edge_off, items, item_off)
    lib, ptr = _lib.lib(), (lambda t: None if t is None or isinstance(t, int) and t == 0 else (t if isinstance(t, int) else t.data_ptr()))
    out = torch.full((2, 10), GARBAGE, dtype=torch.int64, device=DEV)
    ws = torch.full((lib.srbh_zone_pair_ws_bytes(tab.NI) // 8,), GARBAGE, dtype=torch.int64, device=DEV)
    common = dict(p=dp, tp=U16, rsp=W0, r=dr, tr=U8, rsr=W0, m=dm, tm=U8, rsm=W0, H=H0, W=W0, mode=0, pthr=0, rthr=0, mthr=0)

    def call(a):
        return lib.srbh_zone_pair_sums(ptr(a["p"]), a["tp"], a["rsp"], ptr(a["r"]), a["tr"], a["rsr"], ptr(a["m"]), a["tm"], a["rsm"], a["H"], a["W"],
                                       *tab.args(**{k: (ptr(a[k]) if k in ("edges", "edge_off", "items", "item_off") else a[k])
                                                    for k in ("edges", "edge_off", "Z", "E", "items", "item_off", "NI") if k in a}),
                                       a["mode"], a["pthr"], a["rthr"], a["mthr"], ptr(a.get("out", out)), ptr(a.get("ws", ws)), _lib.stream_ptr())

    odd = torch.zeros(64, dtype=torch.uint8, device=DEV)
    changes = [dict(tp=I16), dict(tp=F32), dict(tp=4), dict(tp=-1), dict(tr=I16), dict(tr=F32), dict(tr=7), dict(tm=I16), dict(tm=9),
               dict(tm=F32), dict(m=None), dict(m=None, rsm=0), dict(p=None), dict(r=None), dict(out=None), dict(ws=None),
               dict(H=0), dict(W=0), dict(H=-3), dict(rsp=W0 - 1), dict(rsr=W0 - 1), dict(rsm=W0 - 1),
               dict(H=2 ** 16, W=2 ** 15, rsp=2 ** 15, rsr=2 ** 15, rsm=2 ** 15), dict(mode=-1), dict(mode=4),
               dict(pthr=-2), dict(pthr=65536), dict(rthr=-2), dict(rthr=65536), dict(mthr=-2), dict(mthr=65536),
               dict(p=dp.view(torch.uint8)[:, 1:]), dict(r=dev(r.astype(np.uint16)).view(torch.uint8)[:, 1:], tr=U16),
               dict(m=dev(m.astype(np.uint16)).view(torch.uint8)[:, 1:], tm=U16),
               dict(edges=0), dict(edge_off=0), dict(items=0), dict(item_off=0), dict(Z=0), dict(Z=-1), dict(E=0), dict(E=-5), dict(NI=0),
               dict(NI=-2), dict(edges=tab.t[0].data_ptr() + 4), dict(edge_off=tab.t[1].data_ptr() + 2), dict(items=tab.t[2].data_ptr() + 1),
               dict(item_off=tab.t[3].data_ptr() + 3), dict(out=odd.data_ptr() + 4), dict(ws=odd.data_ptr() + 4)]
    for change in changes:
        rc = call({**common, **change})
        assert rc == ERR_ARG, change
        with pytest.raises(RuntimeError, match="srbh_zone_pair_sums"):
            _lib.check(rc, "srbh_zone_pair_sums")
    assert call({**common, "m": None, "tm": U8, "rsm": 0}) == ERR_ARG    # a type code without its raster
    torch.cuda.synchronize()
    assert (out == GARBAGE).all() and (ws == GARBAGE).all()              # nothing was launched, nothing written: the garbage stands
    assert call(common) == 0
    assert np.array_equal(out.cpu().numpy(), ZCO.zone_pair_sums(p, r, polys, m))
    assert call({**common, "m": None, "tm": 0, "rsm": 0}) == 0
    assert np.array_equal(out.cpu().numpy(), ZCO.zone_pair_sums(p, r, polys))
