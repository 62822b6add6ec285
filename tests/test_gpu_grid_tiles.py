"""GPU: the inference tile cutter (srbh_grid_tiles), loader_math.GridTiles and harness.predict_city against the numpy oracle
tests/grid_oracle.py (a literal restatement of the reference's gridimgLoader.__getitem__, pinned by tests/golden/g18_grid_tiles.npz),
against the parent's own normalize_tiles, and end to end through predict_tiles / evaluate_tiles.

The bound.  Inside a window every element lies within 2^-23 (|v| + |min_c|) / range_c of the float64 oracle: the kernel makes two
correctly rounded fp32 operations, each contributing 2^-24 of at most (|v| + |min|) / range, and the conversion of the source to
float32 is exact for uint16, int16 and float32.  The bound counts the kernel's arithmetic, so every stats value used here (and its
max - min) is a float32 value: the constants reach the kernel unrounded.  Against the fixture, which stores the reference's float32
result, half an ulp of the stored value is added.  Outside a window every element is +0.0 bit for bit.  All elements are compared."""
import os

import numpy as np
import pytest
import torch

from srbh_amd import _lib
from srbh_amd import loader_math as LM
from tests import grid_oracle as GO
from tests.gpu_util import GuardedBuffers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = 8
F32, U16, I16 = 0, 1, 2                                  # include/srbh.h SRBH_GRID_*
CODE = {np.dtype(np.float32): F32, np.dtype(np.uint16): U16, np.dtype(np.int16): I16}
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31

# float32-representable mins and maxs with float32-representable differences (see the bound above)
S2_STATS = np.stack([np.array([100.0, 120.5, -90.25, 0.0, 310.0, 77.0, 5.0, 9.0]),
                     np.array([3100.0, 4020.5, 5090.75, 6000.0, 7310.0, 8077.0, 9005.0, 9009.0])])
S1_STATS = np.stack([np.array([-25.0, -28.5]), np.array([5.0, 2.25])])


def dev(a):
    """a numpy raster on the device as a torch tensor of its own type (uint16 travels as int16 bits)"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).to(DEV).view(torch.uint16)
    return torch.from_numpy(a).to(DEV)


def raster(dtype, Cc, H, W, seed):
    rs = np.random.RandomState(seed)
    if dtype == np.uint16:
        a = rs.randint(0, 9000, size=(Cc, H, W)).astype(np.uint16)
        a[:, 0, 0], a[:, -1, -1] = 65535, 0
    elif dtype == np.int16:
        a = rs.randint(-3000, 6000, size=(Cc, H, W)).astype(np.int16)          # negatives: a sign-extending load
        a[:, 0, 0], a[:, -1, -1] = -32768, 32767
    else:
        a = (rs.rand(Cc, H, W) * 9000 - 1500).astype(np.float32)
    return a


def windows(W, H, n, seed):
    """grid_windows with clipped edges, odd offsets, a 1 x 1 window in the far corner, then random overlapping ones (at least 14) up to n"""
    rs = np.random.RandomState(seed)
    pos = LM.grid_windows(W, H, TILE, 6).tolist() + [[1, 3, 7, 5], [W - 1, H - 1, 1, 1], [5, 1, 8, 8]]
    assert n - len(pos) >= 14
    while len(pos) < n:
        xc, yc = rs.randint(1, TILE + 1, size=2)
        pos.append([int(rs.randint(0, W - xc + 1)), int(rs.randint(0, H - yc + 1)), int(xc), int(yc)])
    return np.array(pos, dtype=np.int64)


def compare(got, s2, s1, pos, s2_stats, s1_stats, nchans, extra=None, want=None):
    """every element of got (N, C, T, T) against the oracle; returns the worst error / bound seen inside the windows"""
    worst = 0.0
    got = got.cpu().numpy()
    T = got.shape[-1]
    for n, w in enumerate(pos):
        xc, yc = int(w[2]), int(w[3])
        ref = GO.cell64(s2, s1, w, s2_stats, s1_stats, nchans) if want is None else want[n].astype(np.float64)
        bnd = GO.bound(s2, s1, w, s2_stats, s1_stats, nchans) + (0.0 if extra is None else extra[n])
        err = np.abs(got[n, :, :yc, :xc].astype(np.float64) - ref)
        ratio = np.divide(err, bnd, out=np.zeros_like(err), where=bnd > 0)      # (v = min = 0: the bound is 0 and so is the error)
        assert (err <= bnd).all(), f"window {n} {tuple(w)}: error {err.max():.3e} beyond the bound (worst ratio {ratio.max():.3f})"
        worst = max(worst, float(ratio.max()))
        outside = np.ones((T, T), dtype=bool)
        outside[:yc, :xc] = False
        assert not got[n].view(np.int32)[:, outside].any(), f"window {n} {tuple(w)}: not +0.0 outside the window"
    return worst


TYPE_PAIRS = {"u16_f32": (np.uint16, np.float32), "i16_f32": (np.int16, np.float32), "f32_f32": (np.float32, np.float32),
              "u16_none": (np.uint16, None)}


@pytest.mark.parametrize("size", [(20, 24), (21, 27)], ids=lambda s: f"{s[0]}x{s[1]}")      # the odd width misaligns 16-bit rows
@pytest.mark.parametrize("pair", list(TYPE_PAIRS))
def test_every_element_against_the_float64_oracle(size, pair):
    H, W = size
    tA, tB = TYPE_PAIRS[pair]
    worst = 0.0
    for C2, nchans in ((8, 6), (3, 3)):
        s2 = raster(tA, C2, H, W, seed=H * 100 + C2)
        s1 = None if tB is None else raster(tB, 2, H, W, seed=H * 100 + 50 + C2)
        if s1 is not None:
            s1 = (s1 / 225.0 - 26.0).astype(np.float32)                       # a Sentinel-1 band's range of values
        s2_stats, s1_stats = S2_STATS[:, :C2], None if s1 is None else S1_STATS
        pos = windows(W, H, 37, seed=W)
        gt = LM.GridTiles(dev(s2), None if s1 is None else dev(s1), pos, s2_stats, s1_stats, nchans=nchans, tile=TILE)
        assert gt.shape == (37, nchans + (0 if s1 is None else 2), TILE, TILE) and len(gt) == 37 and gt.device == torch.device(DEV)
        assert np.array_equal(gt.pos, pos)
        got = gt[0:37]
        assert got.dtype == torch.float32 and tuple(got.shape) == gt.shape and got.is_contiguous()
        worst = max(worst, compare(got, s2, s1, pos, s2_stats, s1_stats, nchans))
        for n in (0, 13, 36):                                                  # N = 1: one launch per single window
            one = gt[n:n + 1]
            assert tuple(one.shape) == (1,) + gt.shape[1:] and torch.equal(one[0], got[n])
    print(f"\n[grid_tiles] {size[0]}x{size[1]} {pair}: worst error / bound = {worst:.3f}")
    assert 0.0 < worst <= 1.0


def test_against_the_reference_fixture(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "g18_grid_tiles.npz")))
    nchans, tile, pos = int(g["nchans"]), int(g["tile"]), g["windows"]
    gt = LM.GridTiles(dev(g["s2"]), dev(g["s1"]), pos, g["s2_stats"], g["s1_stats"], nchans=nchans, tile=tile)
    imgs = [g[f"img_{i}"] for i in range(len(pos))]
    for i in range(len(pos)):
        assert np.array_equal(gt.pos[i], g[f"pos_{i}"])                        # the window the reference returned with the image
    half_ulp = [np.spacing(np.abs(im)).astype(np.float64) / 2 for im in imgs]
    worst = compare(gt[:], g["s2"], g["s1"], pos, g["s2_stats"], g["s1_stats"], nchans, extra=half_ulp, want=imgs)
    print(f"\n[grid_tiles] fixture: worst error / (bound + half an ulp) = {worst:.3f}")


def test_full_tiles_equal_the_parents_normalize_tiles_bit_for_bit():
    H, W, T, nchans = 130, 150, 64, 6
    s2, s1 = raster(np.uint16, 8, H, W, seed=1), (raster(np.float32, 2, H, W, seed=2) / 225.0 - 26.0).astype(np.float32)
    pos = np.array([[0, 0, T, T], [64, 0, T, T], [86, 66, T, T], [1, 3, T, T], [33, 17, T, T], [85, 65, T, T], [0, 66, T, T]])
    gt = LM.GridTiles(dev(s2), dev(s1), pos, S2_STATS, S1_STATS, nchans=nchans, tile=T)
    crops = [torch.from_numpy(np.concatenate([s2[:nchans, y:y + T, x:x + T].astype(np.float32), s1[:, y:y + T, x:x + T]]))
             for x, y, _, _ in pos]
    mins = np.concatenate([S2_STATS[0, :nchans], S1_STATS[0]])
    maxs = np.concatenate([S2_STATS[1, :nchans], S1_STATS[1]])
    want = LM.normalize_tiles(torch.stack(crops).float().to(DEV), mins, maxs, None)
    got = gt[:]
    assert tuple(got.shape) == (7, 8, T, T)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# ---- the memory contract of the C entry ---------------------------------------------------------------------------------------------
def embedded(a, margin):
    """`a` in the middle of a larger device buffer whose margins hold 0xFFFF (16-bit types) or NaN: (buffer, address of the raster,
    host copy of the whole buffer).  A read outside the raster shows up as a wrong value, no fault needed."""
    flat = np.full((a.size + 2 * margin,), 0xFFFF if a.dtype.itemsize == 2 else np.nan, dtype=np.uint16 if a.dtype.itemsize == 2 else a.dtype)
    flat = flat.view(a.dtype)
    flat[margin:margin + a.size] = a.reshape(-1)
    buf = torch.from_numpy(flat.view(np.int16) if a.dtype.itemsize == 2 else flat).to(DEV)
    return buf, buf.data_ptr() + margin * a.dtype.itemsize, flat.copy()


def call(srcA, typeA, CA, CA_used, srcB, typeB, CB, H, W, pos, N, mins, ranges, dst, tile):
    ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())      # noqa: E731
    return _lib.lib().srbh_grid_tiles(ptr(srcA), typeA, CA, CA_used, ptr(srcB), typeB, CB, H, W, ptr(pos), N, ptr(mins), ptr(ranges),
                                      ptr(dst), tile, _lib.stream_ptr())


def expected_tile(s2, s1, w, nchans, mins, ranges, T):
    """the definition, element by element, for ANY window: inside the window AND inside the raster the float64 value and its bound,
    elsewhere None"""
    H, W = s2.shape[1:]
    xoff, yoff, xc, yc = (int(v) for v in w)
    val = np.zeros((len(mins), T, T))
    bnd = np.full((len(mins), T, T), -1.0)
    for j in range(T):
        for i in range(T):
            x, y = xoff + i, yoff + j
            if i < xc and j < yc and 0 <= x < W and 0 <= y < H:
                v = np.concatenate([s2[:nchans, y, x].astype(np.float64), s1[:, y, x].astype(np.float64)])
                val[:, j, i] = (v - mins) / ranges
                bnd[:, j, i] = 2.0 ** -23 * (np.abs(v) + np.abs(mins)) / np.abs(ranges)
    return val, bnd


@pytest.mark.parametrize("tA", [np.uint16, np.int16, np.float32], ids=lambda t: np.dtype(t).name)
def test_memory_contract_of_the_c_entry(tA):
    H, W, nchans = 21, 27, 6
    s2, s1 = raster(tA, 8, H, W, seed=5), (raster(np.float32, 2, H, W, seed=6) / 225.0 - 26.0).astype(np.float32)
    bufA, ptrA, hostA = embedded(s2, margin=1001)                              # an odd margin: the raster starts 2-byte aligned only
    bufB, ptrB, hostB = embedded(s1, margin=999)
    inside = [[0, 0, 8, 8], [W - 8, 0, 8, 8], [0, H - 8, 8, 8], [W - 8, H - 8, 8, 8], [W - 3, H - 5, 3, 5], [11, 0, 5, 8], [0, 9, 8, 3]]
    past = [[W - 3, 0, 8, 8], [0, H - 2, 8, 8], [W - 1, H - 1, 8, 8], [-3, -2, 8, 8], [-8, 0, 8, 8], [W, H, 8, 8], [0, -1, 8, 8],
            [INT_MAX - 2, 0, 8, 8], [0, INT_MAX - 2, 8, 8], [INT_MIN, INT_MIN, 8, 8], [INT_MAX, INT_MAX, INT_MAX, INT_MAX],
            [3, 2, INT_MAX, INT_MAX], [3, 2, -1, 8], [3, 2, 8, INT_MIN], [3, 2, 0, 0], [0, 0, 99, 2]]
    pos = np.array(inside + past, dtype=np.int64)
    mins = np.concatenate([S2_STATS[0, :nchans], S1_STATS[0]])
    ranges = np.concatenate([S2_STATS[1, :nchans], S1_STATS[1]]) - mins
    G = GuardedBuffers()
    pos_d = torch.from_numpy(pos.astype(np.int32)).to(DEV)
    mins_d, ranges_d = G.inp(torch.from_numpy(mins.astype(np.float32)), offset=1), G.inp(torch.from_numpy(ranges.astype(np.float32)), offset=3)
    dst = G.out((len(pos), nchans + 2, TILE, TILE))
    _lib.check(call(ptrA, CODE[np.dtype(tA)], 8, nchans, ptrB, F32, 2, H, W, pos_d, len(pos), mins_d, ranges_d, dst, TILE), "grid_tiles")
    G.verify()                                                                 # guards intact, inputs unchanged, every dst element written (no NaN)
    for buf, host in ((bufA, hostA), (bufB, hostB), (pos_d, pos.astype(np.int32))):                # the inputs are as they were, bit for bit
        assert np.array_equal(buf.cpu().numpy().view(np.uint8), host.view(np.uint8))
    got = dst.cpu().numpy()
    for n, w in enumerate(pos):
        val, bnd = expected_tile(s2, s1, w, nchans, mins, ranges, TILE)
        live = bnd >= 0
        assert (np.abs(got[n].astype(np.float64) - val)[live] <= bnd[live]).all(), f"window {n} {tuple(w)}: a wrong value"
        assert not got[n].view(np.int32)[~live].any(), f"window {n} {tuple(w)}: not +0.0 outside the window or the raster"


def _good_call():
    s2, s1 = dev(raster(np.uint16, 8, 20, 24, seed=7)), dev(raster(np.float32, 2, 20, 24, seed=8))
    pos = torch.tensor([[0, 0, 8, 8], [3, 5, 7, 2]], dtype=torch.int32, device=DEV)
    mins, ranges = torch.zeros(8, device=DEV), torch.ones(8, device=DEV)
    kw = dict(srcA=s2, typeA=U16, CA=8, CA_used=6, srcB=s1, typeB=F32, CB=2, H=20, W=24, pos=pos, N=2, mins=mins, ranges=ranges, tile=TILE)
    return kw


REFUSALS = {
    "null srcA": dict(srcA=None), "null pos": dict(pos=None), "null dst": dict(dst=None), "null mins": dict(mins=None),
    "null ranges": dict(ranges=None), "srcB without CB": dict(CB=0), "CB without srcB": dict(srcB=None), "negative CB": dict(CB=-1),
    "unknown typeA": dict(typeA=3), "negative typeA": dict(typeA=-1), "unknown typeB": dict(typeB=7), "CA_used 0": dict(CA_used=0),
    "CA_used above CA": dict(CA_used=9), "N 0": dict(N=0), "negative N": dict(N=-2), "H 0": dict(H=0), "W 0": dict(W=0),
    "negative W": dict(W=-24), "tile 0": dict(tile=0), "tile 2": dict(tile=2), "tile 6": dict(tile=6), "tile 260": dict(tile=260),
    "misaligned dst": dict(dst="misaligned"), "too many workgroups": dict(N=INT_MAX, tile=256),
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_c_entry_refusals_name_the_entry_and_write_nothing(what):
    kw = _good_call()
    G = GuardedBuffers()
    kw["dst"] = G.out((2, 8, TILE, TILE))
    assert call(**kw) == 0                                                     # the call the refusals are one change away from
    G = GuardedBuffers()
    kw["dst"] = G.out((2, 8, TILE, TILE))
    kw.update(REFUSALS[what])
    if isinstance(kw["dst"], str):
        kw["dst"] = G.out((2, 8, TILE, TILE), offset=1)
    rc = call(**kw)
    assert rc == -1
    with pytest.raises(RuntimeError, match="srbh_grid_tiles"):
        _lib.check(rc, "grid_tiles")
    G.verify(written=False)


def test_gridtiles_refusals_name_gridtiles():
    s2, s1 = dev(raster(np.uint16, 8, 20, 24, seed=7)), dev(raster(np.float32, 2, 20, 24, seed=8))
    pos = [[0, 0, 8, 8]]
    ok = LM.GridTiles(s2, s1, pos, S2_STATS, S1_STATS, tile=TILE)
    assert ok.shape == (1, 8, TILE, TILE)
    zero = S2_STATS.copy()
    zero[1, 2] = zero[0, 2]
    cases = [
        (dict(s2=s2.view(torch.int16).cpu()), "CPU s2"), (dict(s1=s1.cpu()), "CPU s1"), (dict(s2=s2.view(torch.uint8)), "uint8 s2"),
        (dict(s1=s1.double()), "float64 s1"), (dict(s2=s2[0]), "2-d s2"), (dict(s1=s1[:, :19]), "s1 of another height"),
        (dict(s1=s1[:, :, :23]), "s1 of another width"), (dict(s2_stats=S2_STATS[:, :5]), "too few s2 stats"),
        (dict(s1_stats=S1_STATS[:, :1]), "too few s1 stats"), (dict(s2_stats=zero), "zero range"), (dict(nchans=9), "nchans above C"),
        (dict(nchans=0), "nchans 0"), (dict(pos=[[0, 0, 8, 8], [17, 0, 8, 8]]), "window past the edge"), (dict(pos=[[0, 0, 9, 8]]), "window above tile"),
        (dict(pos=[]), "no windows"), (dict(tile=6), "tile 6"),
    ]
    for change, what in cases:
        kw = dict(s2=s2, s1=s1, pos=pos, s2_stats=S2_STATS, s1_stats=S1_STATS, nchans=6, tile=TILE)
        kw.update(change)
        with pytest.raises((RuntimeError, TypeError, ValueError), match="GridTiles"):
            LM.GridTiles(**kw)
            pytest.fail(what)
    with pytest.raises(ValueError, match=r"GridTiles.*row 1 "):
        LM.GridTiles(s2, s1, [[0, 0, 8, 8], [17, 0, 8, 8]], S2_STATS, S1_STATS, tile=TILE)
    for key in (0, slice(0, 1, 2), (slice(0, 1), 0)):
        with pytest.raises(TypeError, match="GridTiles"):
            ok[key]


def test_memo_keeps_a_slice_until_two_further_distinct_slices_were_requested():
    H, W = 21, 27
    s2, s1 = raster(np.uint16, 8, H, W, seed=9), (raster(np.float32, 2, H, W, seed=10) / 225.0 - 26.0).astype(np.float32)
    pos = windows(W, H, 37, seed=3)[:20]
    gt = LM.GridTiles(dev(s2), dev(s1), pos, S2_STATS, S1_STATS, tile=TILE)
    a = gt[0:4]
    want = a.clone()
    compare(a, s2, s1, pos[0:4], S2_STATS, S1_STATS, 6)
    b = gt[4:8]
    assert torch.equal(a, want) and b.data_ptr() != a.data_ptr()
    assert gt[0:4] is a                                                        # asked for twice, made once
    c = gt[8:12]                                                               # the second further distinct slice: `a` is still valid
    torch.cuda.synchronize()
    assert torch.equal(a, want) and len({a.data_ptr(), b.data_ptr(), c.data_ptr()}) == 3
    assert gt[4:8] is b and gt[0:4] is a
    del a
    gt[12:16]                                                                  # the third: the memo lets go of [0:4] ...
    again = gt[0:4]                                                            # ... and makes it anew, with equal values
    assert torch.equal(again, want)
    compare(gt[16:20], s2, s1, pos[16:20], S2_STATS, S1_STATS, 6)
    assert torch.equal(gt[:], torch.cat([gt[i:i + 4] for i in range(0, 20, 4)]))


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def _city_rasters():
    rs = np.random.RandomState(11)
    s2 = rs.randint(200, 3000, size=(8, 208, 208)).astype(np.uint16)
    s1 = (rs.rand(2, 208, 208) * 20 - 24).astype(np.float32)
    s2_stats = np.stack([np.zeros(8), np.full(8, 4096.0)])
    s1_stats = np.stack([np.full(2, -32.0), np.full(2, 0.0)])
    return s2, s1, s2_stats, s1_stats, LM.grid_windows(208, 208, 64, 48)[:13]


def test_a_city_from_its_rasters_equals_the_city_from_resident_tiles():
    """13 stride-48 cells at batch 4: three replays of the captured graph (each full batch asked for as the next one and as the current
    one) and a ragged tail of one"""
    from srbh_amd import harness
    from srbh_amd.mosaic import Mosaic
    from tests import test_gpu_predict_sharded as PS
    s2, s1, s2_stats, s1_stats, pos = _city_rasters()
    net_hr, model = PS._nets()
    s2_d, s1_d = dev(s2), dev(s1)

    def run(tiles, posall):
        m = Mosaic(4 * 208, 4 * 208, 7, DEV)
        assert harness.predict_tiles(net_hr, model, tiles, posall, m, batch=4) == 13
        h, b = m.finalize()
        return h.cpu().to(torch.int32), b.cpu()

    gt = LM.GridTiles(s2_d, s1_d, pos, s2_stats, s1_stats)
    assert gt.shape == (13, 8, 64, 64)
    h_gt, b_gt = run(gt, gt.pos)
    assert model.__dict__.get("_srbh_predict_graph") is not None               # the full batches went through the captured graph
    assert [k for k, _ in gt._memo] == [(4, 8), (8, 12), (12, 13)]             # every batch was made, the last three are still held
    resident = LM.GridTiles(s2_d, s1_d, pos, s2_stats, s1_stats)[0:13].clone()
    compare(resident[:2], s2, s1, pos[:2], s2_stats, s1_stats, 6)
    h_t, b_t = run(resident, pos.tolist())
    h_c, b_c = harness.predict_city(net_hr, model, s2_d, s1_d, pos, s2_stats, s1_stats, batch=4)
    assert h_c.dtype == torch.uint16 and b_c.dtype == torch.uint8 and tuple(h_c.shape) == (832, 832) == tuple(b_c.shape)
    h_c, b_c = h_c.cpu().to(torch.int32), b_c.cpu()
    assert torch.equal(h_gt, h_t) and torch.equal(b_gt, b_t)
    assert torch.equal(h_c, h_t) and torch.equal(b_c, b_t)
    assert int(b_t.max()) <= 6 and (bool(h_t.any()) or b_t.unique().numel() > 1)          # (not a trivially empty mosaic)


def test_evaluate_tiles_scores_gridtiles_as_the_resident_tensor():
    from srbh_amd import harness
    from tests import test_gpu_predict_sharded as PS
    s2, s1, s2_stats, s1_stats, pos = _city_rasters()
    net_hr, model = PS._nets()
    g = torch.Generator().manual_seed(29)
    label = torch.randint(0, 7, (13, 32, 32), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)
    ref = (torch.randint(0, 60, (13, 256, 256), generator=g) * (label > 0)).float().to(DEV)
    label = label.to(DEV)
    gt = LM.GridTiles(dev(s2), dev(s1), pos, s2_stats, s1_stats)
    resident = gt[:].clone()
    a = harness.evaluate_tiles(net_hr, model, gt, ref, label, batch=4, ref_batch=4)
    b = harness.evaluate_tiles(net_hr, model, resident, ref, label, batch=4, ref_batch=4)
    assert a.count == 13 == b.count
    for x, y in zip(a.image_sums(), b.image_sums()):
        assert torch.equal(x, y)
    ra, rb = a.result(), b.result()
    for k in ("loss", "rmse", "acc_total"):
        assert torch.equal(torch.as_tensor(ra[k]), torch.as_tensor(rb[k])), k
    assert torch.equal(ra["height"].stats, rb["height"].stats) and torch.equal(ra["seg"].confusionMatrix, rb["seg"].confusionMatrix)
