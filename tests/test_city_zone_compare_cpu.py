"""CPU: the host half of the urban-centre validation -- the oracle tests/city_zone_compare_oracle.py against a pixel-by-pixel Python
loop, against the city comparison's oracle on integer rectangles, against the polygon zones' oracle under mode "pred" and on the fan's
partition; the C ABI's declarations; every refusal the Python layer can make without a device; and the proof that the oracle is not
blind: each plausible wrong rule changes its result on the GPU tests' own inputs.  No kernel is launched here."""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from srbh_amd import _lib
from srbh_amd import city_zone_compare as CZC
from srbh_amd import city_zones as CZ
from tests import city_compare_oracle as CO
from tests import city_zone_compare_oracle as ZCO
from tests import city_zones_oracle as ZO

ENTRIES = ("srbh_zone_pair_sums", "srbh_zone_pair_ws_bytes")
H0, W0 = ZCO.H0, ZCO.W0


def u16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).view(torch.uint16)


# ---- the oracle against a loop ----------------------------------------------------------------------------------------------------------------
def loop_zone(p, r, m, edges, mode, pthr, rthr, mthr):
    """the definition itself: the crossing count in Fractions, the pair test and the ten sums pixel by pixel in Python integers"""
    H, W = p.shape
    o = [0] * 10
    for y in range(H):
        cy = Fraction(2 * y + 1, 2) * 256
        for x in range(W):
            cx = Fraction(2 * x + 1, 2) * 256
            n = 0
            for X0, Y0, X1, Y1 in edges:
                if min(Y0, Y1) <= cy < max(Y0, Y1):
                    n += X0 + (cy - Y0) * Fraction(X1 - X0, Y1 - Y0) > cx
            if n % 2 == 0:
                continue
            o[0] += 1
            a, b = int(p[y, x]), int(r[y, x])
            P, R = a > pthr, b > rthr
            ok = {"any": P or R, "both": P and R, "ref": R, "pred": P}[mode]
            if not ok or (m is not None and not int(m[y, x]) > mthr):
                continue
            d = a - b
            for k, v in enumerate((1, d, abs(d), d * d, a, b, a * a, b * b, a * b)):
                o[1 + k] += v
    return o


@pytest.mark.parametrize("mode", CO.MODES)
def test_oracle_equals_a_pixel_loop(mode):
    rs = np.random.RandomState(3)
    p, r = rs.randint(0, 5, size=(9, 13)).astype(np.uint16) * 300, rs.randint(0, 5, size=(9, 13)).astype(np.uint8) * 60
    m = rs.randint(0, 9, size=(9, 13)).astype(np.uint8)
    polys = [[ZO.rect(1.5, 1.5, 9.5, 6.5)], [ZO.ring((0.5, 0.5), (12.5, 4), (3.25, 8.75))], [ZO.rect(0, 0, 13, 9), ZO.rect(3.3, 2.2, 8.7, 6.9)],
             [ZO.ring((2, 1), (11, 8), (11, 1), (2, 8))], [ZO.rect(-4, -4, 5.5, 3.5)], [], [ZO.rect(20, 20, 30, 30)]]
    edges = [ZO.zone_edge_list(z) for z in polys]
    for mask, (pthr, rthr, mthr) in ((None, (0, 0, 0)), (m, (0, 0, 0)), (m, (300, 60, 3)), (m, (-1, -1, -1)), (None, (-1, 119, 0))):
        got = ZCO.zone_pair_sums(p, r, polys, mask, mode, pthr, rthr, mthr)
        want = [loop_zone(p, r, mask, e, mode, pthr, rthr, mthr) for e in edges]
        assert got.tolist() == want, (mode, pthr, rthr, mthr)
        assert got[5].tolist() == [0] * 10 and got[6].tolist() == [0] * 10 and got[0, 0] == 8 * 5 and got[2, 0] == 13 * 9 - 6 * 5
    every = ZCO.zone_pair_sums(p, r, polys, m, mode, -1, -1, -1)
    assert np.array_equal(every[:, 0], every[:, 1])                       # every test switched off: the compared pixels ARE the zone's


# ---- ties to the two existing oracles -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case():
    p, r, m = CO.triple(np.uint16, np.uint16, np.uint8)
    return p, r, m, ZO.masks(ZCO.POLYS, H0, W0)


def test_an_integer_rectangle_equals_pair_sums_of_the_window():
    p, r, m = CO.triple(np.uint16, np.uint8, np.uint8)
    pos = CO.edge_windows(H0, W0)[::5]
    zones = ZCO.window_zones(pos)
    for mask in (None, m):
        for mode in CO.MODES:
            for thr in ((0, 0, 0), (254, 6, 6), (-1, -1, -1)):
                assert np.array_equal(ZCO.zone_pair_sums(p, r, zones, mask, mode, *thr), CO.pair_sums(p, r, pos, mask, mode, *thr)), (mode, thr)


def test_mode_pred_equals_the_zone_sums_oracle(case):
    p, r, m, masks = case
    for mask in (None, m):
        for pthr, mthr in ((0, 0), (254, 6), (-1, -1)):
            mine = ZCO.zone_pair_sums(p, r, ZCO.POLYS, mask, "pred", pthr, -1, mthr, masks=masks)
            assert np.array_equal(mine[:, [0, 1, 5, 7]], ZO.zone_sums(p, ZCO.POLYS, mask, pthr, mthr)[:, :4])
            swapped = ZCO.zone_pair_sums(r, p, ZCO.POLYS, mask, "ref", -1, pthr, mthr, masks=masks)
            assert np.array_equal(swapped[:, [0, 1, 6, 8]], mine[:, [0, 1, 5, 7]]) and np.array_equal(swapped[:, 2], -mine[:, 2])


def test_the_fan_of_triangles_sums_to_the_whole_rasters_row(case):
    p, r, m, masks = case
    fan = masks[len(ZCO.NAMES):]
    assert len(fan) == 8 and np.array_equal(np.sum([f.astype(int) for f in fan], axis=0), np.ones((H0, W0), dtype=int))
    for mask in (None, m):
        for mode in CO.MODES:
            rows = ZCO.zone_pair_sums(p, r, ZCO.POLYS, mask, mode, masks=masks)
            whole = CO.pair_sums(p, r, [(0, 0, W0, H0)], mask, mode)[0]
            assert np.array_equal(rows[len(ZCO.NAMES):].sum(axis=0), whole) and (rows[len(ZCO.NAMES):, 1] > 0).all()
            for name in ("everything", "beyond everything", "triangle at the limit"):
                assert np.array_equal(rows[ZCO.NAMES.index(name)], whole), name


# ---- structure --------------------------------------------------------------------------------------------------------------------------------
def test_declared_exported_and_built():
    assert "srbh_zone_compare.hip" in _lib.SOURCES and os.path.exists(os.path.join(_lib.CSRC, "srbh_zone_compare.hip"))
    for h in ("srbh_zone_bitmap.h", "srbh_pair_pieces.h"):
        assert os.path.exists(os.path.join(_lib.CSRC, h)), h
    header = open(os.path.join(_lib.INCLUDE, "srbh.h")).read()
    lib = _lib.lib()
    for name in ENTRIES:
        assert name + "(" in header and name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
    at = header.index("srbh_zone_compare.hip")
    section = header[at:header.index("srbh_zone_pair_ws_bytes(int NI);", at)]
    assert "2^63" in section and "65535^2" in section and "2^31" in section   # the overflow derivation is stated with the new entry
    assert "IN THE ZONE" in section and "COMPARED" in section
    import srbh_amd
    import srbh_amd.city_zone_compare as mod                              # the alias package resolves the new module
    assert mod is CZC and os.path.dirname(mod.__file__) == srbh_amd.__path__[0]
    for n, want in ((1, 80), (7, 560), (301, 24080), (2 ** 24, 2 ** 24 * 80), (0, 0), (-1, 0), (-2 ** 31, 0)):
        assert lib.srbh_zone_pair_ws_bytes(n) == want, n


def test_python_layer_refusals_without_a_device():
    a16, a8 = u16(np.arange(70 * 131).reshape(70, 131) % 65536), torch.zeros((70, 131), dtype=torch.uint8)
    zones = CZ.zone_edges([[ZO.rect(3, 3, 40, 40)]])
    calls = {"zone_pair_sums": lambda p, r, **k: CZC.zone_pair_sums(p, r, k.pop("zones", zones), **k),
             "zone_errors": lambda p, r, **k: CZC.zone_errors(p, r, k.pop("zones", zones), k.pop("mask", None), **k)}
    for fn, call in calls.items():
        with pytest.raises(RuntimeError, match="no CPU"):                # a good call on host tensors: there is no CPU path
            call(a16, a8, mask=a8)
        with pytest.raises(RuntimeError, match="no CPU"):
            call(a8, a16)
        for bad in (a16.view(torch.int16), a8.float(), a8.to(torch.int32)):
            for args, kw in (((bad, a8), {}), ((a16, bad), {}), ((a16, a8), dict(mask=bad))):
                with pytest.raises(TypeError, match="zone_pair_sums"):
                    call(*args, **kw)
        for bad in (torch.zeros((131, 70), dtype=torch.uint8).t(), a8[:, ::2]):
            with pytest.raises(ValueError, match="along W"):
                call(bad, bad)
        with pytest.raises(ValueError, match="along W"):
            call(a16, a8, mask=torch.zeros((131, 70), dtype=torch.uint8).t())
        with pytest.raises(ValueError, match=r"\(H, W\)"):
            call(a8[None], a8[None])
        with pytest.raises(ValueError, match="zone_pair_sums"):
            call(a16, None)
        for other in (a8[:, :-1], a8[:-1]):
            with pytest.raises(ValueError, match="does not match"):
                call(a16, other)
            with pytest.raises(ValueError, match="does not match"):
                call(a16, a8, mask=other)
        for name in ("pred_threshold", "ref_threshold", "mask_threshold"):
            for v in (-2, 65536):
                with pytest.raises(ValueError, match="threshold"):
                    call(a16, a8, mask=a8, **{name: v})
        for mode in ("ANY", "or", 0, None, "xor"):
            with pytest.raises(ValueError, match="mode"):
                call(a16, a8, mode=mode)
        for item_pixels in (0, -1, 2.5, None, True, "64"):
            with pytest.raises(ValueError, match="item_pixels"):
                call(a16, a8, item_pixels=item_pixels)
        for bad in ([[ZO.rect(3, 3, 40, 40)]], None, (zones.edges, zones.edge_off)):
            with pytest.raises(TypeError, match="zone_edges"):
                call(a16, a8, zones=bad)
        with pytest.raises(ValueError, match="no zones"):
            call(a16, a8, zones=CZ.zone_edges([]))
        for ws in (np.zeros(4096), torch.zeros(1 << 16, dtype=torch.uint8), "ws"):
            with pytest.raises(ValueError, match="workspace"):
                call(a16, a8, workspace=ws)
    with pytest.raises(RuntimeError, match="no CPU"):
        CZC.urban_centre_validation(a16, a16, a8, zones)
    with pytest.raises(TypeError, match="zone_edges"):
        CZC.urban_centre_validation(a16, a16, a8, [[ZO.rect(3, 3, 40, 40)]])


# ---- the oracle is not blind --------------------------------------------------------------------------------------------------------------------
def test_each_mistaken_rule_changes_the_oracle_on_the_gpu_tests_inputs(case):
    p, r, m, masks = case
    right = ZCO.zone_pair_sums(p, r, ZCO.POLYS, m, masks=masks)
    for mistake in ("zone_or", "mask_on_count", "r_minus_p"):
        wrong = ZCO.zone_pair_sums(p, r, ZCO.POLYS, m, mistake=mistake, masks=masks)
        assert not np.array_equal(wrong, right), mistake
        changed = [n for k, n in enumerate(ZCO.NAMES) if not np.array_equal(wrong[k], right[k])]
        assert len(changed) >= 10, (mistake, changed)
    corner = ZCO.zone_pair_sums(p, r, ZCO.POLYS, m, mistake="corner")
    assert not np.array_equal(corner, right) and not np.array_equal(corner[:, 0], right[:, 0])
    both = ZCO.zone_pair_sums(p, r, ZCO.POLYS, m, "both", masks=masks)
    assert not np.array_equal(ZCO.zone_pair_sums(p, r, ZCO.POLYS, m, "both", mistake="or_in_both", masks=masks), both)
    tp, tr, tm = ZCO.threshold_rasters()
    for mask in (None, tm):
        for thr in ((0, 0, 0), (254, 254, 6)):
            a = ZCO.zone_pair_sums(tp, tr, ZCO.POLYS, mask, "both", *thr, masks=masks)
            assert not np.array_equal(ZCO.zone_pair_sums(tp, tr, ZCO.POLYS, mask, "both", *thr, mistake="or_in_both", masks=masks), a)
    # the integer rectangles of the window test see the mistakes too (but for the corner rule: their edges lie on pixel corners)
    wz = ZCO.window_zones(CO.edge_windows(H0, W0)[::5])
    for mistake in ("zone_or", "mask_on_count", "r_minus_p", "or_in_both"):
        mode = "both" if mistake == "or_in_both" else "any"
        assert not np.array_equal(ZCO.zone_pair_sums(p, r, wz, m, mode, mistake=mistake), ZCO.zone_pair_sums(p, r, wz, m, mode)), mistake
    assert set(ZCO.MISTAKES) == {"zone_or", "mask_on_count", "r_minus_p", "or_in_both", "corner"}
