"""CPU: the host half of the city comparison -- the numpy oracle tests/city_compare_oracle.py against a pixel-by-pixel Python loop and
against the city summary's oracle, city_compare.errors_from_sums against fractions.Fraction bit for bit and against a 60-digit decimal
evaluation, the C ABI's declarations, every refusal the Python layer can make without a device, and the proof that the oracle is not
blind: each plausible wrong rule changes its result on the GPU tests' own inputs.  No kernel is launched here."""
import math
import os
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np
import pytest
import torch

from srbh_amd import _lib
from srbh_amd import city_compare as CC
from tests import city_compare_oracle as CO
from tests import city_summary_oracle as SO

ENTRIES = ("srbh_pair_sums", "srbh_pair_class_sums", "srbh_pair_class_ws_bytes")


def u16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).view(torch.uint16)


# ---- the oracle against a loop and against the summary's oracle ---------------------------------------------------------------------------
def loop_pair(p, r, m, win, mode, pthr, rthr, mthr):
    H, W = p.shape
    x, y, w, h = win
    o = [0] * 10
    for yy in range(y, y + h):
        for xx in range(x, x + w):
            if not (0 <= yy < H and 0 <= xx < W):
                continue
            o[0] += 1
            a, b = int(p[yy, xx]), int(r[yy, xx])
            P, R = a > pthr, b > rthr
            ok = {"any": P or R, "both": P and R, "ref": R, "pred": P}[mode]
            if not ok or (m is not None and not int(m[yy, xx]) > mthr):
                continue
            d = a - b
            for k, v in enumerate((1, d, abs(d), d * d, a, b, a * a, b * b, a * b)):
                o[1 + k] += v
    return o


def loop_class(p, r, m, edges, mode, pthr, rthr, mthr):
    C = len(edges)
    rows, bad = [[0] * (4 + C) for _ in range(C)], 0
    cls = lambda v: sum(1 for k in range(1, C) if v >= edges[k])
    for yy in range(p.shape[0]):
        for xx in range(p.shape[1]):
            a, b = int(p[yy, xx]), int(r[yy, xx])
            P, R = a > pthr, b > rthr
            ok = {"any": P or R, "both": P and R, "ref": R, "pred": P}[mode]
            if not ok or (m is not None and not int(m[yy, xx]) > mthr):
                continue
            c, pc, d = cls(b), (int(m[yy, xx]) if m is not None else cls(a)), a - b
            for k, v in enumerate((1, d, abs(d), d * d)):
                rows[c][k] += v
            if pc < C:
                rows[c][4 + pc] += 1
            else:
                bad += 1
    return rows, bad


@pytest.mark.parametrize("mode", CO.MODES)
def test_oracle_equals_a_pixel_loop(mode):
    rs = np.random.RandomState(3)
    p, r = rs.randint(0, 5, size=(9, 13)).astype(np.uint16) * 300, rs.randint(0, 5, size=(9, 13)).astype(np.uint8) * 60
    m = rs.randint(0, 9, size=(9, 13)).astype(np.uint8)
    wins = [(0, 0, 13, 9), (3, 2, 5, 4), (-2, -1, 6, 6), (10, 7, 9, 9), (20, 0, 3, 3), (1, 1, 0, 4), (12, 8, 1, 1)]
    for mask, (pthr, rthr, mthr) in ((None, (0, 0, 0)), (m, (0, 0, 0)), (m, (300, 60, 3)), (m, (-1, -1, -1)), (None, (-1, 119, 0))):
        got = CO.pair_sums(p, r, wins, mask, mode, pthr, rthr, mthr)
        assert got.tolist() == [loop_pair(p, r, mask, w, mode, pthr, rthr, mthr) for w in wins], (mode, pthr, rthr, mthr)
        for edges in ((0, 60), (0, 60, 120, 300, 301, 1200, 1201)):
            rows, bad = CO.class_sums(p, r, edges, mask, mode, pthr, rthr, mthr)
            want_rows, want_bad = loop_class(p, r, mask, edges, mode, pthr, rthr, mthr)
            assert rows.tolist() == want_rows and bad == want_bad, (mode, edges)
            assert rows[:, 4:].sum() + bad == rows[:, 0].sum()
            assert rows[:, :4].sum(0).tolist() == CO.pair_sums(p, r, [(0, 0, 13, 9)], mask, mode, pthr, rthr, mthr)[0, 1:5].tolist()


def test_oracle_agrees_with_the_city_summary_oracle():
    """under mode "pred" with the reference test switched off the pair rule IS the selection rule of window_sums"""
    p, r, m = CO.triple(np.uint16, np.uint16, np.uint8)
    pos = CO.edge_windows(CO.H0, CO.W0)[::7]
    for mask in (None, m):
        for pthr, mthr in ((0, 0), (254, 6), (-1, -1)):
            mine = CO.pair_sums(p, r, pos, mask, "pred", pthr, -1, mthr)
            assert np.array_equal(mine[:, [0, 1, 5, 7]], SO.window_sums(p, pos, mask, pthr, mthr)[:, :4])
            swapped = CO.pair_sums(r, p, pos, mask, "ref", -1, pthr, mthr)       # the same pixels seen from the other side
            assert np.array_equal(swapped[:, [0, 1, 6, 8]], mine[:, [0, 1, 5, 7]]) and np.array_equal(swapped[:, 2], -mine[:, 2])


# ---- errors_from_sums -------------------------------------------------------------------------------------------------------------------------
def rows_of(pairs, count=None):
    """(N, 10) rows of lists of compared (p, r) pairs, in Python integers"""
    out = []
    for w in pairs:
        d = [a - b for a, b in w]
        out.append([count or max(len(w), 1), len(w), sum(d), sum(abs(t) for t in d), sum(t * t for t in d), sum(a for a, _ in w),
                    sum(b for _, b in w), sum(a * a for a, _ in w), sum(b * b for _, b in w), sum(a * b for a, b in w)])
    return np.array(out, dtype=np.int64)


def ulps(a, b):
    return abs(a - b) / math.ulp(b)


def test_errors_from_sums_against_fractions_and_decimals():
    rs = np.random.RandomState(1)
    rnd = lambda n, hi: list(zip(rs.randint(0, hi, size=n).tolist(), rs.randint(0, hi, size=n).tolist()))
    near = [(int(a), int(min(65535, max(0, a + e)))) for a, e in zip(rs.randint(0, 65536, size=5000), rs.randint(-40, 41, size=5000))]
    wins = [[], [(7, 9)] * 300, [(65535, 0)] * 2 ** 16, [(65534, 65535), (65535, 65534)], [(65534, 65535)] * 1000 + [(65535, 65534)] * 1001,
            [(0, 0)] * 3, [(1, 0)], [(3, 4), (4, 3), (5, 5)], rnd(4096, 65536), rnd(777, 300), near, [(5, 1), (5, 2), (5, 9)], [(1, 5), (2, 5), (9, 5)]]
    sums = rows_of(wins, count=2 ** 17)
    got, want = CC.errors_from_sums(sums), CO.errors(sums)
    for k in ("n", "count"):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), k
    for k in ("fraction", "me", "mae", "rmse", "mean_pred", "mean_ref", "r", "r2"):
        assert got[k].dtype == np.float64 and CO.same_bits(got[k], want[k]), k
    getcontext().prec = 60
    for i, row in enumerate(sums.tolist()):
        count, n, sd, sad, sdd, sp, sr, spp, srr, spr = (int(v) for v in row)
        if n == 0:
            continue
        # me, mae and the quotient under the root: bit for bit the correctly rounded rational
        assert got["me"][i] == float(Fraction(sd, n)) and got["mae"][i] == float(Fraction(sad, n))
        assert got["rmse"][i] == math.sqrt(float(Fraction(sdd, n))) and got["rmse"][i] ** 2 == pytest.approx(sdd / n, rel=1e-15)
        vp, vr, cov = n * spp - sp * sp, n * srr - sr * sr, n * spr - sp * sr
        if vp and vr:
            exact = float(Decimal(cov) / (Decimal(vp) * Decimal(vr)).sqrt())
            assert ulps(got["r"][i], exact) <= 4, (i, got["r"][i], exact)
            assert ulps(got["r2"][i], float(Decimal(1) - Decimal(n * sdd) / Decimal(vr))) <= 4, i
        else:
            assert math.isnan(got["r"][i])
    # n == 0; a constant pair; a constant reference (r and r2 NaN); a constant prediction (r NaN, r2 finite)
    assert all(math.isnan(got[k][0]) for k in ("me", "mae", "rmse", "mean_pred", "mean_ref", "r", "r2")) and got["fraction"][0] == 0.0
    assert got["me"][1] == -2.0 and got["mae"][1] == 2.0 and got["rmse"][1] == 2.0 and math.isnan(got["r"][1]) and math.isnan(got["r2"][1])
    assert got["rmse"][2] == 65535.0 and got["me"][2] == 65535.0 and got["mean_ref"][2] == 0.0
    assert math.isnan(got["r"][11]) and not math.isnan(got["r2"][11]) and math.isnan(got["r"][12]) and math.isnan(got["r2"][12])
    # {65534, 65535} against {65535, 65534}: the integer form gives r = -1 exactly ...
    assert got["r"][3] == -1.0 and got["r2"][3] == -3.0 and got["rmse"][3] == 1.0 and got["me"][3] == 0.0
    assert abs(got["r"][4] + 1.0) < 1e-12
    # ... where the float64 form E[x^2] - E[x]^2 cancels: with 2 001 such pairs it does not give the variance 0.25 (1 - 1 / 2001^2), nor r
    n, sp, sr, spp, srr, spr = (float(v) for v in sums[4, [1, 5, 6, 7, 8, 9]])
    vp, vr, cov = spp / n - (sp / n) ** 2, srr / n - (sr / n) ** 2, spr / n - (sp / n) * (sr / n)
    true_var = float(Fraction(2001 ** 2 - 1, 4 * 2001 ** 2))
    assert abs(vp - true_var) > 1e-9 and abs(vr - true_var) > 1e-9 and abs(cov + true_var) > 1e-9      # every digit behind 0.25 is lost
    n, sp, sr, spp, srr, spr = (int(v) for v in sums[4, [1, 5, 6, 7, 8, 9]])
    assert Fraction(n * spp - sp * sp, n * n) == Fraction(n * srr - sr * sr, n * n) == -Fraction(n * spr - sp * sr, n * n) == Fraction(2001 ** 2 - 1, 4 * 2001 ** 2)
    out = CC.errors_from_sums(np.zeros((1, 10), dtype=np.int64))         # count == 0 (a window wholly outside the raster)
    assert all(math.isnan(out[k][0]) for k in ("fraction", "me", "rmse", "r", "r2")) and out["n"][0] == out["count"][0] == 0
    for bad in (np.zeros((3, 5), dtype=np.int64), np.zeros((2, 10), dtype=np.float64), np.zeros(10, dtype=np.int64)):
        with pytest.raises(ValueError, match="errors_from_sums"):
            CC.errors_from_sums(bad)


# ---- structure --------------------------------------------------------------------------------------------------------------------------------
def test_declared_exported_and_built():
    assert "srbh_compare.hip" in _lib.SOURCES and os.path.exists(os.path.join(_lib.CSRC, "srbh_compare.hip"))
    header = open(os.path.join(_lib.INCLUDE, "srbh.h")).read()
    lib = _lib.lib()
    for name in ENTRIES:
        assert name + "(" in header and name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
    for k, v in CC.MODES.items():
        assert f"#define SRBH_PAIR_{k.upper()} {v}\n" in header
    assert "2^63" in header and "65535^2" in header                      # the overflow derivation is stated
    import srbh_amd
    import srbh_amd.city_compare as mod                                  # the alias package resolves the new module
    assert mod is CC and os.path.dirname(mod.__file__) == srbh_amd.__path__[0]
    L = _lib.lib()
    assert L.srbh_pair_class_ws_bytes(0, 5, 7) == 0 and L.srbh_pair_class_ws_bytes(5, 5, 1) == 0 and L.srbh_pair_class_ws_bytes(5, 5, 17) == 0
    assert L.srbh_pair_class_ws_bytes(2 ** 16, 2 ** 15, 7) == 0
    assert L.srbh_pair_class_ws_bytes(70, 131, 7) % ((7 * 11 + 1) * 8) == 0 < L.srbh_pair_class_ws_bytes(70, 131, 7)
    assert L.srbh_pair_class_ws_bytes(12000, 16000, 16) == 2048 * (16 * 20 + 1) * 8


def test_python_layer_refusals_without_a_device():
    a16, a8 = u16(np.arange(70 * 131).reshape(70, 131) % 65536), torch.zeros((70, 131), dtype=torch.uint8)
    pos = np.array([(0, 0, 16, 16)])
    calls = {"pair_sums": lambda p, r, **k: CC.pair_sums(p, r, k.pop("pos", pos), **k),
             "class_sums": lambda p, r, **k: CC.class_sums(p, r, k.pop("edges", CC.DEFAULT_EDGES), build=k.pop("mask", None), **k)}
    for fn, call in calls.items():
        with pytest.raises(RuntimeError, match="no CPU"):                # a good call on host tensors: there is no CPU path
            call(a16, a8, mask=a8)
        with pytest.raises(RuntimeError, match="no CPU"):
            call(a8, a16)
        for bad in (a16.view(torch.int16), a8.float(), a8.to(torch.int32)):
            for args, kw in (((bad, a8), {}), ((a16, bad), {}), ((a16, a8), dict(mask=bad))):
                with pytest.raises(TypeError, match=fn):
                    call(*args, **kw)
        for bad in (torch.zeros((131, 70), dtype=torch.uint8).t(), a8[:, ::2]):
            with pytest.raises(ValueError, match="along W"):
                call(bad, bad)
        with pytest.raises(ValueError, match="along W"):
            call(a16, a8, mask=torch.zeros((131, 70), dtype=torch.uint8).t())
        with pytest.raises(ValueError, match=r"\(H, W\)"):
            call(a8[None], a8[None])
        with pytest.raises(ValueError, match=fn):
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
    for edges in ((0,), tuple(range(17)), (1, 2, 3), (0, 30, 30), (0, 40, 30), (0, 1.5), (0, True), 7, (0, 2 ** 31), (-1, 0, 5)):
        with pytest.raises(ValueError, match="class_sums"):
            CC.class_sums(a16, a8, edges)
        with pytest.raises(ValueError, match="class_sums"):
            CC.city_validation(a16, a8, None, edges)
    for ws in (np.zeros(4096), torch.zeros(1 << 16, dtype=torch.uint8), "ws"):
        with pytest.raises(ValueError, match="workspace"):
            CC.class_sums(a16, a8, CC.DEFAULT_EDGES, workspace=ws)
    for bad in (np.zeros((0, 4), dtype=np.int64), [(0, 0, 16, 0)], [(120, 0, 16, 16)], [(0, 60, 16, 16)], [(-1, 0, 16, 16)], [(0, 0, 16)]):
        with pytest.raises(ValueError, match="pair_sums"):               # an empty pos, and host windows outside the raster
            CC.pair_sums(a16, a8, bad)
        with pytest.raises(ValueError, match="pair_sums"):
            CC.cell_errors(a16, a8, bad, a8)
    for block in (0, -4, 2.5, None, True):
        with pytest.raises(ValueError, match="block"):
            CC.block_errors(a16, a8, block)


# ---- the oracle is not blind --------------------------------------------------------------------------------------------------------------------
def test_each_mistaken_rule_changes_the_oracle_on_the_gpu_tests_inputs():
    p, r, m = CO.triple(np.uint16, np.uint16, np.uint8)
    pos = CO.edge_windows(CO.H0, CO.W0)
    right = CO.pair_sums(p, r, pos, m)
    for mistake in ("r_minus_p", "no_abs", "mask_on_count"):
        assert not np.array_equal(CO.pair_sums(p, r, pos, m, mistake=mistake), right), mistake
    tp, tr, tm, tpos = CO.threshold_case()
    for mask in (None, tm):
        assert not np.array_equal(CO.pair_sums(tp, tr, tpos, mask, "both", 0, 0, 0, mistake="or_in_both"), CO.pair_sums(tp, tr, tpos, mask, "both"))
    assert not np.array_equal(CO.pair_sums(p, r, pos, m, "both", mistake="or_in_both"), CO.pair_sums(p, r, pos, m, "both"))
    for name in ("131x70", "300x300", "7x9"):
        cp, cr, cb = CO.class_case(name)
        for build in (None, cb):
            rows, bad = CO.class_sums(cp, cr, CO.CLASS_EDGES[7], build)
            for mistake in ("gt_at_edge", "cm_transposed", "r_minus_p", "no_abs"):
                wrong, _ = CO.class_sums(cp, cr, CO.CLASS_EDGES[7], build, mistake=mistake)
                assert not np.array_equal(wrong, rows), (name, mistake)
    assert set(CO.MISTAKES) == {"r_minus_p", "no_abs", "gt_at_edge", "cm_transposed", "or_in_both", "mask_on_count"}
