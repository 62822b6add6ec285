"""Polygon zones in Python integers and numpy, one zone and one pixel row at a time: what srbh_zone_sums and srbh_zone_hist must return.
A helper of tests/test_city_zones_cpu.py and tests/test_gpu_city_zones.py, not a test.  Written from the definition include/srbh.h
states, not from the kernel; pinned itself against a fractions.Fraction crossing count, pixel by pixel, in the CPU test.  The sums are
tests/city_summary_oracle.py's over the zone's mask.  GDAL cannot be run where this project is built: no result of it is compared.

The definition: vertices X = round_half_even(256 p); with cy = 256 y + 128, cx = 256 x + 128 an edge crosses row y when min(Y0, Y1) <= cy
< max(Y0, Y1), at xc = X0 + (cy - Y0)(X1 - X0) / (Y1 - Y0); pixel (x, y) is in the zone iff the number of crossing edges with xc > cx is
odd.  ``rule`` names a MISTAKE for the tests that show the comparison is not blind: 'closed' (min <= cy <= max), 'ge' (xc >= cx),
'corner' (the centre taken at the pixel's corner: cy = 256 y, cx = 256 x)."""
from fractions import Fraction

import numpy as np

from tests import city_summary_oracle as SO


def quantise(p):
    """round_half_even(256 p) of a float, as a Python integer (256 * p is exact; round() of a float rounds half to even)"""
    return int(round(256.0 * float(p)))


def zone_edge_list(zone, geotransform=None):
    """the edges (X0, Y0, X1, Y1) of every ring of the zone, closing segments included, horizontal ones dropped; rings with fewer than 3
    distinct quantised vertices give none"""
    edges = []
    for ring in zone:
        pts = [(float(x), float(y)) for x, y in np.asarray(ring, dtype=np.float64).reshape(-1, 2).tolist()]
        if geotransform is not None:
            x0, dx, _, y0, _, dy = geotransform
            pts = [((x - x0) / dx, (y - y0) / dy) for x, y in pts]
        q = [(quantise(x), quantise(y)) for x, y in pts]
        if len(set(q)) < 3:
            continue
        for a, b in zip(q, q[1:] + q[:1]):
            if a[1] != b[1]:
                edges.append((a[0], a[1], b[0], b[1]))
    return edges


def row_mask(edges, y, W, rule=None):
    """the in-zone pixels of row y, columns 0 .. W - 1: each crossing toggles the pixels x < t, t = ceil((N - 128 den) / (256 den))"""
    half = 0 if rule == "corner" else 128
    cy = 256 * y + half
    row = np.zeros(W, dtype=bool)
    xs = np.arange(W)
    for X0, Y0, X1, Y1 in edges:
        lo, hi = min(Y0, Y1), max(Y0, Y1)
        if not (lo <= cy <= hi if rule == "closed" else lo <= cy < hi):
            continue
        if Y0 > Y1:
            X0, Y0, X1, Y1 = X1, Y1, X0, Y0
        den = Y1 - Y0
        num = X0 * den + (cy - Y0) * (X1 - X0) - half * den            # xc > cx  <=>  256 x den < num
        t = num // (256 * den) + 1 if rule == "ge" else -((-num) // (256 * den))
        row ^= xs < t
    return row


def zone_mask(edges, H, W, rule=None):
    """(H, W) bool: the zone's pixels inside the raster"""
    m = np.zeros((H, W), dtype=bool)
    if edges:
        ys = [e[1] for e in edges] + [e[3] for e in edges]
        for y in range(max(0, (min(ys) >> 8) - 1), min(H, (max(ys) >> 8) + 2)):
            m[y] = row_mask(edges, y, W, rule)
    return m


def fraction_mask(edges, H, W):
    """the definition itself, pixel by pixel, in Fractions -> ((H, W) bool, how many (pixel, edge) pairs had the centre exactly ON the
    edge's crossing point, how many had the scanline through a vertex)"""
    m = np.zeros((H, W), dtype=bool)
    on_edge = on_vertex = 0
    for y in range(H):
        cy = Fraction(2 * y + 1, 2) * 256
        for x in range(W):
            cx = Fraction(2 * x + 1, 2) * 256
            n = 0
            for X0, Y0, X1, Y1 in edges:
                on_vertex += cy in (Y0, Y1)
                if min(Y0, Y1) <= cy < max(Y0, Y1):
                    xc = X0 + (cy - Y0) * Fraction(X1 - X0, Y1 - Y0)
                    on_edge += xc == cx
                    n += xc > cx
            m[y, x] = n % 2 == 1
    return m, on_edge, on_vertex


def masks(polygons, H, W, rule=None, geotransform=None):
    return [zone_mask(zone_edge_list(z, geotransform), H, W, rule) for z in polygons]


def _values(value, mask, zm, vthr, mthr):
    v = value[zm].astype(np.int64)
    sel = v > vthr
    if mask is not None:
        sel &= mask[zm].astype(np.int64) > mthr
    return v, sel


def zone_sums(value, polygons, mask=None, vthr=0, mthr=0, rule=None):
    """(Z, 5) int64 [count, n, sum, sumsq, max]"""
    H, W = value.shape
    return np.array([SO._five(*_values(value, mask, zm, vthr, mthr)) for zm in masks(polygons, H, W, rule)], dtype=np.int64).reshape(-1, 5)


def zone_hist(value, polygons, bin_width=1, nbins=256, mask=None, vthr=0, mthr=0):
    H, W = value.shape
    rows = []
    for zm in masks(polygons, H, W):
        v, sel = _values(value, mask, zm, vthr, mthr)
        rows.append(np.bincount(SO.bin_index(v[sel], bin_width, nbins), minlength=nbins))
    return np.array(rows, dtype=np.int64).reshape(-1, nbins)


def urban_centre_table(height, build, polygons, bin_width=10, nbins=256, num_class=7):
    out = SO.heights(zone_sums(height, polygons, build))
    out["hist"] = zone_hist(height, polygons, bin_width, nbins, build)
    out["class_counts"] = None if build is None else zone_hist(build, polygons, 1, num_class, None, -1)
    return out


# ---- the zones of the GPU test (here, so that the CPU test can show that no mistaken rule passes them) ---------------------------------------
H0, W0 = 70, 131


def ring(*pts):
    return np.array(pts, dtype=np.float64).reshape(-1, 2)


def rect(x0, y0, x1, y1):
    return ring((x0, y0), (x1, y0), (x1, y1), (x0, y1))


def fan(H=H0, W=W0):
    """8 triangles that tile [0, W] x [0, H] from the interior vertex (60.5, 30.5): the edges to (60.5, H), (0, 30.5), (W, 30.5) and
    (30, 0) run through pixel centres"""
    c = (60.5, 30.5)
    b = [(0, 0), (30, 0), (W, 0), (W, 30.5), (W, H), (60.5, H), (0, H), (0, 30.5)]
    return [[ring(c, b[i], b[(i + 1) % 8])] for i in range(8)]


def rule_zones():
    """name -> zone: the half-open rule and even-odd"""
    circle = ring(*[(65 + 30 * np.cos(2 * np.pi * k / 1000), 35 + 30 * np.sin(2 * np.pi * k / 1000)) for k in range(1000)])
    return {
        "rectangle on centres": [rect(10.5, 5.5, 40.5, 20.5)],
        "diamond through centres": [ring((60.5, 10.5), (70.5, 20.5), (60.5, 30.5), (50.5, 20.5))],
        "triangle with a vertex on a centre": [ring((20.5, 30.5), (35, 50), (5.25, 45.75))],
        "local maximum and passing vertex on scanlines": [ring((70, 60), (72, 50.5), (75, 40.5), (80, 50.5), (85, 40.5), (90, 60))],
        "U": [ring((95, 5), (100, 5), (100, 25), (110, 25), (110, 5), (115, 5), (115, 30), (95, 30))],
        "hole": [rect(5, 50, 45, 68), rect(15.3, 55.2, 30.7, 62.9)],
        "hole touching the exterior": [rect(100, 35, 128, 65), ring((100, 45), (110, 40), (110, 55))],
        "two disjoint parts": [rect(2, 2, 8, 9), ring((120, 2), (129.5, 4), (125, 12.5))],
        "two overlapping parts": [rect(45, 40, 60, 55), rect(52.5, 47.5, 68, 62)],
        "bow-tie": [ring((20, 22), (50, 36), (50, 22), (20, 36))],
        "1000-gon": [circle],
        "empty": [],
        "3 edges": [ring((3.2, 12.1), (9.9, 30.4), (1.1, 44.8))],
        "degenerate ring only": [ring((5, 5), (9, 9))],
    }


def clip_zones(H=H0, W=W0):
    big = float(2 ** 21)
    return {
        "left": [rect(-20.3, 10.2, 12.6, 30.1)], "right": [rect(W - 9.4, 20, W + 50, 44.4)], "top": [ring((30, -15), (60, -4), (45, 17.5))],
        "bottom": [ring((70, H + 30), (90.5, H - 10.5), (110, H + 3))], "corner": [rect(W - 3.5, H - 2.5, W + 7, H + 7)],
        "wholly left": [rect(-50, 5, -0.6, 40)], "wholly below": [rect(5, H + 0.5, 90, H + 40)], "wholly right": [rect(W + 0.5, -5, W + 9, 9)],
        "triangle at the limit": [ring((-big, -big), (big, -big), (0, big))],
        "sliver without a centre": [rect(10.6, 3, 10.9, 60)], "sliver with one column": [rect(10.4, 3, 10.6, 60)],
        "everything": [rect(0, 0, W, H)], "beyond everything": [rect(-1000, -1000, W + 1000, H + 1000)],
    }


def small_zones(n, H=H0, W=W0, seed=3):
    """n small random triangles and quadrilaterals on the 1/256, 1/2 and integer grids, some reaching outside"""
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        k = 3 + i % 2
        c = np.array([rs.uniform(-3, W + 3), rs.uniform(-3, H + 3)])
        pts = c + rs.uniform(-9, 9, size=(k, 2))
        grid = (256.0, 2.0, 1.0)[i % 3]
        out.append([np.round(pts * grid) / grid])
    return out
