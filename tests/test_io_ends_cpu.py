"""CPU twin of tests/test_gpu_mosaic_forms.py and tests/test_gpu_loader_forms.py: pins tests/io_ends_oracle.py against the literal oracles of
the reference's lines (oracle/mosaic_oracle.py, oracle/loader_oracle.py) and the reference's own fixtures (g12_mosaic.npz, g13_loader.npz),
and proves by arithmetic that the case tables reach the forms the GPU files claim: margins empty after the redraw, wraps that wrap, ties
that tie, ragged last workgroups, a second grid-stride trip."""
import numpy as np
import pytest
import torch

from oracle import loader_oracle as LO
from oracle.mosaic_oracle import MosaicOracle, synthetic_city
from tests import io_ends_oracle as O

HIR = O.HIR256


def _stock_quanta(z):
    """stock fp32 torch.softmax, quantised as the reference does (predict...py:176-177)"""
    p = torch.softmax(torch.from_numpy(np.array(z, dtype=np.float32)), dim=-1).numpy()
    assert p.dtype == np.float32
    return np.round(p * 255).astype(np.int64)


def _scatter_any(flag, pos, H, W):
    """(H, W) bool: the mosaic pixels that receive a tile pixel whose flag is set"""
    out = np.zeros((H, W), dtype=bool)
    B, th, tw = flag.shape
    f = flag & O.added_mask(pos, th, tw, H, W)
    for b in range(B):
        ys, xs = np.nonzero(f[b])
        out[ys + int(pos[b][1]), xs + int(pos[b][0])] = True
    return out


# ---- the mosaic oracle against the reference's lines and fixture ---------------------------------------------------------------------------
def _city():
    ypred, logits, pos, lr_w, lr_h = synthetic_city()
    H, W = lr_h * 4, lr_w * 4
    z = logits.permute(0, 2, 3, 1).contiguous().numpy()
    acc = O.mosaic_accumulate(ypred[:, 0].numpy(), z, pos.numpy() * 4, H, W)
    dirty = _scatter_any((acc.margin < O.delta(7)).any(axis=-1), pos.numpy() * 4, H, W)
    return ypred, logits, pos, H, W, z, acc, dirty


def test_oracle_reproduces_the_reference_lines_on_the_synthetic_city():
    ypred, logits, pos, H, W, z, acc, dirty = _city()
    ora = MosaicOracle(H, W, 7)
    ora.add(ypred, logits, pos.tolist())
    assert np.array_equal((acc.res_h & 0xFFFF).astype(np.uint16), ora.res_height)
    assert np.array_equal((acc.res_w & 0xFF).astype(np.uint8), ora.res_weight)
    q, margin = O.class_quanta(z)
    ok = margin >= O.delta(7)
    assert np.array_equal(q[ok], _stock_quanta(z)[ok])                       # entry by entry wherever the margin rule holds
    clean = ~dirty
    assert np.array_equal((acc.res_b & 0xFFFF).astype(np.uint16)[:, clean], ora.res_build[:, clean])
    want_h, want_b = ora.finalize()
    got_h, got_b = O.mosaic_finalize(acc.res_h, acc.res_b, acc.res_w, 7)
    assert np.array_equal(got_h, want_h)
    assert np.array_equal(got_b[clean], want_b[clean])
    assert dirty.mean() < 0.01


def test_oracle_reproduces_the_reference_fixture():
    """g12_mosaic.npz: what the reference's own predict_whole_image_grid wrote.  Heights exact; the class map exact wherever every entry that
    reaches the pixel has margin >= delta -- measured: that leaves out 54 of 7 680 pixels (0.70 %), and the map is in fact equal there too"""
    g = O.golden("g12_mosaic.npz")
    ypred, logits, pos, H, W, z, acc, dirty = _city()
    assert np.array_equal(pos.numpy(), g["pos"]) and (H, W) == (int(g["lr_h"]) * 4, int(g["lr_w"]) * 4)
    got_h, got_b = O.mosaic_finalize(acc.res_h, acc.res_b, acc.res_w, 7)
    assert np.array_equal(got_h, g["height"])
    print(f"IOENDS g12: {int(dirty.sum())} of {dirty.size} pixels have an entry inside delta; class map differs at "
          f"{int((got_b != g['build']).sum())}")
    assert np.array_equal(got_b[~dirty], g["build"][~dirty])
    assert dirty.mean() < 0.01


def test_finalize_oracle_known_answers():
    hw = np.array(O.FIN_HW, dtype=np.uint32)
    h, b = O.mosaic_finalize(hw[:, 0][None], np.zeros((1, 1, len(hw)), np.uint32), hw[:, 1][None], 1)
    assert h[0].tolist() == list(O.FIN_HW_WANT) and not b.any()
    # the issue's table: h / 2 half to even
    assert [O.FIN_HW_WANT[O.FIN_HW.index((v, 2))] for v in (1, 3, 5, 7, 65535)] == [0, 2, 2, 4, 32768]
    # high bits never reach an output
    h2, _ = O.mosaic_finalize(hw[:, 0][None] + np.uint32(0x70000), np.zeros((1, 1, len(hw)), np.uint32), hw[:, 1][None] + np.uint32(0x5200), 1)
    assert np.array_equal(h, h2)
    # first maximum, on the masked sums
    rb = np.array([[5], [0x10005], [0x20004], [5]], dtype=np.uint32).reshape(4, 1, 1)
    assert O.mosaic_finalize(np.zeros((1, 1), np.uint32), rb, np.ones((1, 1), np.uint32), 4)[1][0, 0] == 0


def test_height_quanta_known_answers():
    q = O.height_quanta(np.array([-0.0, -3.0, 0.05, 0.15, 0.25, 12.25, 12.35, 2000.0, 6553.5], dtype=np.float32))
    # fl32(0.05 * 10) = 0.5 -> 0 and fl32(0.25 * 10) = 2.5 -> 2 (even floors stay); fl32(0.15 * 10) = 1.5 -> 2, fl32(12.35 * 10) = 123.5 -> 124
    assert q.tolist() == [0, 0, 0, 2, 2, 122, 124, 20000, 65535]


# ---- section 2: the redraw leaves inputs with one right answer --------------------------------------------------------------------------------
def _clean_sets():
    sets = [(c.name, O.clean_logits(c.C, c.B, c.th, c.tw)) for c in O.ACC_CASES]
    w = O.WRAPPER
    sets += [(f"wrapper fp16={f}", O.clean_logits(w.C, w.B, w.th, w.tw, fp16=f, key="wrapper")) for f in (False, True)]
    sets += [("wrap_weight", O.clean_logits(2, 300, 4, 4, key="wrap_weight")), ("wrap_height", O.clean_logits(2, 4, 4, 4, key="wrap_height"))]
    sets.append(("wrap_class", O.clean_pixels(300 * 16, 3, "wrap_class", draw=O._draw_dominant)))
    return sets


@pytest.mark.parametrize("name,c", _clean_sets(), ids=[n for n, _ in _clean_sets()])
def test_redraw_empties_the_margin_and_keeps_the_draw(name, c):
    C = c.z.shape[-1]
    q, margin = O.class_quanta(c.z)
    print(f"IOENDS clean {name}: C={C} entries={margin.size} first draw inside delta {c.first_inside} ({c.first_inside / margin.size:.2e}), "
          f"rounds {c.rounds}, pixels redrawn {c.redrawn}")
    assert c.rounds <= 8 and float(margin.min()) >= O.delta(C)
    assert np.array_equal(_stock_quanta(c.z), q), "stock fp32 softmax misses the zero-mismatch cap on its own"
    assert np.array_equal(O.class_quanta_fp32(c.z), q)
    assert c.redrawn < 0.01 * (c.z.size // C)
    if C == 1:
        assert (q == 255).all()
    if "fp16=True" in name:
        assert np.array_equal(torch.from_numpy(c.z.copy()).half().float().numpy(), c.z)      # the half tensor holds exactly these values


def test_delta_covers_the_derived_error_for_every_class_count():
    for C in range(1, 21):
        assert O.delta(C) >= 255 * (C + 9) * O.EPS32


@pytest.mark.parametrize("C", [7, 16])
@pytest.mark.parametrize("big_first", [True, False])
def test_order_case_is_what_its_docstring_says(C, big_first):
    z, want = O.order_case(C, big_first)
    q64, margin = O.class_quanta(z)
    assert q64.max() == 127 and margin.min() < O.delta(C)                   # inside the margin: the float64 oracle is not the answer here
    t = np.exp(np.float32(-17))
    assert t.dtype == np.float32 and 0 < t < 2.0 ** -23 and (C - 2) * float(t) > 1.5 * 2.0 ** -23
    assert np.array_equal(O.class_quanta_fp32(z), want)                      # class order 0 .. C - 1 in fp32
    assert np.array_equal(O.class_quanta_fp32(z[::-1])[::-1], O.order_case(C, not big_first)[1][::-1])    # descending: the other answer
    assert not np.array_equal(O.class_quanta_fp32(z[::-1])[::-1], want)


# ---- section 3: the accumulate table reaches its forms --------------------------------------------------------------------------------------
def test_accumulate_cases_reach_their_forms():
    totals = {c.name: c.B * c.th * c.tw for c in O.ACC_CASES}
    assert any(t < 256 for t in totals.values())
    assert any(t > 256 and 0 < t % 256 <= 32 for t in totals.values()), "no ragged last workgroup just above a multiple of 256"
    assert sum(t > 4 * 256 for t in totals.values()) >= 3
    assert {c.C for c in O.ACC_CASES} == {1, 2, 7, 15, 16}
    assert {(c.th, c.tw) for c in O.ACC_CASES} == {(4, 4), (8, 20), (12, 8), (64, 64)}
    H, W = O.CITY_H, O.CITY_W
    seen, tie_even, tie_odd, neg, negzero, top, overlap = set(), 0, 0, 0, 0, 0, 0
    for ci, c in enumerate(O.ACC_CASES):
        inp = O.acc_inputs(c)
        assert np.abs(inp.pos[:, :2]).max() <= max(H, W) + 2 * max(c.th, c.tw)           # offsets within a few tiles of the city
        added = O.added_mask(inp.pos, c.th, c.tw, H, W)
        for b in range(c.B):
            kind = O.WINDOW_KINDS[(ci * 5 + b) % len(O.WINDOW_KINDS)]
            n, full = int(added[b].sum()), min(c.th, H) * min(c.tw, W)
            xoff, yoff, xc, yc = inp.pos[b]
            if kind in ("out_left", "out_top", "out_right", "out_bottom", "xcount0", "count_negative"):
                assert n == 0
            elif kind == "count1":
                assert n == 1
            elif kind.startswith("hang") or kind == "cropped":
                assert 0 < n < c.th * c.tw
            elif kind == "count_over":
                assert xc > c.tw and yc > c.th and n == (min(yoff + c.th, H) - yoff) * (min(xoff + c.tw, W) - xoff)
            elif c.th <= H and c.tw <= W:
                assert n == c.th * c.tw == full
            seen.add(kind)
        overlap += int((inp.want.res_w.astype(np.int64) - inp.state[2]).max() >= 2)               # overlapping windows
        assert all(int(s.min()) >= 0 and int(s.max()) < 1 << 15 and int(s.max()) > 0 for s in inp.state)
        t = np.where(inp.height < 0, np.float32(0), inp.height) * np.float32(10)
        fl = np.floor(t)
        tie = added & (t - fl == 0.5)
        tie_even += int((tie & (fl % 2 == 0)).sum())
        tie_odd += int((tie & (fl % 2 == 1)).sum())
        neg += int((added & (inp.height < 0)).sum())
        negzero += int((added & (inp.height == 0) & np.signbit(inp.height)).sum())
        top += int((added & (inp.height == np.float32(6553.5))).sum())
        assert float(inp.height.max()) <= 6553.5
    assert seen == set(O.WINDOW_KINDS) and overlap >= 5
    assert min(tie_even, tie_odd, neg, negzero, top) > 0, (tie_even, tie_odd, neg, negzero, top)


def test_wrap_cases_wrap():
    H, W = O.CITY_H, O.CITY_W
    w = O.wrap_inputs("weight").want
    assert int(w.res_w.max()) == 300 and int(w.res_w[w.res_w > 0].min()) == 256
    zero_w = (w.res_w & 0xFF) == 0
    assert (zero_w & ((w.res_h & 0xFFFF) != 0)).any(), "no pixel with w8 == 0 and a non-zero height sum"
    fh, _ = O.mosaic_finalize(w.res_h, w.res_b, w.res_w, 2)
    sel = zero_w & (w.res_w > 0)
    assert np.array_equal(fh[sel], (w.res_h & 0xFFFF).astype(np.uint16)[sel])          # left undivided
    h = O.wrap_inputs("height").want
    assert int(h.res_h.max()) == 80000 > 65535
    c = O.wrap_inputs("class").want
    covered = c.res_w > 0
    assert int(c.res_b[0][covered].min()) > 65535
    raw, masked = np.argmax(c.res_b, axis=0), O.mosaic_finalize(c.res_h, c.res_b, c.res_w, 3)[1]
    assert (raw[covered] == 0).all() and (masked[covered] == 1).all()                  # on the wrapped sums another class wins
    assert covered.sum() == 16 and (H, W) == c.res_w.shape


def test_finalize_cases_reach_their_forms():
    assert [h * w for h, w in O.FIN_SHAPES] == [1, 255, 256, 257, 1000] and O.FIN_C == (1, 2, 7, 16, 20)
    for C in O.FIN_C:
        res_h, res_b, res_w = O.finalize_inputs(C, 25, 40)
        assert int(res_h.min()) >= 0x10000 or (res_h >> 16).any()
        assert (res_h >> 16).any() and (res_b >> 16).any() and (res_w >> 9).any()
        fh, fb = O.mosaic_finalize(res_h, res_b, res_w, C)
        # dropping a mask changes the result: the high bits matter to a kernel that forgets one
        assert not np.array_equal(np.argmax(res_b, axis=0), fb) or C == 1
        w8, h16 = res_w & 0xFF, res_h & 0xFFFF
        assert ((w8 == 0) & (h16 != 0) & ((res_w & 0x100) != 0)).any() and ((w8 == 0) & (h16 != 0) & ((res_w & 0x100) == 0)).any()
        assert {1, 2, 3, 255} <= set(np.unique(w8).tolist())
        q = h16[w8 > 0].astype(np.float64) / w8[w8 > 0]
        ties = q - np.floor(q) == 0.5
        assert (ties & (np.floor(q) % 2 == 0)).any() and (ties & (np.floor(q) % 2 == 1)).any()
        if C > 1:
            b16 = (res_b & 0xFFFF).reshape(C, -1)
            top = b16.max(axis=0)
            nmax = (b16 == top).sum(axis=0)
            assert (nmax == C).any() and ((nmax == 2) & (b16[-1] == top)).any() and ((nmax == 1) & (b16[-1] == top)).any()
            assert (nmax > 1).mean() > 0.2
            raw = res_b.reshape(C, -1).astype(np.int64)
            assert ((nmax > 1) & ((raw == raw.max(axis=0)).sum(axis=0) == 1)).any()         # a tie that exists only after the mask


# ---- section 4: the loader tables ------------------------------------------------------------------------------------------------------------
def test_label_prep_cases_reach_their_forms():
    assert O.PREP_SHAPES[2][1] % 8 and O.PREP_SHAPES[2][2] % 8 and not (O.PREP_SHAPES[2][1] % 4 or O.PREP_SHAPES[2][2] % 4)
    B, H, W = O.PREP_SHAPES[3]
    cells = B * H * W // 16
    assert cells == 1360 and cells > 256 and cells % 256
    assert all(s[0] * s[1] * s[2] // 16 < 256 for s in O.PREP_SHAPES[:3])
    for shape in O.PREP_SHAPES[1:]:
        lab = O.prep_labels(shape)
        if shape[1] * shape[2] >= 256:
            assert np.unique(lab).size == 256
        assert (lab[-1] == 255).all()
        s = lab.reshape(shape[0], shape[1] // 4, 4, shape[2] // 4, 4).sum(axis=(2, 4))
        assert (s % 16 == 0).any() and (s % 16 == 15).any()
        # one below a multiple of 16 AT a class edge: truncation and rounding of the mean give different classes
        lut = LO.buildhir_lut(HIR)
        below = s[s % 16 == 15]
        assert (lut[below // 16] != lut[np.minimum((below + 8) // 16, 255)]).any()
    assert (O.prep_labels((1, 4, 4), "all255") == 255).all() and O.prep_labels((1, 4, 4), "one_below").sum() % 16 == 15
    assert LO.buildhir_lut(O.HIR255)[255] == 0 and LO.buildhir_lut(O.HIR256)[255] == 6
    cw = O.CLASS_WEIGHTS
    assert (cw < 0).any() and not np.array_equal(torch.from_numpy(cw).bfloat16().float().numpy(), cw)
    assert np.isfinite(cw).all() and len(cw) == len(HIR) - 1


def test_label_prep_wrapper_equals_the_oracle_and_the_reference_fixture():
    g = O.golden("g13_loader.npz")
    b, hf, w, ha, wa = O.label_prep(g["height_u8"], HIR, g["heightweight"])
    for i in range(g["height_u8"].shape[0]):
        ohf, oha, ob, ow, owa = LO.label_prep(g["height_u8"][i], HIR, g["heightweight"].astype(np.float32))
        assert torch.equal(hf[i], ohf) and torch.equal(b[i], ob) and torch.equal(w[i], ow)
        assert torch.equal(ha[i], oha.reshape(ha[i].shape)) and torch.equal(wa[i], owa.reshape(wa[i].shape))
        assert np.array_equal(ha[i].numpy(), g[f"height_aggre{i}"].reshape(ha[i].shape)) and np.array_equal(b[i].numpy(), g[f"build{i}"])
        assert np.array_equal(w[i].numpy(), g[f"weight{i}"]) and np.array_equal(wa[i].numpy(), g[f"weight_aggre{i}"].reshape(wa[i].shape))


def test_height_aggre_is_exact():
    """a cell's sum is an integer <= 4080 and fl32(16 + 1e-10) is 16: the mean is the exact quotient, (long) of it the floor"""
    assert np.float32(16) + np.float32(1e-10) == np.float32(16)
    for shape in O.PREP_SHAPES:
        lab = O.prep_labels(shape)
        ha = O.label_prep(lab, HIR, O.CLASS_WEIGHTS)[3].numpy()
        s = lab.reshape(shape[0], shape[1] // 4, 4, shape[2] // 4, 4).astype(np.int64).sum(axis=(2, 4))
        assert np.array_equal(ha.astype(np.float64) * 16, s.astype(np.float64))


def test_normalize_wrapper_equals_the_oracle_on_the_reference_fixture():
    g = O.golden("g13_loader.npz")
    raw = np.ascontiguousarray(np.concatenate([g["s2"], g["s1"]], axis=-1).transpose(0, 3, 1, 2)).astype(np.float32)
    mins = g["mins"].astype(np.float32)
    ranges = (g["maxs"] - g["mins"]).astype(np.float32)
    got = O.normalize(raw, mins, ranges, (0, 1))
    for i in range(raw.shape[0]):
        want = LO.normalize(torch.from_numpy(raw[i]), g["mins"], g["maxs"], (0, 1))
        assert np.array_equal(O.bits(got[i]), O.bits(want))


def test_normalize_cases_reach_their_forms():
    B, C, H, W = O.NORM_SHAPES[3]
    n = B * C * H * W
    assert n == 1_080_000 and n > O.NORM_GRID_CAP and n % 256 != 0
    assert O.NORM_SHAPES[0][2] * O.NORM_SHAPES[0][3] == 1
    f = np.float32
    for shape in O.NORM_SHAPES:
        for clamp in O.NORM_CLAMPS:
            x, mins, ranges = O.norm_inputs(shape, clamp)
            out = O.normalize(x, mins, ranges, clamp).numpy()
            assert np.isnan(out).any() and np.isnan(x).any()                  # NaN stays NaN, clip or not
            if shape[1] == 1 or shape[2] * shape[3] < 60:          # a lone general band; 15 elements hold 15 specials, not every one in band 0
                continue
            assert ranges[1] == 0 and mins[0] == 0 and ranges[0] == 1
            b0, ob = O.bits(x[:, 0]), O.bits(out[:, 0])
            lo, hi = clamp if clamp else (0.0, 1.0)
            inf = f(np.inf)
            for v in (f(lo), f(hi), np.nextafter(f(lo), inf), np.nextafter(f(lo), -inf), np.nextafter(f(hi), inf), np.nextafter(f(hi), -inf)):
                assert (b0 == v.view(np.int32)).any(), (shape, clamp, v)
            assert (ob == f(lo).view(np.int32)).any() and (ob == f(hi).view(np.int32)).any()
            assert (ob == np.nextafter(f(lo), inf).view(np.int32)).any() and (ob == np.nextafter(f(hi), -inf).view(np.int32)).any()
            negzero = f(-0.0).view(np.int32)
            assert (b0 == negzero).any()
            if clamp is None or lo <= 0:
                assert (ob == negzero).any()                                       # -0.0 is not below lo = 0: it stays
            if clamp is None or (lo <= 0 and hi >= 1):
                sub = np.abs(out[:, 0])
                assert ((sub > 0) & (sub < np.finfo(np.float32).tiny)).any()           # a subnormal result
            o1 = out[:, 1]
            assert np.isnan(o1).any()
            if clamp:
                assert set(np.unique(o1[~np.isnan(o1)]).tolist()) == {lo, hi}          # +-inf of the zero range, clipped
                assert np.isfinite(out[~np.isnan(out)]).all()
            else:
                assert np.isposinf(o1).any() and np.isneginf(o1).any()
    # the second grid-stride trip holds specials of its own
    x, _, _ = O.norm_inputs(O.NORM_SHAPES[3], (0.0, 1.0))
    tail = x.reshape(-1)[O.NORM_GRID_CAP:]
    assert np.isnan(tail).any() and np.isinf(tail).any() and tail.size == n - O.NORM_GRID_CAP
