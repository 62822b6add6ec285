"""The SR trunk's training kernels ("fast" mode of rrdbnet_autograd.py: the 69 dense blocks of SR/rrdbnet_arch.py:136-167 forward and backward)
against the float64 oracle of tests/trunk_train_oracle.py, layer by layer from the planes the kernels leave behind:

  srbh_trunk_wgrad, called directly on synthetic rows   exact (integer operands, impulses, roundings of the saved planes) and bounded (random)
  the persistent backward (bf16 form of the trunk kernel) every g4..g1 plane, every g5 plane, the input gradient, dw_all / db_all
  the persistent training forward (fp16 form)           every x1..x4 plane, planes 0..1 of every next buffer, the fp32 output
  the per-layer fallback                                 at a geometry the persistent kernel does not take (12 x 48)

Each stored plane was computed from stored planes, so each layer is compared with float64 of the SAME rounded operands under
    |error| <= K 2^-23 sum|a||b|   (+ half an ulp of the 16-bit format where the value is stored in 16 bits; streams: the sum over their convs),
every element, nothing sampled.  The exact cases compare with torch.equal.  Half an ulp of bf16 is taken exactly, 2^(floor(log2 |ref|) - 8): between
2^-9 |ref| and 2^-8 |ref| (2^-9 |ref| alone is no bound of a correct rounding: 1 + 2^-8 goes to 1), 2^-134 below 2^-126 -- an impulse's gradient
tails off into bf16's subnormals, which the kernels keep -- and every fp32 sum carries fp32's own underflow floor, 2^-149 per term.

Largest error / bound seen on an MI355X (a plane stored in 16 bits comes close to 1 by construction: its rounding reaches half an ulp):
  srbh_trunk_wgrad, random operands      dw_all 5.0e-4 (1, 8), 9.5e-5 (3, 8); db_all 1.2e-4, 2.7e-5
  persistent forward                     x1..x4 0.60, fp16 of the stream 0.96, fp32 output 6.5e-3
  persistent backward                    g4..g1 0.93, g5 0.995, input gradient 1.1e-2, dw_all 7.9e-4, db_all 1.5e-4
  persistent backward, corner impulse    g4..g1 0.98, g5 0.99, input gradient 1.5e-2, dw_all 1.5e-3, db_all 9.4e-4
  per-layer fallback at 12 x 48          forward x1..x4 0.55 / stream 0.95 / output 6.2e-3; g4..g1 0.89, dw_all 8.2e-4, db_all 1.3e-4,
                                         g5 of RDB 0 0.99, input gradient 0.99 (both through a g5 plane known to half a bf16 ulp)
No kernel was found wrong.  What a mistake of a given kind is caught by: tests/test_trunk_train_oracle_cpu.py plants a tap shifted by one column
(6.5e3 x the bound), a weight slice from the neighbouring plane (1.8e3 x) and a bias sum without the last tile (1.9e3 x) into the oracle.

Not covered: SRBH_TWG_SPLITS other than 4, batch sizes that need two persistent launches, the mixed and f32 modes."""
import ctypes as C
import functools

import pytest
import torch

from srbh_amd import _lib
from tests import gpu_util as G
from tests import trunk_train_oracle as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _randint(shape, seed, lo, hi):
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _rand(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


# ---- a. srbh_trunk_wgrad on synthetic rows -------------------------------------------------------------------------------------------------------
def _stride(B, H, W=64):
    n = _lib.lib().srbh_act16_bytes(B, 192, H, W)
    return n, (n + 255) // 256 * 256          # (as rrdbnet_autograd._fast_buffers places its buffers)


def _row(values, bf16):
    """values (n_buf, B, 192, H, 64) fp32 -> a row of zero-bordered ACT16 buffers of six planes (fp16, or bf16), buffer k at k * stride; whatever
    lies between two buffers holds 0xFFFF (a NaN in either format)"""
    n_buf, B, _, H, W = values.shape
    n, nb = _stride(B, H, W)
    row = torch.full((n_buf * nb,), 0xFF, dtype=torch.uint8, device=DEV)
    for k in range(n_buf):
        row[k * nb:k * nb + n].zero_()
        G.act16_from_nchw_x16(values[k].to(DEV), bf16=bf16, chunks_total=6, buf=row[k * nb:(k + 1) * nb])
        stored = G.act16_planes(row[k * nb:(k + 1) * nb], B, 6, H, W, torch.bfloat16 if bf16 else torch.float16).cpu()
        want = values[k].to(torch.bfloat16 if bf16 else torch.float16)
        assert torch.equal(stored.view(torch.int16), want.view(torch.int16)), "the synthetic planes are not the bits asked for"
    return row, nb


def _call_wgrad(num_block, drow, grow, nb, B, H, W=64):
    """one call with a NaN-filled workspace and NaN-filled outputs (whatever is left unwritten, or added to, stays NaN)"""
    L = _lib.lib()
    nws = L.srbh_trunk_wgrad_ws_bytes(num_block, B, H, W)
    ws = torch.full((max(nws // 4, 64),), NAN, dtype=torch.float32, device=DEV)
    dw = torch.full((num_block * 3 * T.DW_RDB,), NAN, dtype=torch.float32, device=DEV)
    db = torch.full((num_block * 3 * T.DB_RDB,), NAN, dtype=torch.float32, device=DEV)
    rc = L.srbh_trunk_wgrad(num_block, drow.data_ptr(), nb, grow.data_ptr(), nb, B, H, W, dw.data_ptr(), db.data_ptr(), ws.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, dw.cpu(), db.cpu(), ws


def _wgrad_oracle(Dv, Gv, with_scale=False):
    """Dv (n_rdb, ...) in forward order, Gv (n_rdb, ...) in row order (buffer k = RDB n_rdb - 1 - k) -> dw_all, db_all (and their scales)"""
    n_rdb = Dv.shape[0]
    parts = [T.wgrad(T.f16_to_bf16(Dv[i].half()), T.bf16_rne(Gv[n_rdb - 1 - i]), with_scale) for i in range(n_rdb)]
    return tuple(torch.cat([p[j] for p in parts]) for j in range(len(parts[0])))


@pytest.mark.parametrize("num_block", [1, 2])
@pytest.mark.parametrize("B,H", [(1, 8), (3, 8), (5, 8), (1, 16), (2, 24)])
def test_trunk_wgrad_integer_operands_are_exact(B, H, num_block):
    """g from integers in [-2, 2], D from integers in [-4, 4]: exact in bf16 / fp16, every partial sum below 2^24, so fp32 accumulation is exact
    in any order and dw_all / db_all EQUAL the oracle.  Tiles of 4 rows over 4 splits: (1, 8) fewer tiles than splits; (3, 8) six tiles in ranges
    2, 2, 2, 0 -- the empty split's workspace slot must contribute zeros; (5, 8) ranges 3, 3, 3, 1; (1, 16) one tile each; (2, 24) even ranges.
    Every RDB, plane and image holds other data: a swapped RDB order, pair or split shows."""
    n_rdb = 3 * num_block
    assert B * H * 64 * 8 < 2 ** 24
    Dv = _randint((n_rdb, B, 192, H, 64), 1000 + 10 * B + H, -4, 4)
    Gv = _randint((n_rdb, B, 192, H, 64), 2000 + 10 * B + H, -2, 2)
    drow, nb = _row(Dv, 0)
    grow, _ = _row(Gv, 1)
    rc, dw, db, _ = _call_wgrad(num_block, drow, grow, nb, B, H)
    assert rc == 0
    want_dw, want_db = _wgrad_oracle(Dv, Gv)
    assert torch.equal(db.double(), want_db), "db_all"
    assert torch.equal(dw.double(), want_dw), "dw_all"


def _distinct_planes(n_rdb, B, H):
    """another value at every pixel, exact in fp16 AND bf16 (bf16 bit patterns 0x3F80 + p: 1.0 upwards, 128 values per binade), the sign
    alternating over channels and images, each RDB starting at another pixel number"""
    p = torch.arange(H * 64, dtype=torch.int32).view(1, 1, 1, H, 64) + 131 * torch.arange(n_rdb, dtype=torch.int32).view(n_rdb, 1, 1, 1, 1)
    v = (0x3F80 + p).to(torch.int16).view(torch.bfloat16).float()
    assert float(v.max()) < 60000 and torch.equal(v.half().float(), v)
    sign = 1.0 - 2.0 * ((torch.arange(192).view(1, 1, 192, 1, 1) + torch.arange(B).view(1, B, 1, 1, 1)) % 2)
    return (v * sign).contiguous()


@pytest.mark.parametrize("y,x", [(0, 0), (0, 63), (15, 0), (15, 63), (0, 31), (15, 32), (9, 0), (6, 63), (3, 20), (4, 20), (7, 41), (8, 41)])
def test_trunk_wgrad_impulse_picks_the_named_neighbour(y, x):
    """g = 1 at ONE pixel of the second image (all channels), D another value at every pixel: tap (ky, kx) of every block must hold exactly
    D[y + ky - 1][x + kx - 1] of that image, and zero where that neighbour lies outside the image.  Corners, edge middles, and both sides of the
    4-row tile boundaries (rows 3 | 4, 7 | 8)."""
    B, H, n_rdb = 2, 16, 3
    Dv = _distinct_planes(n_rdb, B, H)
    Gv = torch.zeros(n_rdb, B, 192, H, 64)
    Gv[:, 1, :, y, x] = 1.0
    drow, nb = _row(Dv, 0)
    grow, _ = _row(Gv, 1)
    rc, dw, db, _ = _call_wgrad(1, drow, grow, nb, B, H)
    assert rc == 0
    assert torch.equal(db, torch.ones_like(db))
    Dp = torch.nn.functional.pad(Dv, (1, 1, 1, 1))
    for i in range(n_rdb):
        for k, (ch0, cout, cin) in enumerate(T.CONV_GEO):
            got = dw[i * T.DW_RDB + T.DW_OFF[k]:i * T.DW_RDB + T.DW_OFF[k] + cout * cin * 9].view(cout, cin, 3, 3)
            want = Dp[i, 1, :cin, y:y + 3, x:x + 3].expand(cout, cin, 3, 3)          # (padded coordinates: image row y + ky - 1 is padded row y + ky)
            assert torch.equal(got, want), (i, k)
    want_dw, _ = _wgrad_oracle(Dv, Gv)
    assert torch.equal(dw.double(), want_dw)


def test_trunk_wgrad_rounds_the_saved_planes_to_nearest_even():
    """the saved planes are fp16 and the kernel multiplies bf16: with g a single 1.0 each tap IS the rounded neighbour.  Ties under bf16 go to
    even (1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6, and their negatives), 65504 -> 65536, the smallest fp16 subnormal survives, -0.0 adds nothing."""
    B, H, n_rdb, y, x = 1, 8, 3, 4, 30
    vals = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 65504.0, 2.0 ** -24, -0.0, 2.0 ** -14, 1 + 2.0 ** -7]
    want9 = [1.0, 1 + 2.0 ** -6, -1.0, -(1 + 2.0 ** -6), 65536.0, 2.0 ** -24, 0.0, 2.0 ** -14, 1 + 2.0 ** -7]
    Dv = torch.zeros(n_rdb, B, 192, H, 64)
    want = torch.zeros(n_rdb, 192, 3, 3)
    for i in range(n_rdb):
        for c in range(192):
            for t in range(9):
                j = (t + c + i) % 9          # another value under every tap from channel to channel
                Dv[i, 0, c, y - 1 + t // 3, x - 1 + t % 3] = vals[j]
                want[i, c, t // 3, t % 3] = want9[j]
    Gv = torch.zeros(n_rdb, B, 192, H, 64)
    Gv[:, 0, :, y, x] = 1.0
    drow, nb = _row(Dv, 0)          # (asserts that the fp16 bits are the ones asked for: the subnormal and -0.0 included)
    grow, _ = _row(Gv, 1)
    rc, dw, db, _ = _call_wgrad(1, drow, grow, nb, B, H)
    assert rc == 0
    for i in range(n_rdb):
        for k, (ch0, cout, cin) in enumerate(T.CONV_GEO):
            got = dw[i * T.DW_RDB + T.DW_OFF[k]:i * T.DW_RDB + T.DW_OFF[k] + cout * cin * 9].view(cout, cin, 3, 3)
            assert torch.equal(got, want[i, :cin].expand(cout, cin, 3, 3)), (i, k)
    assert torch.equal(dw.double(), _wgrad_oracle(Dv, Gv)[0])


@pytest.mark.parametrize("B,H", [(1, 8), (3, 8)])
def test_trunk_wgrad_random_operands_within_the_bound(B, H):
    """random fp16 planes and bf16 gradients at the two smallest shapes (512 and 1 536 pixels: one dropped term is far above the bound), every
    element within K u sum|g||D|, K = B H W.  Two calls (fresh NaN workspace, fresh NaN outputs) are bit-equal: the splits are added in a fixed order."""
    n_rdb = 3
    Dv = _rand((n_rdb, B, 192, H, 64), 300 + B).half().float()
    Gv = _rand((n_rdb, B, 192, H, 64), 400 + B).to(torch.bfloat16).float()
    drow, nb = _row(Dv, 0)
    grow, _ = _row(Gv, 1)
    rc, dw, db, ws = _call_wgrad(1, drow, grow, nb, B, H)
    assert rc == 0 and bool(torch.isfinite(ws[:_lib.lib().srbh_trunk_wgrad_ws_bytes(1, B, H, 64) // 4]).all()), "a workspace slot the reduce reads was never written"
    want_dw, want_db, sw, sb = _wgrad_oracle(Dv, Gv, with_scale=True)
    K = B * H * 64
    T.check_bound(f"trunk_wgrad dw_all B={B} H={H}", dw, want_dw, K * T.U * sw)
    T.check_bound(f"trunk_wgrad db_all B={B} H={H}", db, want_db, K * T.U * sb)
    rc2, dw2, db2, _ = _call_wgrad(1, drow, grow, nb, B, H)
    assert rc2 == 0 and torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize("B,H,W", [(1, 8, 32), (1, 12, 64), (1, 0, 64)])
def test_trunk_wgrad_refuses_other_geometries(B, H, W):
    L = _lib.lib()
    assert L.srbh_trunk_wgrad_ws_bytes(1, B, H, W) == 0 and L.srbh_trunk_wgrad_ws_bytes(1, 1, 8, 64) > 0
    Dv = torch.ones(3, 1, 192, 16, 64)
    drow, nb = _row(Dv, 0)
    grow, _ = _row(Dv, 1)
    before = (drow.clone(), grow.clone())
    rc, dw, db, ws = _call_wgrad(1, drow, grow, nb, B, H, W)
    assert rc != 0
    assert bool(dw.isnan().all()) and bool(db.isnan().all()) and bool(ws.isnan().all()), "a refused call wrote"
    assert torch.equal(drow, before[0]) and torch.equal(grow, before[1])


# ---- b, c, d. the fast forward and backward on a network, read back layer by layer --------------------------------------------------------------
def _net(blocks):
    from srbh_amd import synth
    from srbh_amd.rrdbnet import RRDBNet
    net = RRDBNet(3, 3, num_block=blocks)
    net.load_state_dict(synth.rrdbnet_state_dict(num_block=blocks, seed=5, mode="stress"))
    return net.to(DEV)


def _read_row(row, nb, n_buf, B, H, W, dtype):
    return [G.act16_planes(row[k * nb:(k + 1) * nb], B, 6, H, W, dtype).cpu().clone() for k in range(n_buf)]


@functools.lru_cache(maxsize=None)
def _case(blocks, B, H, W, mode):
    """ONE run of the fast forward and backward (mode: "persistent", "impulse" = persistent with the output gradient at one corner pixel,
    "per_layer" = the fallback through the C ABI with two G buffers); everything the checks need, on the CPU.  Shared by the tests below."""
    from srbh_amd import rrdbnet_autograd as RA
    net = _net(blocks)
    n_rdb = 3 * blocks
    feat = _rand((B, H, W, 64), 31).to(DEV).contiguous()
    if mode == "impulse":
        g = torch.zeros(B, H, W, 64)
        g[B - 1, H - 1, W - 1] = _rand((64,), 33)
        g = g.to(DEV)
    else:
        g = _rand((B, H, W, 64), 32).to(DEV).contiguous()
    old = (RA.BWD_PERSISTENT, RA.TRUNK_WGRAD)
    RA._FAST_WS.clear()
    lease = None
    try:
        RA.BWD_PERSISTENT, RA.TRUNK_WGRAD = True, True
        fwd0 = dict(RA.TRUNK_FWD_PATHS)
        xr, lease = RA._trunk_fast_forward(net, feat)
        torch.cuda.synchronize()
        ws = lease.ws
        nb = ws["nb"]
        fwd_path = [k for k in fwd0 if RA.TRUNK_FWD_PATHS[k] != fwd0[k]]
        d_before = ws["D"].clone()
        bwd0 = dict(RA.TRUNK_BWD_PATHS)
        if mode == "per_layer":
            assert ws.get("aux") is None and ws["G"].numel() == 2 * nb, "this geometry was meant to be one the persistent kernel does not take"
            packs = net.__dict__.setdefault("_srbh_trunk_bwd_packs", RA._TrunkBwdPacks()).get(net)
            offs = (C.c_size_t * 5)(*packs.offs)
            ga, gb, gc = g.clone(), torch.empty_like(g), torch.empty_like(g)
            dw_all = torch.full((n_rdb * T.DW_RDB,), NAN, dtype=torch.float32, device=DEV)
            db_all = torch.full((n_rdb * T.DB_RDB,), NAN, dtype=torch.float32, device=DEV)
            gout = C.c_void_p()
            _lib.check(_lib.lib().srbh_rrdbnet_trunk_train_backward(blocks, ws["D"].data_ptr(), nb, packs.buf.data_ptr(), packs.stride, offs, ga.data_ptr(),
                                                                    gb.data_ptr(), gc.data_ptr(), C.byref(gout), ws["G"].data_ptr(), nb, dw_all.data_ptr(),
                                                                    db_all.data_ptr(), ws["wg"].data_ptr(), B, H, W, _lib.stream_ptr()), "rrdbnet_trunk_train_backward")
            torch.cuda.synchronize()
            gin = {t.data_ptr(): t for t in (ga, gb, gc)}[gout.value]
            dw_all, db_all, n_g = dw_all.cpu(), db_all.cpu(), 2
        else:
            grads = {}
            gin = RA._trunk_fast_backward(net, lease, g.clone(), grads)
            torch.cuda.synchronize()
            dw_all = torch.cat([grads[id(getattr(getattr(blk, f"rdb{r}"), f"conv{k}").weight)].reshape(-1).cpu()
                                for blk in net.body for r in (1, 2, 3) for k in range(1, 6)])
            db_all = torch.full((n_rdb * T.DB_RDB,), NAN)
            i = 0
            for blk in net.body:
                for r in (1, 2, 3):
                    for k, (ch0, cout, _) in enumerate(T.CONV_GEO):
                        db_all[i * 192 + ch0:i * 192 + ch0 + cout] = grads[id(getattr(getattr(blk, f"rdb{r}"), f"conv{k + 1}").bias)].cpu()
                    i += 1
            n_g = n_rdb + 1
        bwd_path = [k for k in bwd0 if RA.TRUNK_BWD_PATHS[k] != bwd0[k]]
        res = {
            "blocks": blocks, "B": B, "H": H, "Wimg": W, "n_rdb": n_rdb, "fwd_path": fwd_path, "bwd_path": bwd_path,
            "feat": feat.cpu().permute(0, 3, 1, 2).double(), "g32": g.cpu().permute(0, 3, 1, 2).contiguous(),
            "xr": xr.cpu().permute(0, 3, 1, 2).double(), "gin": gin.cpu().permute(0, 3, 1, 2).double(), "dw_all": dw_all, "db_all": db_all,
            "D": _read_row(ws["D"], nb, n_rdb + 1, B, H, W, torch.float16), "G": _read_row(ws["G"], nb, n_g, B, H, W, torch.bfloat16),
            "borders": all(G.border_is_zero(ws["D"][k * nb:(k + 1) * nb], B, 6, H, W) for k in range(n_rdb + 1))
            and all(G.border_is_zero(ws["G"][k * nb:(k + 1) * nb], B, 6, H, W) for k in range(n_g)),
            "d_unchanged": torch.equal(d_before, ws["D"]),
            "W": [[getattr(getattr(blk, f"rdb{r}"), f"conv{k}").weight.detach().cpu().float() for k in range(1, 6)] for blk in net.body for r in (1, 2, 3)],
            "b": [[getattr(getattr(blk, f"rdb{r}"), f"conv{k}").bias.detach().cpu().double() for k in range(1, 6)] for blk in net.body for r in (1, 2, 3)],
        }
        return res
    finally:
        RA.BWD_PERSISTENT, RA.TRUNK_WGRAD = old
        if lease is not None:
            lease.release()
        RA._FAST_WS.clear()


GEOMETRIES = [(1, 1, 8), (1, 2, 16), (2, 1, 24)]      # (blocks, B, H): one tile per image; one neighbour per tile; a tile with two neighbours + an RRDB boundary


def _check_forward(c, tag):
    """every saved plane x1..x4 against dense_local (fp16 weights, bias, LeakyReLU), planes 0..1 of every next buffer against fp16 of the float64
    stream, the fp32 output against the stream"""
    n_rdb = c["n_rdb"]
    D = [d.double() for d in c["D"]]
    assert torch.equal(c["D"][0][:, :64].view(torch.int16), c["feat"].half().view(torch.int16)), "buffer 0 holds fp16 of the input"
    Wf = [[w.half().double() for w in ws] for ws in c["W"]]
    out = T.trunk_streams(D[:n_rdb], Wf, c["b"], c["feat"])
    worst = {"plane": 0.0, "next": 0.0}
    for i in range(n_rdb):
        for k in range(4):
            ref, sc = out[i]["inner"][k]
            r = T.ratio(D[i][:, 64 + 32 * k:96 + 32 * k], ref, T.inner_bound(k, sc, ref, T.half_ulp_f16))
            assert r <= 1.0, (tag, "forward plane", i, k, r)
            worst["plane"] = max(worst["plane"], r)
        ref, bnd = out[i]["stream"], out[i]["bound"]
        r = T.ratio(D[i + 1][:, :64], ref, bnd + T.half_ulp_f16(ref.abs() + bnd))
        assert r <= 1.0, (tag, "planes 0..1 of buffer", i + 1, r)
        worst["next"] = max(worst["next"], r)
        assert not bool(D[i + 1][:, 64:].any()) or i + 1 < n_rdb
    print(f"[trunk_train] {tag} forward: x1..x4 {worst['plane']:.3e}, fp16 of the stream {worst['next']:.3e}")
    T.check_bound(f"{tag} forward fp32 output", c["xr"], out[-1]["stream"], out[-1]["bound"])
    assert bool(torch.isfinite(c["xr"]).all()) and c["borders"]


def _bwd_operands(c, i):
    """gradient convs (bf16 of the stacked slices) and LeakyReLU masks [X4 | X3 | X2 | X1] of forward RDB i"""
    Wb = [T.bf16_rne(w) for w in T.bwd_weights(c["W"][i])]
    D = c["D"][i].double()
    return Wb, torch.cat([D[:, 160:192], D[:, 128:160], D[:, 96:128], D[:, 64:96]], 1)


def _check_wgrad(c, tag, k, i):
    """RDB i's slices of dw_all / db_all against wgrad of its saved buffer and G buffer k"""
    dw, db, sw, sb = T.wgrad(T.f16_to_bf16(c["D"][i]), c["G"][k].double(), with_scale=True)
    K = c["B"] * c["H"] * c["Wimg"]
    rw = T.ratio(c["dw_all"][i * T.DW_RDB:(i + 1) * T.DW_RDB], dw, K * (T.U * sw + T.TINY))
    rb = T.ratio(c["db_all"][i * 192:(i + 1) * 192], db, K * (T.U * sb + T.TINY))
    assert rw <= 1.0 and rb <= 1.0, (tag, "weight / bias gradient of RDB", i, rw, rb)
    return rw, rb


def _check_persistent_backward(c, tag):
    n_rdb = c["n_rdb"]
    assert c["bwd_path"] == ["persistent"] and c["fwd_path"] == ["persistent"]
    Gr = [g.double() for g in c["G"]]
    x0 = (c["g32"] * 0.04).double()          # fp32 product, as staged (srbh_axpby_f32 / srbh_nhwc32_to_act16 with scale 0.04f)
    assert torch.equal(c["G"][0][:, :64].view(torch.int16), (c["g32"] * 0.04).to(torch.bfloat16).view(torch.int16)), "g5 of buffer 0 is bf16(0.2 * 0.2 * g)"
    ops = [_bwd_operands(c, n_rdb - 1 - k) for k in range(n_rdb)]
    out = T.trunk_streams(Gr[:n_rdb], [o[0] for o in ops], None, x0, masks=[o[1] for o in ops])
    worst = {"plane": 0.0, "g5": 0.0, "dw": 0.0, "db": 0.0}
    for k in range(n_rdb):
        for j in range(4):
            ref, sc = out[k]["inner"][j]
            r = T.ratio(Gr[k][:, 64 + 32 * j:96 + 32 * j], ref, T.inner_bound(j, sc, ref, T.half_ulp_bf16))
            assert r <= 1.0, (tag, "gradient plane", k, j, r)
            worst["plane"] = max(worst["plane"], r)
        ref, bnd = out[k]["stream"], out[k]["bound"]
        r = T.ratio(Gr[k + 1][:, :64], ref, bnd + T.half_ulp_bf16(ref.abs() + bnd))
        assert r <= 1.0, (tag, "g5 of buffer", k + 1, r)
        worst["g5"] = max(worst["g5"], r)
        rw, rb = _check_wgrad(c, tag, k, n_rdb - 1 - k)
        worst["dw"], worst["db"] = max(worst["dw"], rw), max(worst["db"], rb)
    print(f"[trunk_train] {tag} backward: g4..g1 {worst['plane']:.3e}, g5 {worst['g5']:.3e}, dw_all {worst['dw']:.3e}, db_all {worst['db']:.3e}")
    ref = 25.0 * out[-1]["stream"]
    T.check_bound(f"{tag} input gradient", c["gin"], ref, 25.0 * out[-1]["bound"] + T.U * ref.abs() + T.TINY)
    assert bool(torch.isfinite(c["gin"]).all()) and bool(torch.isfinite(c["dw_all"]).all()) and bool(torch.isfinite(c["db_all"]).all())
    assert all(bool(torch.isfinite(g).all()) for g in Gr)
    assert c["borders"], "a border of the D or G row was written"
    assert c["d_unchanged"], "the backward wrote to the saved forward planes"
    assert float(c["gin"].abs().max()) > 0 and float(c["dw_all"].abs().max()) > 0


@pytest.mark.parametrize("blocks,B,H", GEOMETRIES)
def test_persistent_training_forward_layer_by_layer(blocks, B, H):
    c = _case(blocks, B, H, 64, "persistent")
    assert c["fwd_path"] == ["persistent"]
    _check_forward(c, f"persistent ({blocks}, {B}, {H})")


@pytest.mark.parametrize("blocks,B,H", GEOMETRIES)
def test_persistent_training_backward_layer_by_layer(blocks, B, H):
    """srbh_rrdbnet_trunk_train_backward_persistent + srbh_trunk_wgrad behind it, read back from the G row: every g4..g1 plane of every RDB, g5 of
    every next buffer (bf16 of the float64 stream), the input gradient (25 x the stream), every element of dw_all / db_all, borders, finiteness"""
    _check_persistent_backward(_case(blocks, B, H, 64, "persistent"), f"persistent ({blocks}, {B}, {H})")


def test_persistent_training_backward_of_a_corner_impulse():
    """the same checks with the output gradient at the last image's last pixel only: few terms reach each output, a dropped tap is glaring"""
    c = _case(2, 1, 24, 64, "impulse")
    assert not bool(c["G"][0][:, :, :8].any()) and bool(c["G"][0][:, :64, 23, 63].any())          # (the impulse sits where it was put)
    _check_persistent_backward(c, "impulse (2, 1, 24)")


def test_per_layer_training_backward_at_a_geometry_the_persistent_kernel_refuses():
    """srbh_rrdbnet_trunk_train_backward (srbh_conv3x3_x16 + srbh_act16_wgrad_b16 + srbh_act16_channel_sum) through the C ABI with two G buffers at
    12 x 48 (srbh_rrdbnet_trunk_train_aux_bytes is 0 there: ragged in both directions), num_block 1.  The G buffers of RDB 1 (buffer 1) and RDB 0
    (buffer 0) survive: their g4..g1 planes, those RDBs' slices of dw_all / db_all (db_all comes from fp32 atomics: bounded, never compared by bits),
    and what of the streams survives: g5 of RDB 0 is bf16 of 0.2 (dx_1 + cur_1) with 0.2 cur_1 known as RDB 1's g5 to half a bf16 ulp, and the input
    gradient is g + dx_0 + cur_0 with 0.2 cur_0 known the same way.  The per-layer forward that fed it is checked like the persistent one."""
    c = _case(1, 1, 12, 48, "per_layer")
    tag = "per-layer (1, 1, 12, 48)"
    assert c["fwd_path"] == ["per_layer"] and _lib.lib().srbh_rrdbnet_trunk_train_aux_bytes(1, 12, 48) == 0
    _check_forward(c, tag)
    Gr = [g.double() for g in c["G"]]
    streams = {}
    for k, i in ((1, 1), (0, 0)):
        Wb, mask = _bwd_operands(c, i)
        inner, (s, sc) = T.dense_local(Gr[k], Wb, None, mask, Gr[k][:, :64])
        for j in range(4):
            ref, scj = inner[j]
            T.check_bound(f"{tag} RDB {i} gradient plane {j + 1}", Gr[k][:, 64 + 32 * j:96 + 32 * j], ref, T.inner_bound(j, scj, ref, T.half_ulp_bf16))
        rw, rb = _check_wgrad(c, tag, k, i)
        print(f"[trunk_train] {tag} RDB {i}: dw_all {rw:.3e}, db_all {rb:.3e}")
        # s = 0.2 conv5(G) + g5 = 0.2 (dx + cur) up to g5's own rounding
        streams[i] = (s, (9 * 192 + 2) * (T.U * (sc - Gr[k][:, :64].abs()) + T.TINY) + T.half_ulp_bf16(Gr[k][:, :64]) + 3 * T.U * s.abs())          # (|v - bf16(v)| <= half an ulp at bf16(v))
    s1, b1 = streams[1]
    T.check_bound(f"{tag} g5 of RDB 0", Gr[0][:, :64], s1, b1 + T.half_ulp_bf16(s1.abs() + b1))
    s0, b0 = streams[0]
    g64 = c["g32"].double()
    ref = g64 + 5.0 * s0
    T.check_bound(f"{tag} input gradient", c["gin"], ref, 5.0 * b0 + 2 * T.U * (g64.abs() + 5.0 * s0.abs()))
    assert c["borders"] and c["d_unchanged"] and bool(torch.isfinite(c["gin"]).all())
    assert bool(torch.isfinite(c["dw_all"]).all()) and bool(torch.isfinite(c["db_all"]).all())
