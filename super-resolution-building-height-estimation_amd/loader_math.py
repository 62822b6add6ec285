"""Loader-side tensor math on the device (reference BH_loader.py:30-61,326-329,361-392).

``hierweight*`` are the (tiny, host-side) class-weight formulas; ``LabelPrep`` / ``normalize_tiles`` are libsrbh
kernels that turn a batch of raw uint8 height labels / raw band values into the tensors the training step consumes;
``GridTiles`` cuts and normalises the inference tiles of a city from its two device rasters, one batch per launch."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

__all__ = ["hierweight", "hierweight_simple", "hierweight_equal", "LabelPrep", "normalize_tiles", "Augment", "AugmentParams",
           "DeviceAugment", "train_batch", "sr_pair", "grid_windows", "check_windows", "GridTiles"]


def _class_freq(stats, hir):
    stats = np.asarray(stats, dtype=np.float64)
    stats = stats / stats.sum()
    return np.array([stats[hir[i]:hir[i + 1]].sum() for i in range(len(hir) - 1)])


def _rescale(w):
    w = w / w.sum()
    return len(w) / np.sum(w) * w


def hierweight(stats, hir):
    """inverse square-root class frequency, rescaled so that the weights sum to the class count (BH_loader.py:30-41)."""
    return _rescale(1.0 / np.sqrt(_class_freq(stats, hir)))


def hierweight_simple(stats, hir):
    """plain inverse frequency (BH_loader.py:44-55)."""
    return _rescale(1.0 / _class_freq(stats, hir))


def hierweight_equal(stats, hir):
    return np.ones((len(hir) - 1,))


class LabelPrep:
    """buildhir LUT + class weights on the device (BH_loader.py:326-329,373-392)."""

    def __init__(self, hir, heightweight, device):
        lut = np.zeros((256,), dtype=np.uint8)
        for i in range(len(hir) - 1):
            lut[hir[i]:hir[i + 1]] = i
        self.lut = torch.from_numpy(lut).to(device)
        self.cw = torch.as_tensor(np.asarray(heightweight), dtype=torch.float32, device=device)

    def __call__(self, height_u8):
        """height_u8: (B,H,W) uint8 device tensor -> (height [B,H,W] f32, height_aggre [B,H/4,W/4], build int64,
        weight, weight_aggre)"""
        if not (height_u8.is_cuda and height_u8.dtype == torch.uint8 and height_u8.dim() == 3):
            raise RuntimeError("LabelPrep (libsrbh): expects a (B,H,W) uint8 device tensor")
        h = height_u8.contiguous()
        if h.data_ptr() % 4:          # a contiguous view may start at any byte; the kernel reads four labels at a time
            h = h.clone()
        B, Hh, Ww = h.shape
        dev = h.device
        build = torch.empty((B, Hh, Ww), dtype=torch.int64, device=dev)
        hf = torch.empty((B, Hh, Ww), dtype=torch.float32, device=dev)
        wt = torch.empty((B, Hh, Ww), dtype=torch.float32, device=dev)
        ha = torch.empty((B, Hh // 4, Ww // 4), dtype=torch.float32, device=dev)
        wa = torch.empty((B, Hh // 4, Ww // 4), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().srbh_label_prep(h.data_ptr(), B, Hh, Ww, self.lut.data_ptr(), self.cw.data_ptr(),
                                              build.data_ptr(), hf.data_ptr(), wt.data_ptr(), ha.data_ptr(), wa.data_ptr(),
                                              _lib.stream_ptr()), "label_prep")
        return hf, ha, build, wt, wa


def normalize_tiles(img, mins, maxs, datarange=(0, 1)):
    """(img - min) / (max - min) per band then clip (BH_loader.py:361-369; `normmethod='minmax'`, :304-306)."""
    if not img.is_cuda:
        raise RuntimeError("normalize_tiles (libsrbh): device tensors only")
    x = img.detach().float().contiguous()
    B, Cc, Hh, Ww = x.shape
    mn = torch.as_tensor(np.asarray(mins), dtype=torch.float32, device=x.device)
    rg = torch.as_tensor(np.asarray(maxs) - np.asarray(mins), dtype=torch.float32, device=x.device)
    out = torch.empty_like(x)
    clamp = isinstance(datarange, tuple)
    lo, hi = (datarange if clamp else (0.0, 0.0))
    _lib.check(_lib.lib().srbh_normalize_clamp(x.data_ptr(), out.data_ptr(), B, Cc, Hh, Ww, mn.data_ptr(), rg.data_ptr(),
                                               float(lo), float(hi), int(clamp), _lib.stream_ptr()), "normalize_clamp")
    return out


# ---- training augmentation on the device (BH_loader.py:356-359, :735-737; definition: DESIGN.md 3.x) ------------------------------
_IDENTITY_PERM = (0, 1, 2, 3)
_FIX = 1024.0               # the rotation's coordinates are 2^-10 fixed point
_MAX_GRID = 32768           # as libsrbh's check: |coordinate| * 1024 stays far inside int32


class AugmentParams:
    """One batch's augmentation as CPU tensors: ``flip`` (B,) int32 codes 0..3 (bit 0 reverses the columns, bit 1 the rows), ``perm``
    (B, 4) int32 (source cell of destination cell i; cells row-major), ``angle`` (B,) float64 degrees counter-clockwise and ``rotate``
    (B,) bool (False: that image is not rotated whatever its angle).  ``Augment.draw`` makes one; tests build them from explicit values."""

    def __init__(self, flip, perm, angle, rotate=None):
        self.flip = torch.as_tensor(flip, dtype=torch.int32).reshape(-1).contiguous()
        B = self.flip.numel()
        self.perm = torch.as_tensor(perm, dtype=torch.int32).reshape(-1, 4).contiguous()
        self.angle = torch.as_tensor(angle, dtype=torch.float64).reshape(-1).contiguous()
        self.rotate = (torch.ones(B, dtype=torch.bool) if rotate is None else torch.as_tensor(rotate, dtype=torch.bool).reshape(-1)).contiguous()
        for t in (self.flip, self.perm, self.angle, self.rotate):
            if t.is_cuda:
                raise ValueError("AugmentParams: the parameters are CPU tensors (Augment.to_device uploads them)")
        if not (self.perm.shape[0] == B and self.angle.numel() == B and self.rotate.numel() == B):
            raise ValueError(f"AugmentParams: flip, perm, angle and rotate must describe the same {B} images")
        if B and (int(self.flip.min()) < 0 or int(self.flip.max()) > 3):
            raise ValueError("AugmentParams: a flip code is 0 (none), 1 (columns), 2 (rows) or 3 (both)")
        if B and not bool((self.perm.sort(dim=1).values == torch.arange(4, dtype=torch.int32)).all()):
            raise ValueError("AugmentParams: every perm row must be a permutation of 0..3")
        if not bool(torch.isfinite(self.angle).all()):
            raise ValueError("AugmentParams: angles must be finite")

    def __len__(self):
        return self.flip.numel()

    @classmethod
    def identity(cls, B):
        return cls(torch.zeros(B, dtype=torch.int32), torch.tensor(_IDENTITY_PERM, dtype=torch.int32).repeat(B, 1),
                   torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.bool))


class DeviceAugment:
    """``AugmentParams`` for one grid size on the device: int32 ``flip`` (B,), ``perm`` (B, 4), ``tables`` (B, 2 Wg + 2 Hg) and the fp32
    ``consts`` that rode along, all views of ONE device buffer that one copy filled."""

    def __init__(self, B, Hg, Wg, flip, perm, tables, consts):
        self.B, self.Hg, self.Wg = B, Hg, Wg
        self.flip, self.perm, self.tables, self.consts = flip, perm, tables, consts


class Augment:
    """The reference's ``A.Compose([A.Flip(p=0.5), A.RandomGridShuffle(grid=(2, 2), p=0.5), A.Rotate(p=0.5)])`` (BH_loader.py:62-66,
    :713-716) as parameters for libsrbh's gather kernels.  The transforms are DEFINED in DESIGN.md 3.x: modelled on what albumentations
    and cv2 are understood to do, not tested against either (neither is available), and albumentations' random stream is not matched."""

    def __init__(self, grid=(2, 2), limit=90, p_flip=0.5, p_shuffle=0.5, p_rotate=0.5):
        if tuple(grid) != (2, 2):
            raise NotImplementedError(f"Augment: only grid=(2, 2) is supported (got {tuple(grid)})")
        self.grid, self.limit = (2, 2), float(limit)
        self.p_flip, self.p_shuffle, self.p_rotate = float(p_flip), float(p_shuffle), float(p_rotate)

    def draw(self, B, generator):
        """each step independently with its probability: a flip code uniform on {1, 2, 3}, a uniform permutation of the four cells (the
        identity included), an angle uniform on [-limit, limit).  `generator`: a CPU torch.Generator, so a seed reproduces a run."""
        if generator.device.type != "cpu":
            raise ValueError("Augment.draw: a CPU torch.Generator (the parameters are made on the host)")
        u = torch.rand((B, 3), generator=generator, dtype=torch.float64)
        code = torch.randint(1, 4, (B,), generator=generator, dtype=torch.int32)
        perm = torch.rand((B, 4), generator=generator, dtype=torch.float64).argsort(dim=1).to(torch.int32)
        angle = (torch.rand((B,), generator=generator, dtype=torch.float64) * 2.0 - 1.0) * self.limit
        do_flip, do_shuffle, do_rotate = u[:, 0] < self.p_flip, u[:, 1] < self.p_shuffle, u[:, 2] < self.p_rotate
        flip = torch.where(do_flip, code, torch.zeros_like(code))
        perm = torch.where(do_shuffle[:, None], perm, torch.tensor(_IDENTITY_PERM, dtype=torch.int32).expand(B, 4))
        angle = torch.where(do_rotate, angle, torch.zeros_like(angle))
        return AugmentParams(flip, perm, angle, do_rotate)

    @staticmethod
    def _check_grid(Hg, Wg):
        if Hg <= 0 or Wg <= 0 or Hg % 8 or Wg % 8 or Hg > _MAX_GRID or Wg > _MAX_GRID:
            raise ValueError(f"Augment: the grid {Hg} x {Wg} must be multiples of 8, at most {_MAX_GRID} a side")

    def tables(self, params, Hg, Wg):
        """(B, 2 Wg + 2 Hg) int32 numpy: per image ax[Wg], bx[Wg], X0[Hg], Y0[Hg] of the inverse rotation about the pixel-centre
        point ((Wg-1)/2, (Hg-1)/2), float64 on the host, rounded to nearest-even at 2^-10.  An image that is not rotated gets the
        identity tables, which give back every pixel exactly with fraction 0."""
        self._check_grid(Hg, Wg)
        ang = np.radians(np.where(params.rotate.numpy(), params.angle.numpy(), 0.0))
        a, b = np.cos(ang)[:, None], np.sin(ang)[:, None]
        cx, cy = (Wg - 1) / 2.0, (Hg - 1) / 2.0
        m0, m1, m2 = a, -b, cx - a * cx + b * cy
        m3, m4, m5 = b, a, cy - b * cx - a * cy
        x, y = np.arange(Wg, dtype=np.float64)[None, :], np.arange(Hg, dtype=np.float64)[None, :]
        t = np.concatenate([np.rint(m0 * x * _FIX), np.rint(m3 * x * _FIX), np.rint((m1 * y + m2) * _FIX), np.rint((m4 * y + m5) * _FIX)], axis=1)
        return t.astype(np.int32)

    def to_device(self, params, Hg, Wg, device, consts=()):
        """Upload one batch's parameters for an Hg x Wg grid: one pinned staging buffer, one non_blocking copy, no host synchronisation
        (the thread that prepares a batch is the thread that queues the training step's launches: see harness._label_consts).  `consts`:
        float vectors (the bands' mins / ranges) that ride in the same copy and come back as fp32 device views.  The pinned buffer is a
        fresh one per batch from torch's caching host allocator, which hands it out again only after the copy has run."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("Augment.to_device (libsrbh): device tensors only -- there is no CPU path")
        B, T = len(params), 2 * Wg + 2 * Hg
        tab = self.tables(params, Hg, Wg)
        cs = [np.ascontiguousarray(c, dtype=np.float32).reshape(-1) for c in consts]
        n_t, n_p = B * T, B * 4                  # tables first, then perm: both stay 16-byte aligned (T % 16 == 0)
        offs = np.cumsum([0, n_t, n_p, (B + 3) // 4 * 4] + [(c.size + 3) // 4 * 4 for c in cs]).tolist()
        stage = torch.empty((int(offs[-1]),), dtype=torch.int32, pin_memory=True)
        host = stage.numpy()
        host[:n_t] = tab.reshape(-1)
        host[n_t:n_t + n_p] = params.perm.numpy().reshape(-1)
        host[offs[2]:offs[2] + B] = params.flip.numpy()
        for c, o in zip(cs, offs[3:]):
            host[o:o + c.size] = c.view(np.int32)
        dev = stage.to(device, non_blocking=True)
        views = [dev[o:o + c.size].view(torch.float32) for c, o in zip(cs, offs[3:])]
        return DeviceAugment(B, Hg, Wg, dev[offs[2]:offs[2] + B], dev[n_t:n_t + n_p].view(B, 4), dev[:n_t].view(B, T), views)


_AUGMENT = Augment()


def _aug_image(x, up, step, dp, mins, ranges, datarange, what):
    """x (B,C,Hs,Ws) fp32 device tensor -> the augmented grid (Hs up x Ws up) sampled every `step` pixels, normalised when mins is given"""
    B, Cc, Hs, Ws = x.shape
    if (B, Hs * up, Ws * up) != (dp.B, dp.Hg, dp.Wg):
        raise ValueError(f"{what}: parameters made for {dp.B} images of {dp.Hg} x {dp.Wg}, tensor is {B} x {Hs * up} x {Ws * up}")
    out = torch.empty((B, Cc, Hs * up // step, Ws * up // step), dtype=torch.float32, device=x.device)
    clamp = mins is not None and isinstance(datarange, tuple)
    lo, hi = (datarange if clamp else (0.0, 0.0))
    _lib.check(_lib.lib().srbh_aug_image(x.data_ptr(), B, Cc, Hs, Ws, up, out.data_ptr(), step, dp.flip.data_ptr(), dp.perm.data_ptr(),
                                         dp.tables.data_ptr(), None if mins is None else mins.data_ptr(),
                                         None if mins is None else ranges.data_ptr(), float(lo), float(hi), int(clamp),
                                         _lib.stream_ptr()), what)
    return out


def _f32_image(t, what):
    if not (t.is_cuda and t.dim() == 4):
        raise RuntimeError(f"{what} (libsrbh): expects (B,C,H,W) device tensors -- there is no CPU path")
    return t.detach().float().contiguous()


def _band_consts(mins, maxs, Cc, what):
    mn, rg = np.asarray(mins), np.asarray(maxs) - np.asarray(mins)
    if mn.shape != (Cc,) or rg.shape != (Cc,):
        raise ValueError(f"{what}: mins / maxs must hold one value per band ({Cc})")
    return mn, rg


def train_batch(raw_img, height_u8, mins, maxs, prep, params=None, datarange=(0, 1)):
    """One height-stage training batch from raw tensors on the device, as myImageFloder_S12_globe.__getitem__ makes it
    (BH_loader.py:353-392): raw_img (B,C,h,w) fp32 raw bands, height_u8 (B,4h,4w) uint8 labels, `prep` a LabelPrep.  Returns
    (lr, height, height_aggre, build, weight, weight_aggre) -- what harness.synthetic_batch_device returns and TrainStep consumes.
    `params`: AugmentParams (Augment.draw); None is the un-augmented batch, through the same kernels with identity parameters."""
    x = _f32_image(raw_img, "train_batch")
    if not (height_u8.is_cuda and height_u8.dtype == torch.uint8 and height_u8.dim() == 3):
        raise RuntimeError("train_batch (libsrbh): expects a (B,H,W) uint8 device tensor of labels -- there is no CPU path")
    B, Cc, Hs, Ws = x.shape
    h = height_u8.contiguous()
    if tuple(h.shape) != (B, 4 * Hs, 4 * Ws):
        raise ValueError(f"train_batch: labels {tuple(h.shape)} do not match the x4 grid of tiles {tuple(x.shape)}")
    Hg, Wg = 4 * Hs, 4 * Ws
    if params is None:
        params = AugmentParams.identity(B)
    dp = _AUGMENT.to_device(params, Hg, Wg, x.device, _band_consts(mins, maxs, Cc, "train_batch"))
    lr = _aug_image(x, 4, 4, dp, dp.consts[0], dp.consts[1], datarange, "aug_image")
    dev = x.device
    build = torch.empty((B, Hg, Wg), dtype=torch.int64, device=dev)
    hf = torch.empty((B, Hg, Wg), dtype=torch.float32, device=dev)
    wt = torch.empty((B, Hg, Wg), dtype=torch.float32, device=dev)
    ha = torch.empty((B, Hs, Ws), dtype=torch.float32, device=dev)
    wa = torch.empty((B, Hs, Ws), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().srbh_aug_label_prep(h.data_ptr(), B, Hg, Wg, dp.flip.data_ptr(), dp.perm.data_ptr(), dp.tables.data_ptr(),
                                              prep.lut.data_ptr(), prep.cw.data_ptr(), build.data_ptr(), hf.data_ptr(), wt.data_ptr(),
                                              ha.data_ptr(), wa.data_ptr(), None, _lib.stream_ptr()), "aug_label_prep")
    return lr, hf, ha, build, wt, wa


def sr_pair(raw_lr, raw_hr, lr_mins, lr_maxs, hr_mins, hr_maxs, params, datarange=(0, 1)):
    """One SR-stage training pair as myImageFloderLRHRglobe.__getitem__ makes it (BH_loader.py:731-750): raw_lr (B,C,h,w) and raw_hr
    (B,C',4h,4w) fp32 raw values -> (lq, gt) for RealESRGAN.feed_data; both get the same augmentation, lq is clipped to `datarange`,
    gt is not (:747-750).  `params` None: no augmentation."""
    lr, hr = _f32_image(raw_lr, "sr_pair"), _f32_image(raw_hr, "sr_pair")
    B, Cl, Hs, Ws = lr.shape
    if (hr.shape[0], hr.shape[2], hr.shape[3]) != (B, 4 * Hs, 4 * Ws):
        raise ValueError(f"sr_pair: HR {tuple(hr.shape)} is not the x4 grid of LR {tuple(lr.shape)}")
    if params is None:
        params = AugmentParams.identity(B)
    consts = _band_consts(lr_mins, lr_maxs, Cl, "sr_pair") + _band_consts(hr_mins, hr_maxs, hr.shape[1], "sr_pair")
    dp = _AUGMENT.to_device(params, 4 * Hs, 4 * Ws, lr.device, consts)
    lq = _aug_image(lr, 4, 4, dp, dp.consts[0], dp.consts[1], datarange, "aug_image")
    gt = _aug_image(hr, 1, 1, dp, dp.consts[2], dp.consts[3], None, "aug_image")
    return lq, gt


# ---- inference tiles cut from a city's device rasters (BH_loader.py:933-993, gridimgLoader; definition: DESIGN.md 3.24) -------------
def _grid_starts(length, cell, stride):
    """starts k * stride below `length`; one with k > 0 is kept only if its window holds a pixel the previous window did not"""
    return [x for x in range(0, length, stride) if x == 0 or x + cell - stride < length]


def grid_windows(width, height, cell=64, stride=64):
    """(N, 4) int64, row-major: the windows (xoff, yoff, xcount, ycount) of a regular grid of `cell`-sided cells every `stride` pixels over
    a width x height raster, clipped at the right and bottom edges (count = min(cell, length - start)).  Every pixel lies in at least
    one window; stride 48 with cell 64 is the overlapping layout of the inference workload."""
    if not (width >= 1 and height >= 1 and cell >= 1 and 1 <= stride <= cell):
        raise ValueError(f"grid_windows: needs width, height, cell >= 1 and 1 <= stride <= cell (got {width}, {height}, {cell}, {stride})")
    xs, ys = _grid_starts(width, cell, stride), _grid_starts(height, cell, stride)
    return np.array([[x, y, min(cell, width - x), min(cell, height - y)] for y in ys for x in xs], dtype=np.int64).reshape(-1, 4)


def check_windows(pos, width, height, tile):
    """Host-side validation of (N, 4) windows (xoff, yoff, xcount, ycount): every window is non-empty, at most `tile` a side and inside
    the width x height raster.  Returns them as an (N, 4) int64 array; raises ValueError naming the first offending row."""
    p = np.asarray(pos.cpu() if torch.is_tensor(pos) else pos)
    if p.ndim != 2 or p.shape[1] != 4 or not np.issubdtype(p.dtype, np.integer):
        raise ValueError(f"check_windows: pos must be (N, 4) integers (xoff, yoff, xcount, ycount), got {p.dtype} {p.shape}")
    p = p.astype(np.int64)
    off, cnt, lim = p[:, :2], p[:, 2:], np.array([width, height], dtype=np.int64)
    bad = np.flatnonzero(((off < 0) | (cnt < 1) | (cnt > tile) | (off + cnt > lim)).any(axis=1))
    if bad.size:
        r = int(bad[0])
        raise ValueError(f"check_windows: row {r} {tuple(int(v) for v in p[r])} is not a window of 1..{tile} pixels a side inside the "
                         f"{width} x {height} raster")
    return p


_GRID_TYPES = {torch.float32: 0, torch.uint16: 1, torch.int16: 2}          # include/srbh.h SRBH_GRID_*


class GridTiles:
    """A city's inference tiles, cut and normalised from its two device rasters one batch at a time: stands where predict_tiles and
    evaluate_tiles take ``tiles``.  ``s2`` (C2, H, W) and ``s1`` (C1, H, W) or None are device tensors of dtype uint16, int16 or float32;
    the stats are (2, C) arrays as np.loadtxt returns them from s2_minmax.txt / s1_minmax.txt (row 0 min, row 1 max), the Sentinel-2
    ones cut to [:, :nchans] (BH_loader.py:956-961); ``pos`` (N, 4) host windows, checked once (check_windows) and uploaded once.
    ``gt[s:e]`` is a fresh fp32 (e - s, nchans + C1, tile, tile) device tensor made by one srbh_grid_tiles launch on the current stream:
    (v - min) / (max - min) inside each window and +0.0 outside it.  ``.pos`` is the validated host array, the ``posall`` to pass on."""

    def __init__(self, s2, s1, pos, s2_stats, s1_stats, nchans=6, tile=64):
        for name, t in (("s2", s2), ("s1", s1)):
            if t is None and name == "s1":
                continue
            if not (torch.is_tensor(t) and t.is_cuda and t.dim() == 3):
                raise RuntimeError(f"GridTiles (libsrbh): {name} must be a (C, H, W) device tensor -- there is no CPU path")
            if t.dtype not in _GRID_TYPES:
                raise TypeError(f"GridTiles: {name} is {t.dtype}; the rasters are uint16, int16 or float32")
        C2, H, W = s2.shape
        if not 1 <= nchans <= C2:
            raise ValueError(f"GridTiles: nchans={nchans} outside 1..{C2}, the bands of s2")
        if s1 is not None and (tuple(s1.shape[1:]) != (H, W) or s1.device != s2.device):
            raise ValueError(f"GridTiles: s1 {tuple(s1.shape)} on {s1.device} does not match s2's {H} x {W} raster on {s2.device}")
        if tile < 4 or tile % 4 or tile > 256:
            raise ValueError(f"GridTiles: tile={tile} must be a multiple of 4 in 4..256")
        C1 = 0 if s1 is None else s1.shape[0]
        st2 = np.asarray(s2_stats, dtype=np.float64)
        if st2.ndim != 2 or st2.shape[0] != 2 or st2.shape[1] < nchans:
            raise ValueError(f"GridTiles: s2_stats {st2.shape} must be (2, C) with at least nchans={nchans} columns (row 0 min, row 1 max)")
        mins, maxs = [st2[0, :nchans]], [st2[1, :nchans]]
        if s1 is not None:
            st1 = np.asarray(s1_stats, dtype=np.float64)
            st1 = st1.reshape(2, -1) if st1.ndim == 1 and st1.size == 2 else st1        # (np.loadtxt of a one-band file gives (2,))
            if st1.ndim != 2 or st1.shape[0] != 2 or st1.shape[1] < C1:
                raise ValueError(f"GridTiles: s1_stats {st1.shape} must be (2, C) with at least the {C1} bands of s1")
            mins.append(st1[0, :C1])
            maxs.append(st1[1, :C1])
        mins, maxs = np.concatenate(mins), np.concatenate(maxs)
        ranges = maxs - mins                                      # float64, rounded once below: as normalize_tiles
        if not (np.isfinite(mins).all() and np.isfinite(ranges).all()) or (ranges.astype(np.float32) == 0).any():
            raise ValueError("GridTiles: every band needs finite stats with max != min (a zero range divides by zero)")
        try:
            self.pos = check_windows(pos, W, H, tile)
        except ValueError as e:
            raise ValueError(f"GridTiles: {e}") from None
        if self.pos.shape[0] == 0:
            raise ValueError("GridTiles: no windows")
        self.s2, self.s1 = s2.contiguous(), None if s1 is None else s1.contiguous()
        self.nchans, self.tile, self.device = nchans, tile, s2.device
        self.shape = (self.pos.shape[0], nchans + C1, tile, tile)
        consts = torch.from_numpy(np.concatenate([mins, ranges]).astype(np.float32))
        self._mins, self._ranges = consts.to(self.device).split(nchans + C1)
        self._pos_dev = torch.from_numpy(self.pos.astype(np.int32)).to(self.device)
        # The memo.  _PredictGraph's look-ahead asks for every full batch twice -- as the NEXT batch of call k and as the CURRENT batch
        # of call k + 1 --, so a slice handed out is kept and handed out again, and it stays valid (neither rewritten nor returned to
        # the allocator) until TWO further distinct slices have been requested; the third further one drops it.  Why that is long
        # enough: a slice is made on the stream that is current at the request (the main stream) but as the "next" batch of call k it
        # is read by a copy on the graph's SIDE stream.  That copy is ordered behind ev_trunk of call k, hence behind the kernel that
        # made the slice, and in front of ev_lr[parity] recorded on the side stream right after; call k + 1 makes the main stream wait
        # for exactly that event (cur.wait_event(ev_lr[p])) before its reg / seg graph.  The two further slices are the "next" batches
        # of calls k + 1 and k + 2, so the slice is dropped no earlier than the request in front of call k + 2, i.e. after call
        # k + 1 was queued whole: whatever the main stream's allocator then puts into that memory is queued behind call k + 1's
        # wait_event and so behind the side stream's read.  As the CURRENT batch the slice is read by copies on the main stream only.
        self._memo = []                                           # [(start, stop), tensor], oldest first, at most three

    def __len__(self):
        return self.shape[0]

    def __getitem__(self, key):
        if not isinstance(key, slice) or key.step not in (None, 1):
            raise TypeError("GridTiles: index with a plain slice gt[s:e] (step 1)")
        s, e, _ = key.indices(self.shape[0])
        if e <= s:
            return torch.empty((0,) + self.shape[1:], dtype=torch.float32, device=self.device)
        for k, t in self._memo:
            if k == (s, e):
                return t
        out = torch.empty((e - s,) + self.shape[1:], dtype=torch.float32, device=self.device)
        s1 = self.s1
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().srbh_grid_tiles(self.s2.data_ptr(), _GRID_TYPES[self.s2.dtype], self.s2.shape[0], self.nchans,
                                                  None if s1 is None else s1.data_ptr(), 0 if s1 is None else _GRID_TYPES[s1.dtype],
                                                  0 if s1 is None else s1.shape[0], self.s2.shape[1], self.s2.shape[2],
                                                  self._pos_dev[s:e].data_ptr(), e - s, self._mins.data_ptr(), self._ranges.data_ptr(),
                                                  out.data_ptr(), self.tile, _lib.stream_ptr()), "grid_tiles")
        self._memo.append(((s, e), out))
        del self._memo[:-3]
        return out
