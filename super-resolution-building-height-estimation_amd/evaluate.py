"""Validation / test pass of the height stage on one libsrbh reduction per batch (reference train.py:315-344 ``vtest_epoch`` and
:427-486 ``vtest_epoch2``).

``HeightEvaluation.add`` is ONE ``srbh_eval_sums`` launch (csrc/srbh_eval.hip) over a batch of head outputs and labels: it reads the
height map, the building logits (NCHW or channels_last, in place), the reference height and the label once and leaves, PER IMAGE, the
float64 sums of d^2, |d| and d per label class and the int64 confusion matrix of argmax(logits) -- where the reference runs an argmax to an
int64 map, a bincount, seven mask-gather reductions and two more reductions for the RMSE, with a ``.item()`` per batch.  The per-image
results stay on the device; nothing synchronises until ``result()`` reads the label-range flag.

The reference's numbers depend on how its loader batched the tiles: ``HeightMetric.addBatch`` accumulates sqrt(mean d^2) * count per class
and BATCH (metrics.py:186-200) and the two loops average a per-batch sqrt (train.py:333-336, :444-445).  ``result()`` therefore regroups the
images, in arrival order, into runs of ``ref_batch`` -- the reference loader's ``batch_size`` (1 in ``main_test``) -- whatever batch size the
device loop ran with.  The kernel is bit-reproducible (ordered float64 sums, no floating-point atomics), so an image's sums do not depend on
the batch it travelled in.  GPU only."""
import torch

from . import _lib
from .metrics import HeightMetric, SegmentationMetric


def _plane(t, H, W):
    """(tensor, pixel stride): `t` of shape (..., H, W) as fp32 whose H x W plane is addressed by ONE element stride per pixel (row stride ==
    W * column stride) -- an NCHW or a channels_last tensor, or a batch slice of one, as it is; anything else is copied"""
    if t.dtype != torch.float32:
        t = t.float()
    sh, sw = t.stride(-2), t.stride(-1)
    if W == 1:
        ps, ok = (sh if H > 1 else 1), True
    else:
        ps, ok = sw, (H == 1 or sh == W * sw)
    if not ok or min(t.stride()) < 0:
        t, ps = t.contiguous(), 1
    return t, ps


class HeightEvaluation:
    """Accumulates the per-image results of ``vtest_epoch`` / ``vtest_epoch2`` on the device.

    ``add(height_pred, build_logits, height_ref, build_label)`` -- one launch per batch, never synchronises.  ``result()`` -- what the
    reference prints and writes, for images grouped into runs of ``ref_batch``.  ``merge_(other)`` -- append another rank's images."""

    def __init__(self, num_class=7, device="cuda", ref_batch=1, keep_maps=False):
        if not 2 <= int(num_class) <= 16:
            raise ValueError(f"HeightEvaluation: 2 to 16 classes (got {num_class})")
        if int(ref_batch) < 1:
            raise ValueError(f"HeightEvaluation: ref_batch must be at least 1 (got {ref_batch})")
        self.num_class = int(num_class)
        self.device = device
        self.ref_batch = int(ref_batch)
        self.keep_maps = bool(keep_maps)
        self.reset()

    def reset(self):
        self._sums = []        # per add: (B, C, 4) float64 -- sum d^2, sum |d|, sum d, count per label class
        self._cm = []          # per add: (B, C, C) int64 -- [label, pred]
        self._bad = None       # int32 device scalar, sticky: a label outside [0, C) was seen
        self.maps = []         # filled by harness.evaluate_tiles(keep_maps=True): per batch, what add() returned
        self.count = 0

    def add(self, height_pred, build_logits, height_ref, build_label):
        """height_pred (B,1,H,W) or (B,H,W) fp32; build_logits (B,C,H,W) fp32, NCHW or channels_last; height_ref (B,H,W); build_label (B,H,W)
        int64 or uint8.  With keep_maps returns (uint16 round(max(h,0)*10), uint8 argmax), each (B,H,W) -- the two rasters ``issave=True``
        writes (train.py:464-478); otherwise None."""
        C = self.num_class
        if height_pred.dim() == 4:
            if height_pred.shape[1] != 1:
                raise ValueError(f"HeightEvaluation.add: height_pred must be (B,1,H,W) or (B,H,W) (got {tuple(height_pred.shape)})")
            height_pred = height_pred[:, 0]
        if height_pred.dim() != 3 or build_logits.dim() != 4:
            raise ValueError("HeightEvaluation.add: height_pred must be (B,1,H,W) or (B,H,W) and build_logits (B,C,H,W) "
                             f"(got {tuple(height_pred.shape)}, {tuple(build_logits.shape)})")
        B, H, W = (int(v) for v in height_pred.shape)
        if tuple(build_logits.shape) != (B, C, H, W):
            raise ValueError(f"HeightEvaluation.add: build_logits must be {(B, C, H, W)} (got {tuple(build_logits.shape)})")
        if tuple(height_ref.shape) != (B, H, W) or tuple(build_label.shape) != (B, H, W):
            raise ValueError(f"HeightEvaluation.add: height_ref and build_label must be {(B, H, W)} "
                             f"(got {tuple(height_ref.shape)}, {tuple(build_label.shape)})")
        if B < 1 or H * W < 1:
            raise ValueError("HeightEvaluation.add: an empty batch")
        if not (height_pred.is_cuda and build_logits.is_cuda and height_ref.is_cuda and build_label.is_cuda):
            raise RuntimeError("srbh metrics run on the GPU only")
        dev = height_pred.device
        hp, hps = _plane(height_pred, H, W)
        if hps != 1:
            hp = hp.contiguous()
        lg, lps = _plane(build_logits, H, W)
        ref = height_ref.float().contiguous()
        lab = build_label.contiguous()
        if lab.dtype not in (torch.int64, torch.uint8):
            lab = lab.long()
        L = _lib.lib()
        out = torch.empty((B, C, 4), dtype=torch.float64, device=dev)
        cm = torch.empty((B, C, C), dtype=torch.int64, device=dev)
        if self._bad is None:
            self._bad = torch.zeros((), dtype=torch.int32, device=dev)
        bad = self._bad if self._bad.device == dev else torch.zeros((), dtype=torch.int32, device=dev)
        nbytes = L.srbh_eval_ws_bytes(B, H * W, C)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        qh = cl = None
        if self.keep_maps:
            qh = torch.empty((B, H, W), dtype=torch.uint16, device=dev)
            cl = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
        a = _lib.EvalArgs(height=hp.data_ptr(), height_bs=hp.stride(0), logits=lg.data_ptr(), logits_bs=lg.stride(0), logits_cs=lg.stride(1),
                          logits_ps=lps, ref=ref.data_ptr(), label=lab.data_ptr(), label_u8=int(lab.dtype == torch.uint8),
                          B=B, C=C, HW=H * W, sums=out.data_ptr(), cm=cm.data_ptr(), bad=bad.data_ptr(),
                          q_height=qh.data_ptr() if qh is not None else None, cls_map=cl.data_ptr() if cl is not None else None,
                          ws=ws.data_ptr(), ws_bytes=nbytes)
        with torch.cuda.device(dev):
            _lib.check(L.srbh_eval_sums(a, _lib.stream_ptr()), "srbh_eval_sums")
        if bad is not self._bad:
            self._bad |= bad.to(self._bad.device)
        self._sums.append(out)
        self._cm.append(cm)
        self.count += B
        return (qh, cl) if self.keep_maps else None

    def merge_(self, other):
        """append the images of `other` (another rank's evaluation, in rank order) behind this one's"""
        if other.num_class != self.num_class:
            raise ValueError("HeightEvaluation.merge_: different class counts")
        if other.count:
            dev = self._bad.device if self._bad is not None else torch.device(self.device)
            self._sums += [t.to(dev) for t in other._sums]
            self._cm += [t.to(dev) for t in other._cm]
            if self._bad is None:
                self._bad = torch.zeros((), dtype=torch.int32, device=dev)
            self._bad |= other._bad.to(dev)
            self.maps += other.maps
            self.count += other.count
        return self

    def image_sums(self):
        """(N, C, 4) float64 and (N, C, C) int64: every image's sums and confusion matrix, in arrival order, on the device"""
        C = self.num_class
        if not self.count:
            dev = torch.device(self.device)
            return torch.zeros((0, C, 4), dtype=torch.float64, device=dev), torch.zeros((0, C, C), dtype=torch.int64, device=dev)
        return torch.cat(self._sums, 0), torch.cat(self._cm, 0)

    def result(self, ref_batch=None):
        """{"loss", "rmse"}: vtest_epoch's two AverageMeter averages (train.py:333-336: mean d^2 and sqrt(mean d^2) per group of ``ref_batch``
        images, weighted by the group size); "acc_total": vtest_epoch2's (train.py:444-445: the same rmse); "seg": a filled
        metrics.SegmentationMetric; "height": a filled metrics.HeightMetric (per group and class sqrt(sum d^2 / n) * n, sum |d|, sum d, n;
        classes without pixels in a group are skipped, metrics.py:190-192); "count": the number of images.  0-dim float64 device tensors.
        Raises SegmentationMetric.check_range's ValueError if any label lay outside [0, num_class) -- the only host read."""
        C = self.num_class
        rb = self.ref_batch if ref_batch is None else int(ref_batch)
        if rb < 1:
            raise ValueError(f"HeightEvaluation.result: ref_batch must be at least 1 (got {rb})")
        sums, cm = self.image_sums()
        dev = sums.device
        seg = SegmentationMetric(C, device=dev)
        hm = HeightMetric(C, device=dev)
        N = self.count
        if self._bad is not None:
            seg._bad |= self._bad.to(torch.int64)
        seg.check_range()
        if N == 0:
            nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
            return {"loss": nan, "rmse": nan, "acc_total": nan, "seg": seg, "height": hm, "count": 0}
        G = (N + rb - 1) // rb
        if G * rb > N:
            sums = torch.cat([sums, sums.new_zeros((G * rb - N, C, 4))], 0)
        gs = sums.reshape(G, rb, C, 4).sum(1)                         # per group and class
        size = torch.tensor([min(rb, N - g * rb) for g in range(G)], dtype=torch.float64, device=dev)
        n = gs[:, :, 3]
        mse = gs[:, :, 0].sum(1) / n.sum(1)                           # torch.mean((ypred - y_true) ** 2) of a group
        loss = (mse * size).sum() / N
        rmse = (torch.sqrt(mse) * size).sum() / N
        seg.confusionMatrix += cm.sum(0).to(torch.float64)
        hm.stats[:, 0] = (torch.sqrt(gs[:, :, 0] / n.clamp_min(1.0)) * n).sum(0)      # rmse * count; a class without pixels adds 0
        hm.stats[:, 1] = gs[:, :, 1].sum(0)                                            # mae * count == sum |d|
        hm.stats[:, 2] = gs[:, :, 2].sum(0)
        hm.count[:, 0] = n.sum(0)
        return {"loss": loss, "rmse": rmse, "acc_total": rmse, "seg": seg, "height": hm, "count": N}
