"""Test infrastructure: the reference's validation / test loops restated in float64 torch on the CPU.

``evaluate`` is the loop body of vtest_epoch2 (reference train.py:436-449) plus the two averages of vtest_epoch (:333-336) over images
grouped into the loader's batches of ``ref_batch``, with SegmentationMetric.genConfusionMatrix (metrics.py:67-74), HeightMetric.addBatch
(:186-200) and AverageMeter (:143-160) written out; ``image_sums`` gives what csrc/srbh_eval.hip returns per image; ``saved_maps`` the two
rasters of issave=True (:464-478).  The only difference from the reference is the precision: differences, squares and means are float64
here where the reference subtracts and squares in fp32 (tools/make_golden_evaluate.py pins the two against each other at 1e-5).
``fixture_inputs`` are the seeded synthetic head outputs of tests/golden/g17_evaluate.npz."""
import numpy as np
import torch

NUM_CLASS = 7
REF_BATCHES = (1, 3, 4)


def fixture_inputs():
    """10 images of 24x20, 7 classes: (height, logits, ref, label) -- fp32, fp32 (10,7,24,20), fp32, uint8.
    Labels are blocky 4x4 patches; image 3 lacks classes 5 and 6, image 7 is class 0 only.  Reference heights are whole metres; predicted
    heights lie on a 1/64 m grid around them, negatives included, and ~3 % of the pixels hold k + 0.05 (2m+1) with x10 exact in fp32 and on a
    half (0.25, 0.75, 1.25, ...).  Logits lie on a 1/256 grid, and in ~2 % of the pixels the maximum is copied into a second channel."""
    rs = np.random.RandomState(17)
    B, C, H, W = 10, NUM_CLASS, 24, 20
    coarse = rs.randint(0, C, size=(B, H // 4, W // 4))
    label = np.kron(coarse, np.ones((4, 4), dtype=np.int64)).astype(np.uint8)
    label[3] = label[3] % 5
    label[7] = 0
    ref = (rs.randint(0, 40, size=(B, H, W)) * (label > 0)).astype(np.float32)
    height = (ref + np.round(rs.randn(B, H, W) * 3.0 * 64) / 64).astype(np.float32)
    halves = np.array([0.25, 0.75, 1.25, 1.75, 2.25, 6.25, 12.75], dtype=np.float32)       # x10 -> 2.5, 7.5, 12.5, 17.5, 22.5, 62.5, 127.5
    pick = rs.rand(B, H, W) < 0.03
    height[pick] = halves[rs.randint(0, len(halves), size=int(pick.sum()))]
    logits = (np.round(rs.randn(B, C, H, W) * 2.0 * 256) / 256).astype(np.float32)
    onehot = np.moveaxis(np.eye(C, dtype=np.float32)[label], -1, 1)
    logits += 1.5 * onehot                                                             # about a third of the pixels classified correctly
    tie = rs.rand(B, H, W) < 0.02
    other = rs.randint(0, C, size=(B, H, W))
    mx = logits.max(1)
    for b, r, c in zip(*np.nonzero(tie)):
        logits[b, other[b, r, c], r, c] = mx[b, r, c]
    return torch.from_numpy(height), torch.from_numpy(logits), torch.from_numpy(ref), torch.from_numpy(label)


def tie_fraction(logits):
    """fraction of the pixels whose maximum logit is held by more than one channel"""
    mx = logits.max(1, keepdim=True).values
    return float(((logits == mx).sum(1) > 1).double().mean())


def image_sums(height, logits, ref, label, num_class=NUM_CLASS):
    """(sums (B, C, 4) float64: sum d^2, sum |d|, sum d, count per label class; cm (B, C, C) int64 [label, pred]) per image; a pixel whose
    label is outside [0, C) is counted nowhere.  height (B,H,W) or (B,1,H,W)."""
    B, C = logits.shape[0], num_class
    d = height.reshape(B, -1).double() - ref.reshape(B, -1).double()
    lab = label.reshape(B, -1).long()
    pred = logits.argmax(1).reshape(B, -1)
    sums = torch.zeros((B, C, 4), dtype=torch.float64)
    cm = torch.zeros((B, C, C), dtype=torch.int64)
    for b in range(B):
        for k in range(C):
            m = lab[b] == k
            dk = d[b][m]
            sums[b, k] = torch.stack([(dk * dk).sum(), dk.abs().sum(), dk.sum(), m.sum().double()])
        ok = (lab[b] >= 0) & (lab[b] < C)
        cm[b] = torch.bincount(C * lab[b][ok] + pred[b][ok], minlength=C * C).reshape(C, C)
    return sums, cm


def saved_maps(height, logits):
    """train.py:464-466 and :476 -- (uint16 np.round(max(h, 0) * 10) in fp32, uint8 argmax), as numpy arrays (B,H,W)"""
    tmp = height.reshape(height.shape[0], *height.shape[-2:]).float().numpy().copy()
    tmp[tmp < 0] = 0
    return np.round(tmp * 10).astype("uint16"), logits.argmax(1).numpy().astype("uint8")


class AverageMeter:
    def __init__(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def evaluate(height, logits, ref, label, ref_batch, num_class=NUM_CLASS):
    """the reference loops over consecutive groups of ``ref_batch`` images (the last may be shorter), float64 throughout.  Returns float64
    tensors: loss, rmse (vtest_epoch's losses.avg / acc.avg), acc_total (vtest_epoch2's), cm (C, C), hm_stats (C, 3), hm_count (C, 1)."""
    N, C = logits.shape[0], num_class
    height = height.reshape(N, *height.shape[-2:]).double()
    ref = ref.double()
    losses, acc, acc_total = AverageMeter(), AverageMeter(), AverageMeter()
    cm = torch.zeros((C, C), dtype=torch.float64)
    stats = torch.zeros((C, 3), dtype=torch.float64)
    count = torch.zeros((C, 1), dtype=torch.float64)
    for s in range(0, N, ref_batch):
        ypred, y_true, build = height[s:s + ref_batch], ref[s:s + ref_batch], label[s:s + ref_batch].long()
        n = ypred.shape[0]
        loss = torch.mean((ypred - y_true) ** 2)
        losses.update(loss, n)
        rmse = torch.sqrt(((ypred - y_true) ** 2).mean())
        acc.update(rmse, n)
        acc_total.update(rmse, n)
        build_pred = logits[s:s + ref_batch].argmax(1)
        lin = C * build.flatten() + build_pred.flatten()                                  # genConfusionMatrix
        cm += torch.bincount(lin, minlength=C * C).reshape(C, C).double()
        for i in range(C):                                                                # HeightMetric.addBatch
            mask = build == i
            cnt = mask.sum().double()
            if int(cnt) == 0:
                continue
            dd = ypred[mask] - y_true[mask]
            stats[i, 0] += torch.sqrt((dd ** 2).mean()) * cnt
            stats[i, 1] += dd.abs().mean() * cnt
            stats[i, 2] += dd.mean() * cnt
            count[i] += cnt
    return {"loss": torch.as_tensor(losses.avg, dtype=torch.float64), "rmse": torch.as_tensor(acc.avg, dtype=torch.float64),
            "acc_total": torch.as_tensor(acc_total.avg, dtype=torch.float64), "cm": cm, "hm_stats": stats, "hm_count": count}


def derived(cm, stats, count):
    """the getters of the two metric classes that the reference writes to its text files (metrics.py:14-65, :202-215)"""
    diag = torch.diag(cm)
    union = cm.sum(1) + cm.sum(0) - diag
    each = stats / (count + 1e-10)
    return {"oa": diag.sum() / cm.sum(), "iou": diag / union, "mfwiou": ((cm.sum(1) / (cm.sum() + 1e-8)) * (diag / (union + 1e-8))).sum(),
            "hm_each": each, "hm_balance": each.mean(dim=0), "hm_all": stats.sum(dim=0) / count.sum()}


def rel_err(got, want, scale=None):
    """largest |got - want| / |want| over the entries (an entry that is 0 in `want` must be 0 in `got`; NaN entries must coincide).  scale:
    a tensor of magnitudes that the entries are sums of (sum |d| for sum d, which cancels): the error is then taken relative to
    max(|want|, scale)"""
    got, want = torch.as_tensor(got, dtype=torch.float64).cpu(), torch.as_tensor(want, dtype=torch.float64).cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    den = want.abs() if scale is None else torch.maximum(want.abs(), torch.as_tensor(scale, dtype=torch.float64).cpu().abs())
    err = (got - want).abs() / den.clamp_min(1e-300)
    err = err[~torch.isnan(want)]
    return float(err.max()) if err.numel() else 0.0
