"""Pseudo-labels for the old classes in the task step (build-defined, parity unpinned: the reference has no continual-learning code).

In a task-2 batch every pixel of an old class is labelled 0 -- the new task's annotation only knows the new classes.  The classification
half of PLOP (Douillard et al., CVPR 2021, section 3.2), as include/clamd.h defines it: the frozen old model labels the background pixels
it is confident about (normalised entropy below the per-class median, calibrated once on the new task's data), the others are ignored, and
each image's loss is scaled by the share of its background that was accepted (``CrossEntropyLoss(..., image_weight=nu)``).

    lab = PseudoLabeler(c_old).calibrate(old_model, loader, device)         # or accumulate(...) per batch, then finish()
    labels2, nu = lab(old_model(x), labels)
    loss = CrossEntropyLoss()(model(x), labels2, nu)

Both passes run on libclamd's kernels (clamd_pseudo_entropy_hist, clamd_pseudo_label); the thresholds come from the tiny histogram with
integer arithmetic in torch (``thresholds_from_histogram``), after an all-reduce under data parallelism so that every rank derives the same.
"""
import torch

from . import _lib
from ._lib import ptr


def thresholds_from_histogram(hist, bins=None):
    """[c_old, bins] integer histogram -> float32 [c_old] thresholds (on hist's device; CPU tensors work): tau_c = (j* + 1) / bins with j*
    the smallest j whose cumulative count reaches ceil(n_c / 2) -- the class's median entropy rounded up to a bin edge -- and 0 for a class
    without pixels."""
    if hist.dim() != 2 or hist.dtype.is_floating_point:
        raise ValueError('hist must be an integer [c_old, bins] tensor')
    bins = hist.shape[1] if bins is None else int(bins)
    if hist.shape[1] != bins:
        raise ValueError(f'hist has {hist.shape[1]} bins, expected {bins}')
    h = hist.to(torch.int64)
    n = h.sum(1)
    half = (n + 1) // 2
    jstar = (h.cumsum(1) < half[:, None]).sum(1)          # the number of bins whose cumulative count is still short = the first that reaches it
    tau = (jstar + 1).to(torch.float64) / bins
    return torch.where(n > 0, tau, torch.zeros_like(tau)).to(torch.float32)


class PseudoLabeler:
    """thresholds: a float or a [c_old] tensor fixes them and skips the calibration.  adaptive: __call__ also returns nu (float32 [B]),
    the accepted share of each image's background, at least min_factor.  After a call ``counts`` holds the device int32 [B, 2] {n_bg, n_acc}."""

    def __init__(self, c_old, bins=100, adaptive=True, min_factor=0.0, ignore_index=-100, thresholds=None):
        if not 1 <= int(c_old) <= 32:
            raise ValueError('c_old must be in [1, 32]')
        if int(bins) < 1 or int(c_old) * int(bins) > 8192:
            raise ValueError('bins must be >= 1 and c_old * bins <= 8192')
        if not min_factor >= 0.0:
            raise ValueError('min_factor must be >= 0')
        self.c_old, self.bins, self.adaptive = int(c_old), int(bins), bool(adaptive)
        self.min_factor, self.ignore_index = float(min_factor), int(ignore_index)
        self.hist = None               # this rank's calibration histogram
        self.hist_total = None         # what finish() derived the thresholds from (the sum over the ranks)
        self.counts = None
        self.thresholds = None
        if thresholds is not None:
            t = torch.as_tensor(thresholds, dtype=torch.float32)
            self.thresholds = t.expand(self.c_old).clone() if t.dim() == 0 else t.clone()
            if tuple(self.thresholds.shape) != (self.c_old,):
                raise ValueError(f'thresholds must be a float or a [{self.c_old}] tensor')

    def _check(self, old_logits, labels):
        if not old_logits.is_cuda or not labels.is_cuda:
            raise RuntimeError('continual-learning_amd pseudo-labelling runs only on GPU tensors: there is no CPU fallback')
        if labels.dtype != torch.int64:
            raise TypeError('labels must be int64 (datasets/voc.py:72)')
        if old_logits.dim() != 4 or old_logits.shape[1] < self.c_old:
            raise ValueError(f'old_logits must be [B, K_old >= {self.c_old}, H, W]')
        B, Ko, H, W = old_logits.shape
        if tuple(labels.shape) != (B, H, W):
            raise ValueError(f'labels shape {tuple(labels.shape)} does not match old_logits {tuple(old_logits.shape)}')
        return old_logits.detach().contiguous().float(), labels.contiguous(), B, Ko, H, W

    def accumulate(self, old_logits, labels):
        """Adds one batch to the calibration histogram ``hist`` (device int64 [c_old, bins])."""
        zo, y, B, Ko, H, W = self._check(old_logits, labels)
        if self.hist is None:
            self.hist = torch.zeros(self.c_old, self.bins, dtype=torch.int64, device=zo.device)
        from . import unet as U
        # algorithmic bytes: the c_old old-model logits and the label of every pixel
        U._hbm('pseudo', B * H * W * (4 * self.c_old + 8), 'clamd_pseudo_entropy_hist', ptr(zo), Ko, self.c_old, ptr(y), ptr(self.hist),
               self.bins, B, H, W, _lib.stream_ptr())
        return self

    def finish(self, group=None):
        """Thresholds from the accumulated histogram; under an initialised process group from its sum over the ranks, so every rank derives
        the same.  ``hist`` stays this rank's own counts (``hist_total`` holds the sum the thresholds came from): accumulate() and finish()
        may be called again without counting the other ranks' pixels twice."""
        if self.hist is None:
            raise RuntimeError('PseudoLabeler.finish: no batch was accumulated')
        total = self.hist
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            total = self.hist.clone()
            torch.distributed.all_reduce(total, op=torch.distributed.ReduceOp.SUM, group=group)
        self.hist_total = total
        self.thresholds = thresholds_from_histogram(total, self.bins)
        return self

    @torch.no_grad()
    def calibrate(self, old_model, loader, device, max_batches=None, group=None):
        """The old model's eval-mode forward + accumulate over a loader of (images, labels) -- the NEW task's data --, then finish."""
        modes = [(mod, mod.training) for mod in old_model.modules()]
        old_model.eval()
        try:
            for i, (images, masks) in enumerate(loader):
                if max_batches is not None and i >= max_batches:
                    break
                self.accumulate(old_model(images.to(device, non_blocking=True)), masks.to(device, non_blocking=True))
        finally:
            for mod, mode in modes:
                mod.training = mode
        return self.finish(group)

    def __call__(self, old_logits, labels):
        """-> (labels_out, nu or None).  labels is not modified."""
        if self.thresholds is None:
            raise RuntimeError('PseudoLabeler has no thresholds yet: calibrate() (or accumulate() ... finish()) first, or pass thresholds=')
        zo, y, B, Ko, H, W = self._check(old_logits, labels)
        if self.thresholds.device != zo.device:
            self.thresholds = self.thresholds.to(zo.device)
        out = torch.empty_like(y)
        self.counts = torch.empty(B, 2, dtype=torch.int32, device=zo.device)
        nu = torch.empty(B, dtype=torch.float32, device=zo.device) if self.adaptive else None
        from . import unet as U
        # algorithmic bytes: the c_old old-model logits, the label read and the label written
        U._hbm('pseudo', B * H * W * (4 * self.c_old + 16), 'clamd_pseudo_label', ptr(zo), Ko, self.c_old, ptr(y), ptr(self.thresholds), ptr(out),
               ptr(self.counts), ptr(nu), self.min_factor, B, H, W, self.ignore_index, _lib.stream_ptr())
        return out, nu
