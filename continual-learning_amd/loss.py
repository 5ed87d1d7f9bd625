"""Per-pixel cross-entropy (+ build-defined continual-learning distillation) on libclamd's fused kernel.

``CrossEntropyLoss()`` mirrors ``nn.CrossEntropyLoss()`` as the reference uses it (trainer.py:113,174): fp32 NCHW
logits, int64 [B,H,W] labels, mean over non-ignored pixels, ignore_index -100.  Forward and backward are ONE kernel
pass: the forward computes the loss and d loss / d logits; backward only scales it by the incoming gradient.

``DistillationCrossEntropy`` adds  lam * mean_px KL(softmax(z_old[:, :c_old]/T) || softmax(z[:, :c_old]/T))  (LwF-style,
SURVEY.md §8a row A12).  The reference has NO such code: this term is build-defined and its parity is
pinned only by tests against this repo's own CPU restatement.

``UnbiasedDistillationCrossEntropy`` is the class-incremental step's criterion (build-defined and parity-unpinned as well): the unbiased
cross-entropy and unbiased distillation of Cermelli et al. (CVPR 2020) as include/clamd.h states them, on ``clamd_ce_unbiased_fwd_bwd``.

``CrossEntropyLoss()(logits, labels, image_weight)`` is the pseudo-label step's loss (build-defined, pseudo.py): every pixel's term times its
image's weight, on ``clamd_ce_fwd_bwd_weighted``; without the weight nothing changes.

``CrossEntropyLoss(weight=, label_smoothing=, focal_gamma=)`` is the generalised per-pixel loss (torch's class weights and label smoothing;
the focal term build-defined) on ``clamd_ce_class_fwd_bwd``; ``class_weights`` derives the weights from per-image class pixel counts.

``DiceCrossEntropyLoss`` is cross-entropy plus soft Dice (build-defined, the compound loss of nnU-Net / MONAI's DiceCELoss), on
``clamd_ce_dice_fwd_bwd``: a sums pass, a coefficient pass and a gradient pass, every reduction in a fixed order.
"""
import collections
import os

import torch
import torch.nn as nn

from . import _lib
from ._lib import call, ptr


# d logits handed to the UNet's backward pass in the head data gradient's own layout (see _LossFn); =0: the engine converts the NCHW
# gradient as it does for any other loss (A/B measurements)
HANDOVER = os.environ.get('CLAMD_LOSS_HANDOVER', '1') != '0'

# What a criterion tells _LossFn about its library call  entry(logits, labels, <old>, <vectors>, *lead, d logits, ..., ignore_index, *tail, grad_scale):
#   old        (old_logits,) where the entry takes the old model's logits and their class count ((None,): called without them); () otherwise
#   vectors    ((tensor or None, 'image_weight' | 'class weights'), ...): per-image / per-class fp32 factors, checked by _vector
#   lead, tail the numbers behind those / between ignore_index and grad_scale
#   px_bytes, px_logits   what the entry reads per pixel beyond the logits and the label: bytes, and further reads of the K logits
#   count      clamd_ce_count runs in front (False: the entry counts for itself)
#   ws_bytes   ``ws_bytes(lib, B, K, H, W)``: the size of a workspace larger than the cross-entropy one (which it starts with)
#   handover   False: clamd_ce_fwd_bwd's argument list -- no NHWC copy of d logits, nothing handed to the UNet
_Launch = collections.namedtuple('_Launch', 'entry old vectors lead tail px_bytes px_logits count ws_bytes handover',
                                 defaults=((), (), (), (), 0, 0, True, None, True))
_PLAIN = _Launch('clamd_ce_fwd_bwd_counted')


def _any_size(old_logits=None, c_old=0, temperature=1.0, lam=0.0):
    """clamd_ce_fwd_bwd: the temperature-distillation term, odd sizes, misaligned storage"""
    return _Launch('clamd_ce_fwd_bwd', (old_logits,), lead=(int(c_old), float(temperature), float(lam)), count=False, handover=False)


_VECTORS = {'image_weight': (0, ' (one factor per image)'), 'class weights': (1, '')}      # -> (the logits dimension it spans, the message's note)


def _vector(t, what, shape):
    """-> `t` contiguous (None stays None); ValueError unless it is float32 with one entry per image / per class of logits `shape`"""
    if t is None:
        return None
    dim, note = _VECTORS[what]
    if t.dtype != torch.float32 or tuple(t.shape) != (shape[dim],):
        raise ValueError(f'{what} must be float32 [{shape[dim]}]{note}, got {t.dtype} {tuple(t.shape)}')
    return t.contiguous()


def _old_logits(old_logits, logits):
    """-> (contiguous fp32 old_logits or None, its class count)"""
    if old_logits is None:
        return None, 0
    old_logits = old_logits.contiguous().float()
    B, _, H, W = logits.shape
    if old_logits.dim() != 4 or old_logits.shape[0] != B or tuple(old_logits.shape[2:]) != (H, W):
        raise ValueError('old_logits must be [B, K_old, H, W]')
    return old_logits, old_logits.shape[1]


class _LossFn(torch.autograd.Function):
    """Every criterion's forward and backward: the checks, the allocation, [clamd_ce_count and] the entry point `launch` names, and the
    bookkeeping behind the kernels.  `holder`: the criterion; it supplies ignore_index and receives `parts` and `bad_labels`."""

    @staticmethod
    def forward(ctx, logits, labels, holder, launch):
        ignore_index = int(holder.ignore_index)
        others = launch.old + tuple(t for t, _ in launch.vectors)
        if not all(t.is_cuda for t in (logits, labels) + others if t is not None):
            raise RuntimeError('continual-learning_amd loss runs only on GPU tensors: there is no CPU fallback')
        lib = _lib.load()
        logits_in = logits
        logits = logits.contiguous().float()
        labels = labels.contiguous()
        if labels.dtype != torch.int64:
            raise TypeError('labels must be int64 (datasets/voc.py:72)')
        B, K, H, W = logits.shape
        if tuple(labels.shape) != (B, H, W):
            raise ValueError(f'labels shape {tuple(labels.shape)} does not match logits {tuple(logits.shape)}')
        dl = torch.empty_like(logits)
        out3 = torch.empty(3, dtype=torch.float32, device=logits.device)
        wsb = lib.clamd_ce_workspace_bytes() if launch.ws_bytes is None else launch.ws_bytes(lib, B, K, H, W)
        ws = torch.empty(wsb // 4, dtype=torch.float32, device=logits.device)
        ctx.sink = None
        # the four-pixel kernels read 16 bytes of logits / 32 bytes of labels per lane: an odd storage offset takes the scalar kernel
        aligned = logits.data_ptr() % 16 == 0 and dl.data_ptr() % 16 == 0 and labels.data_ptr() % 32 == 0
        if launch is _PLAIN and not ((H * W) % 4 == 0 and aligned):
            launch = _any_size()
        held = [_old_logits(t, logits) for t in launch.old]                       # (tensor, class count); held until the launch
        vectors = [_vector(t, what, logits.shape) for t, what in launch.vectors]
        lead = tuple(a for t, kold in held for a in (ptr(t), kold)) + tuple(ptr(t) for t in vectors) + launch.lead
        shape = (B, K, H, W, ignore_index)
        if not launch.handover:
            call(launch.entry, ptr(logits), ptr(labels), *lead, ptr(dl), ptr(out3), ptr(ws), wsb, *shape, *launch.tail, 1.0, _lib.stream_ptr())
        else:
            # the training-step form: the count of valid pixels as partial rows (no memset, no atomics), and, when the logits come from this
            # package's UNet, d logits written a second time in the layout (and dtype) its 1x1 head's data gradient reads -- the backward
            # pass then starts without a conversion pass (unet._Engine.backward)
            from . import unet as U
            # (algorithmic bytes, SURVEY 8d: logits read + d logits written + the label; the counting pass reads the labels a second time)
            if launch.count:
                U._hbm('loss', 0, 'clamd_ce_count', ptr(labels), *shape, ptr(ws), wsb, _lib.stream_ptr())
            eng = U.dlogits_sink(logits_in, B, K, H, W) if HANDOVER else None
            nh, ldc, dcode = (eng.dl, eng.Kp, eng.dcode) if eng is not None else (None, 0, 0)
            px = (2 + launch.px_logits) * K * 4 + launch.px_bytes + 8 + (ldc * eng.esize if eng is not None else 0)
            U._hbm('loss', B * H * W * px, launch.entry, ptr(logits), ptr(labels), *lead, ptr(dl), ptr(nh), ldc, dcode, ptr(out3), ptr(ws), wsb,
                   *shape, *launch.tail, 1.0, _lib.stream_ptr())
            if eng is not None:
                ctx.sink = eng
                # a STRONG reference: while the engine waits for this gradient its storage cannot be freed and handed to another
                # tensor of the same shape (a second loss on the same logits would otherwise pass for this one by address)
                eng.dl_src = (dl, dl.data_ptr(), dl._version, eng.generation)
        ctx.save_for_backward(dl)
        ctx.parts = out3
        # labels outside [0, K) that are not ignore_index: a device counter on the criterion (int(...) synchronises);
        # torch's CrossEntropyLoss asserts on such labels, here they are left out of the mean and counted
        off = lib.clamd_ce_bad_label_count_offset() // 4
        holder.bad_labels = ws[off:off + 1].view(torch.int32)
        holder.parts = out3
        return out3[0]

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        # g is the scalar upstream gradient on the DEVICE (exactly 1 for loss.backward()): the kernel tests it there and
        # touches d logits only when it is not 1 -- no host sync, no 176-MB multiply-by-one pass per step
        g = g.contiguous().float()
        eng = ctx.sink
        if eng is not None and eng.dl_src is not None and eng.dl_src[1] == dl.data_ptr():      # the NHWC copy follows: both in one launch
            call('clamd_scale_by_device_scalar_nhwc', ptr(eng.dl), eng.dl.numel(), eng.dcode, ptr(g), ptr(dl), dl.numel(), _lib.stream_ptr())
        else:
            call('clamd_scale_by_device_scalar', ptr(dl), dl.numel(), ptr(g), _lib.stream_ptr())
        return dl, None, None, None


class CrossEntropyLoss(nn.Module):
    """``nn.CrossEntropyLoss(weight=, ignore_index=, label_smoothing=)`` with mean reduction, plus ``focal_gamma`` (build-defined: the focal
    modulation q^gamma of Lin et al. with q = 1 - p_y; not together with label smoothing).  With the three keyword arguments at their
    defaults the forward is the plain loss on the entry points it always used; any of them set takes ``clamd_ce_class_fwd_bwd`` (the
    definition is in include/clamd.h).  ``weight``: K finite numbers >= 0, kept as a non-persistent fp32 buffer (``.to(device)`` moves it;
    ``set_weight`` replaces it); None with smoothing or the focal term means unit weights.  The weighted mean divides by the sum of the valid
    pixels' class weights, as torch does; where that sum is 0 the loss and every gradient are 0 (torch: NaN).  After a forward: ``parts`` =
    device {loss, (1 - eps) nll / D, (eps / K) smo / D}, ``bad_labels`` = device int32[1]."""

    def __init__(self, ignore_index=-100, *, weight=None, label_smoothing=0.0, focal_gamma=0.0):
        super().__init__()
        self.ignore_index = ignore_index
        self.label_smoothing, self.focal_gamma = check_smoothing_and_gamma(label_smoothing, focal_gamma)
        self.register_buffer('weight', None, persistent=False)
        self.set_weight(weight)
        self.bad_labels = None        # after a forward: device int32[1], labels that are neither ignore_index nor a class
        self.parts = None
        self._unit = None             # the unit weights of smoothing / focal without `weight` (forward)

    def set_weight(self, weight):
        """Replaces the class weights (None: none); checked on the host: one dimension, finite, >= 0.  The length is checked against the
        logits at the next forward."""
        if weight is not None:
            dev = self.weight.device if self.weight is not None else getattr(weight, 'device', None)
            weight = check_class_weight(weight).to(dev or 'cpu')
        self.weight = weight

    @property
    def generalised(self):
        return self.weight is not None or self.label_smoothing > 0.0 or self.focal_gamma > 0.0

    def forward(self, logits, labels, image_weight=None):
        """image_weight (fp32 [B] on the device, e.g. PseudoLabeler's nu): every pixel's term and gradient times its image's weight, the mean
        still over the unweighted count of valid pixels (clamd_ce_fwd_bwd_weighted; build-defined) or, with class weights, over their
        unweighted sum D.  None: the plain loss."""
        if self.generalised:
            K = logits.shape[1]
            w = self.weight
            if w is None:             # unit weights: one vector per (K, device), kept -- no allocation or fill launch per step
                w = self._unit
                if w is None or w.numel() != K or w.device != logits.device:
                    w = self._unit = torch.ones(K, dtype=torch.float32, device=logits.device)
            elif w.numel() != K:
                raise ValueError(f'CrossEntropyLoss: weight has {w.numel()} entries, the logits have {K} classes')
            nu = None if image_weight is None else image_weight.detach()
            # clamd_ce_class_fwd_bwd counts for itself: the labels a second time (the K + B weights do not count as traffic)
            return _LossFn.apply(logits, labels, self, _Launch(
                'clamd_ce_class_fwd_bwd', vectors=((w, 'class weights'), (nu, 'image_weight')), tail=(float(self.label_smoothing), float(self.focal_gamma)),
                px_bytes=8, count=False, ws_bytes=lambda lib, *shape: lib.clamd_ce_class_workspace_bytes()))
        if image_weight is not None:
            return _LossFn.apply(logits, labels, self, _Launch('clamd_ce_fwd_bwd_weighted', vectors=((image_weight.detach(), 'image_weight'),)))
        return _LossFn.apply(logits, labels, self, _PLAIN)


def check_smoothing_and_gamma(label_smoothing, focal_gamma):
    """-> (float, float); ValueError outside [0, 1) / [0, inf) or with both non-zero."""
    eps, gamma = float(label_smoothing), float(focal_gamma)
    if not 0.0 <= eps < 1.0:
        raise ValueError(f'label_smoothing must be in [0, 1), got {label_smoothing!r}')
    if not (gamma >= 0.0 and gamma != float('inf')):
        raise ValueError(f'focal_gamma must be finite and >= 0, got {focal_gamma!r}')
    if eps > 0.0 and gamma > 0.0:
        raise ValueError('label_smoothing and focal_gamma are both non-zero: the combination is not defined (clamd_ce_class_fwd_bwd)')
    return eps, gamma


MIN_POSITIVE_WEIGHT = 1e-30      # the smallest positive class weight (include/clamd.h)


def check_class_weight(weight, num_classes=None):
    """-> a detached fp32 [K] tensor of `weight` (a tensor or a sequence of numbers); ValueError unless one-dimensional, non-empty, finite,
    each entry 0 or >= MIN_POSITIVE_WEIGHT, and (when given) of length num_classes.  Reads the values: call it when the weights are set, not per step."""
    w = torch.as_tensor(weight).detach().to(torch.float32)
    if w.dim() != 1 or w.numel() == 0:
        raise ValueError(f'class weights must be a non-empty vector, got shape {tuple(w.shape)}')
    if num_classes is not None and w.numel() != int(num_classes):
        raise ValueError(f'class weights must have {int(num_classes)} entries (one per class), got {w.numel()}')
    if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
        raise ValueError('class weights must be finite and >= 0')
    if bool(((w > 0) & (w < MIN_POSITIVE_WEIGHT)).any()):      # 1 / (float)D must stay finite: D >= the smallest positive weight
        raise ValueError(f'a class weight must be 0 or at least {MIN_POSITIVE_WEIGHT:g} (include/clamd.h: grad_scale / D is formed in fp32)')
    return w.clone()


def class_weights(counts, scheme, normalize=False):
    """Class weights from per-image class pixel counts: `counts` an integer [N, K] tensor (``replay.class_pixel_counts`` over a loader,
    concatenated).  -> fp32 [K] on the CPU, computed in float64.
      'median_frequency'  (Eigen & Fergus, ICCV 2015)  freq_k = n_k / (pixels of the images that contain k),  w_k = median(freq) / freq_k
      'inverse_log'       (ENet, Paszke et al. 2016)   w_k = 1 / ln(1.02 + n_k / sum n)
    n_k = the class's pixels over all images; the median is over the classes that occur; a class that never occurs gets 1.0.
    normalize: rescaled to mean 1 over the classes that occur."""
    c = torch.as_tensor(counts)
    if c.dim() != 2 or c.is_floating_point() or c.is_complex() or c.dtype == torch.bool:
        raise ValueError(f'counts must be an integer [N, K] tensor, got {c.dtype} {tuple(c.shape)}')
    c = c.detach().cpu().to(torch.int64)
    if bool((c < 0).any()):
        raise ValueError('counts must be >= 0')
    n = c.sum(0).double()
    present = n > 0
    w = torch.ones(c.shape[1], dtype=torch.float64)
    if bool(present.any()):
        if scheme == 'median_frequency':
            per_image = c.sum(1, keepdim=True)                                   # the image's labelled pixels
            support = (per_image * (c > 0)).sum(0).double()                      # pixels of the images that contain the class
            freq = n[present] / support[present]
            fs = freq.sort().values                                              # the median of an even number: the middle pair's mean
            w[present] = 0.5 * (fs[(fs.numel() - 1) // 2] + fs[fs.numel() // 2]) / freq
        elif scheme == 'inverse_log':
            w[present] = 1.0 / torch.log(1.02 + n[present] / n.sum())
        else:
            raise ValueError(f"scheme must be 'median_frequency' or 'inverse_log', not {scheme!r}")
        if normalize:
            w[present] = w[present] / w[present].mean()
    elif scheme not in ('median_frequency', 'inverse_log'):
        raise ValueError(f"scheme must be 'median_frequency' or 'inverse_log', not {scheme!r}")
    return w.float()


class DistillationCrossEntropy(nn.Module):
    """CE(logits, labels) + lam * KL(old || new) over the first ``c_old`` classes at temperature T."""

    def __init__(self, c_old, temperature=2.0, lam=1.0, ignore_index=-100):
        super().__init__()
        self.c_old, self.temperature, self.lam, self.ignore_index = c_old, temperature, lam, ignore_index

    def forward(self, logits, labels, old_logits):
        return _LossFn.apply(logits, labels, self, _any_size(old_logits.detach(), self.c_old, self.temperature, self.lam))


class UnbiasedDistillationCrossEntropy(nn.Module):
    """Unbiased cross-entropy + lam * unbiased distillation over the old classes [0, c_old) (class 0 = background); build-defined, parity
    unpinned.  A label below c_old means "background or any old class"; the old model's background is compared with the new model's
    background-or-new-class mass.  ``old_logits`` None: the cross-entropy term alone.  After a forward: ``parts`` = device {total, ce, kd},
    ``bad_labels`` as on CrossEntropyLoss."""

    def __init__(self, c_old, lam=10.0, ignore_index=-100):
        super().__init__()
        if c_old < 1:
            raise ValueError('c_old must be >= 1 (class 0, the background, is always an old class)')
        self.c_old, self.lam, self.ignore_index = int(c_old), float(lam), ignore_index
        self.bad_labels = None
        self.parts = None

    def forward(self, logits, labels, old_logits=None):
        old = None if old_logits is None else old_logits.detach()
        # algorithmic bytes: the c_old old-model logits on top of the plain loss's
        return _LossFn.apply(logits, labels, self, _Launch('clamd_ce_unbiased_fwd_bwd', (old,), lead=(self.c_old, self.lam),
                                                           px_bytes=4 * self.c_old if old is not None and self.lam != 0 else 0))


class DiceCrossEntropyLoss(nn.Module):
    """ce_weight * CE + dice_weight * soft Dice (build-defined; the definitions are in include/clamd.h): the compound loss of nnU-Net and of
    MONAI's DiceCELoss on ``clamd_ce_dice_fwd_bwd``.  The Dice term is computed from softmax probabilities over the valid pixels (label not
    ``ignore_index`` and inside [0, K)), per class over the whole batch or (``per_image``) over each image, averaged over the classes that
    take part: all of them, without the background (``include_background=False``), only those present in the group's labels
    (``present_only``).  After a forward: ``parts`` = device {total, ce_weight * ce, dice_weight * dice}, ``bad_labels`` as on
    CrossEntropyLoss.  Data parallelism: each rank's Dice sums cover its own batch (like non-synchronised BatchNorm); no collective is added."""

    def __init__(self, ce_weight=1.0, dice_weight=1.0, smooth=1e-5, include_background=True, present_only=True, per_image=False,
                 ignore_index=-100):
        super().__init__()
        for name, v in (('ce_weight', ce_weight), ('dice_weight', dice_weight), ('smooth', smooth)):
            if not (float(v) >= 0.0 and float(v) != float('inf')):
                raise ValueError(f'DiceCrossEntropyLoss: {name} must be finite and >= 0, got {v!r}')
        if float(ce_weight) == 0.0 and float(dice_weight) == 0.0:
            raise ValueError('DiceCrossEntropyLoss: ce_weight and dice_weight are both zero')
        self.ce_weight, self.dice_weight, self.smooth = float(ce_weight), float(dice_weight), float(smooth)
        self.include_background, self.present_only, self.per_image = bool(include_background), bool(present_only), bool(per_image)
        self.ignore_index = ignore_index
        self.bad_labels = None
        self.parts = None

    def forward(self, logits, labels):
        def ws_bytes(lib, B, K, H, W):
            n = lib.clamd_ce_dice_workspace_bytes(B, K, H, W, int(self.per_image))
            if n == 0:
                raise ValueError(f'DiceCrossEntropyLoss: logits {(B, K, H, W)}: needs 1 <= K <= 32 classes and at most 2048 images')
            return n
        # clamd_ce_dice_fwd_bwd counts for itself; algorithmic bytes: the logits and the label a second time on top of the plain loss's
        return _LossFn.apply(logits, labels, self, _Launch(
            'clamd_ce_dice_fwd_bwd', tail=(self.ce_weight, self.dice_weight, self.smooth, 0 if self.include_background else 1, int(self.present_only),
                                           int(self.per_image)), px_bytes=8, px_logits=1, count=False, ws_bytes=ws_bytes))
