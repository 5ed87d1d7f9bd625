"""Local POD distillation (build-defined, parity unpinned: the reference has no continual-learning code).

The distillation half of PLOP (Douillard et al., CVPR 2021, section 3.1), as include/clamd.h defines it: the new model's tensor and the
frozen old model's are pooled into row and column strips at 1, 2 and 4 regions per side, the strips of every level and channel are
concatenated into one embedding per image (L2-normalised), and the loss is the mean distance between the two embeddings.  It is the one
term of the task step that distils spatial structure instead of per-pixel class probabilities.

    pod = LocalPODLoss(levels=3, lam=0.5)
    loss = criterion(logits, labels) + pod(logits, old_logits, channels=c_old, merge_extra=True)      # the logits form
    loss = loss + LocalPODLoss(square=True)(model.enc1(x), old_model.enc1(x))                         # a feature level (blocks.py)

One launch sequence (clamd_local_pod_fwd_bwd) computes the loss and d loss / d new in the forward; backward only scales the kept gradient by
the upstream device scalar.  Any fp32 NCHW GPU tensor pair of equal batch and spatial size works; there is no CPU path.
"""
import torch
import torch.nn as nn

from . import _lib
from ._lib import call, ptr


def _check(new, old, channels, levels):
    """-> (contiguous fp32 new, old, B, Ca, Cb, C, H, W)"""
    if not new.is_cuda or not old.is_cuda:
        raise RuntimeError('continual-learning_amd Local POD runs only on GPU tensors: there is no CPU fallback')
    if new.dim() != 4 or old.dim() != 4 or new.shape[0] != old.shape[0] or tuple(new.shape[2:]) != tuple(old.shape[2:]):
        raise ValueError(f'new and old must be [B, Ca, H, W] and [B, Cb, H, W], got {tuple(new.shape)} and {tuple(old.shape)}')
    B, Ca, H, W = new.shape
    Cb = old.shape[1]
    C = min(Ca, Cb) if channels is None else int(channels)
    if not 1 <= C <= min(Ca, Cb):
        raise ValueError(f'channels must be in [1, min(Ca, Cb)] = [1, {min(Ca, Cb)}], got {C}')
    k = 1 << (levels - 1)
    if H % k or W % k:
        raise ValueError(f'H and W must be multiples of 2^(levels-1) = {k}, got {H} x {W}')
    return new.contiguous().float(), old.contiguous().float(), B, Ca, Cb, C, H, W


class _PODFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, new, old, C, merge_extra, square, normalize, levels, lam):
        lib = _lib.load()
        B, Ca, H, W = new.shape
        Cb = old.shape[1]
        da = torch.empty_like(new) if ctx.needs_input_grad[0] else None
        loss = torch.empty(1, dtype=torch.float32, device=new.device)
        wsb = lib.clamd_pod_workspace_bytes(B, C, H, W, levels)
        ws = torch.empty(wsb // 4, dtype=torch.float32, device=new.device)
        from . import unet as U
        # algorithmic bytes: the compared channels of both tensors read (the merged ones too), d new written (and new read again for 2 x)
        read = (C + (Ca - C if merge_extra else 0)) + C
        nbytes = 4 * B * H * W * (read + (Ca + (read - C if square else 0) if da is not None else 0))
        U._hbm('pod', nbytes, 'clamd_local_pod_fwd_bwd', ptr(new), Ca, ptr(old), Cb, C, int(merge_extra), int(square), int(normalize), levels,
               float(lam), ptr(da), ptr(loss), ptr(ws), wsb, B, H, W, 1.0, _lib.stream_ptr())
        ctx.da = da
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        da, ctx.da = ctx.da, None
        if da is None:
            return (None,) * 8
        # the upstream gradient stays on the device (exactly 1 for loss.backward(): the kernel then touches nothing)
        call('clamd_scale_by_device_scalar', ptr(da), da.numel(), ptr(g.contiguous().float()), _lib.stream_ptr())
        return (da,) + (None,) * 7


class LocalPODLoss(nn.Module):
    """lam * mean_n || e(new_n) - e(old_n) ||_2 over the strip-pooled embeddings e (include/clamd.h).  levels: 1, 2 or 3 scales (1, 2, 4
    regions per side; H and W must be multiples of 2^(levels-1)); square: pool x^2 (post-ReLU features); normalize: L2-normalise each
    image's embedding."""

    def __init__(self, levels=3, square=False, normalize=True, lam=1.0):
        super().__init__()
        if int(levels) not in (1, 2, 3):
            raise ValueError('levels must be 1, 2 or 3')
        self.levels, self.square, self.normalize, self.lam = int(levels), bool(square), bool(normalize), float(lam)

    def forward(self, new, old, channels=None, merge_extra=False):
        """channels: compare the first `channels` channels (default min(Ca, Cb)).  merge_extra: channel 0 of `new` is taken as the sum of
        its channel 0 and its channels >= `channels` -- the logits form, the old background against the new background plus new classes.
        `old` is detached; the gradient reaches `new` alone."""
        a, b, B, Ca, Cb, C, H, W = _check(new, old.detach(), channels, self.levels)
        return _PODFn.apply(a, b, C, bool(merge_extra), self.square, self.normalize, self.levels, self.lam)
