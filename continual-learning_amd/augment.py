"""On-device training augmentation (build-defined, parity unpinned: the reference stops at Pad + CenterCrop + Normalize).

The published continual-segmentation recipes (MiB, PLOP) train on randomly rescaled (0.5 - 2), cropped or padded, and flipped batches.  Here
that is ONE launch over the image batch and its label batch (clamd_augment_batch, include/clamd.h states the definition): every coordinate
is a 64-bit integer in Q16, so which label a pixel takes and which pixels are padding never depends on floating-point rounding -- the label
map never goes through float, and the image's fill region and the labels' ignore region are the same pixels by construction.

    aug = RandomScaleCrop(scale=(0.5, 2.0), flip=True, ignore_index=-100, seed=0)
    x, y = aug(images, labels)                            # draw(B, H, W) from a device generator, then augment_batch; no host sync
    x, y = augment_batch(images, labels, params)          # params int64 [B, 4] = {step, y0, x0, flags}, e.g. from params_from_draws

Data parallelism: each rank draws with ``seed + rank`` (Trainer.build_model passes that seed); no collective is added.
"""
import functools

import torch

from . import _lib
from ._lib import ptr

STEP_ONE = 1 << 16                       # Q16: the source pitch of scale 1
STEP_MIN, STEP_MAX = 1 << 13, 1 << 19    # what the kernel accepts: scale 8 ... 1/8
Q_ONE = 256                              # the scale's grid: q / 256
MAX_SIZE = 4096


def _hbm(nbytes, name, *args):
    from . import unet as U
    U._hbm('augment', nbytes, name, *args)


def augment_batch(images, labels, params, fill=0.0, ignore_index=-100, out=None):
    """-> (images', labels') in one launch (clamd_augment_batch): images fp32 [B, C, H, W] and labels int64 [B, H, W] resampled, cropped or
    padded and flipped by params (device int64 [B, 4] = {step, y0, x0, flags}: include/clamd.h).  Pixels outside the source are ``fill`` /
    ``ignore_index``.  Either of images / labels may be None (its result is None too).  ``out``: (out_images, out_labels) to write into
    instead of fresh tensors -- contiguous, of the inputs' shapes and dtypes, not overlapping them (a view at a storage offset takes the
    one-pixel path).  The guard counter (rows whose step was outside [2^13, 2^19]: all fill, all ignore) is returned as ``.bad_params`` of
    the label tensor (and of the image tensor): device int32 [1]; int(...) synchronises.  No host synchronisation otherwise."""
    if images is None and labels is None:
        raise ValueError('augment_batch: neither images nor labels')
    for t in (images, labels, params):
        if t is not None and not t.is_cuda:
            raise RuntimeError('continual-learning_amd augmentation runs only on GPU tensors: there is no CPU fallback')
    if images is not None and (images.dtype != torch.float32 or images.dim() != 4):
        raise TypeError('images must be a float32 [B, C, H, W] tensor')
    if labels is not None and (labels.dtype != torch.int64 or labels.dim() != 3):
        raise TypeError('labels must be an int64 [B, H, W] tensor (datasets/voc.py:72)')
    if images is not None and labels is not None and (images.shape[0],) + tuple(images.shape[2:]) != tuple(labels.shape):
        raise ValueError(f'expected images [B, C, H, W] and labels [B, H, W], got {tuple(images.shape)} and {tuple(labels.shape)}')
    B, H, W = (labels.shape if labels is not None else (images.shape[0],) + tuple(images.shape[2:]))
    C = images.shape[1] if images is not None else 1
    if params.dtype != torch.int64 or tuple(params.shape) != (B, 4):
        raise TypeError(f'params must be an int64 [{B}, 4] tensor of (step, y0, x0, flags)')
    dev = params.device
    x = images if images is None or images.is_contiguous() else images.contiguous()     # a view at a storage offset stays as it is
    y = labels if labels is None or labels.is_contiguous() else labels.contiguous()
    p = params if params.is_contiguous() else params.contiguous()
    if out is not None:
        out_x, out_y = out
        for o, i, what in ((out_x, x, 'out_images'), (out_y, y, 'out_labels')):
            if (o is None) != (i is None):
                raise ValueError(f'augment_batch: {what} goes with its input')
            if o is not None and (o.shape != i.shape or o.dtype != i.dtype or o.device != i.device or not o.is_contiguous()):
                raise ValueError(f'augment_batch: {what} must be a contiguous tensor of its input\'s shape, dtype and device')
    else:
        out_x = None if x is None else torch.empty_like(x)
        out_y = None if y is None else torch.empty_like(y)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    # algorithmic bytes: every output pixel written, as many source bytes read (scale 1; a zoom reads fewer, a zoom-out pads)
    nbytes = B * H * W * ((8 * C if x is not None else 0) + (16 if y is not None else 0))
    _hbm(nbytes, 'clamd_augment_batch', ptr(x), ptr(y), ptr(p), B, C, H, W, ptr(out_x), ptr(out_y), float(fill), int(ignore_index), ptr(bad),
         _lib.stream_ptr())
    for o in (out_x, out_y):
        if o is not None:
            o.bad_params = bad
    return out_x, out_y


def step_from_q(q):
    """Q16 source pitch of scale q / 256, rounded to nearest: (2^24 + q // 2) // q.  q a Python int or an int64 tensor."""
    return ((1 << 24) + q // 2) // q


@functools.lru_cache(maxsize=16)
def _sizes(H, W, device):
    """int64 [2] = (H, W) on the device, built there (a tensor from a host list would be a synchronising copy), once per shape."""
    return torch.arange(2, device=device) * (W - H) + H


def params_from_draws(q, ry, rx, flip, H, W):
    """Draws -> params int64 [B, 4] = {step, y0, x0, flags}, in int64 torch arithmetic on the draws' device (CPU tensors work too).
    q [B]: the scale in 1/256 steps (32 ... 2048); ry, rx [B] in [0, 2^31): where the window sits; flip [B] in {0, 1}.
    step = (2^24 + q // 2) // q.  Per axis of N pixels: slack = N * (65536 - step), lo = min(0, slack), hi = max(0, slack),
    o = lo + ((r * (hi - lo + 1)) >> 31), origin = o + (step >> 1) - 32768.  Scale >= 1: every output pixel is inside -- a random crop of the
    enlarged image.  Scale < 1: the whole source lies inside the window at a random position, fill / ignore_index around it."""
    H, W = int(H), int(W)
    if not (1 <= H <= MAX_SIZE and 1 <= W <= MAX_SIZE):
        raise ValueError(f'H and W must be in [1, {MAX_SIZE}]')
    q, ry, rx, flip = (torch.as_tensor(t).to(torch.int64) for t in (q, ry, rx, flip))
    # both axes at once as [B, 2]: every operation here is a launch of its own in the step's stream.  hi - lo is |slack|.
    step = step_from_q(q)[:, None]
    slack = (STEP_ONE - step) * _sizes(H, W, q.device)
    o = slack.clamp(max=0) + ((torch.stack([ry, rx], dim=-1) * (slack.abs() + 1)) >> 31)
    origin = o + ((step >> 1) - (STEP_ONE >> 1))
    return torch.cat([step, origin, flip[:, None]], dim=1)


def _q_bounds(scale):
    try:
        smin, smax = (float(v) for v in scale)
    except (TypeError, ValueError):
        raise ValueError('scale must be a pair (smin, smax)') from None
    if not smin <= smax:
        raise ValueError('scale: smin must not exceed smax')
    if smin < 1 / 8 or smax > 8:
        raise ValueError('scale must lie within [1/8, 8] (the kernel accepts a source pitch of 2^13 ... 2^19)')
    return round(Q_ONE * smin), round(Q_ONE * smax)


class RandomScaleCrop:
    """Random scale in [smin, smax] (on a grid of 1/256), a random crop to the input's own size or random padding around the shrunk image,
    and a horizontal flip, per image, drawn from a torch.Generator on the batch's device: the sampler of the task step (Trainer with
    cfg.augment=True).  ``draw`` never synchronises with the host."""

    def __init__(self, scale=(0.5, 2.0), flip=True, fill=0.0, ignore_index=-100, seed=0):
        self.qmin, self.qmax = _q_bounds(scale)
        self.scale = tuple(float(v) for v in scale)
        self.flip, self.fill, self.ignore_index, self.seed = bool(flip), float(fill), int(ignore_index), int(seed)
        self.gen = None                       # torch.Generator, created on the device of the first draw
        self._gen_state = None                # a loaded generator state waiting for the device

    def _ensure_gen(self, device):
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if self.gen is None:
            self.gen = torch.Generator(device=device)
            self.gen.manual_seed(self.seed)
            if self._gen_state is not None:
                self.gen.set_state(self._gen_state)
                self._gen_state = None
        elif self.gen.device != device:
            raise ValueError(f'RandomScaleCrop draws on {self.gen.device}, not on {device}')
        return device

    def draw(self, B, H, W, device='cuda'):
        """-> params int64 [B, 4] on the device: q = randint(qmin, qmax + 1), two randint(2^31), one randint(2) (zeros with flip=False, no
        draw), through params_from_draws.  No host synchronisation."""
        dev = self._ensure_gen(device)
        q = torch.randint(self.qmin, self.qmax + 1, (B,), generator=self.gen, device=dev)
        ry = torch.randint(1 << 31, (B,), generator=self.gen, device=dev)
        rx = torch.randint(1 << 31, (B,), generator=self.gen, device=dev)
        if self.flip:
            flip = torch.randint(2, (B,), generator=self.gen, device=dev)
        else:
            flip = torch.zeros(B, dtype=torch.int64, device=dev)
        return params_from_draws(q, ry, rx, flip, H, W)

    def __call__(self, images, labels):
        """draw, then augment_batch: -> (images', labels') of the inputs' shapes."""
        ref = images if images is not None else labels
        if not ref.is_cuda:
            raise RuntimeError('continual-learning_amd augmentation runs only on GPU tensors: there is no CPU fallback')
        return augment_batch(images, labels, self.draw(ref.shape[0], ref.shape[-2], ref.shape[-1], ref.device), self.fill, self.ignore_index)

    def state_dict(self):
        """The configuration and the generator state (a host byte tensor, as torch hands it out; None before the first draw)."""
        return dict(scale=self.scale, flip=self.flip, fill=self.fill, ignore_index=self.ignore_index, seed=self.seed,
                    rng=self.gen.get_state() if self.gen is not None else self._gen_state)

    def load_state_dict(self, state):
        """Restores state_dict()'s result.  The generator state waits for the first draw, which creates the generator on the batch's
        device (a state taken from a generator of another device type is refused there by torch)."""
        self.qmin, self.qmax = _q_bounds(state['scale'])
        self.scale = tuple(float(v) for v in state['scale'])
        self.flip, self.fill, self.ignore_index, self.seed = bool(state['flip']), float(state['fill']), int(state['ignore_index']), int(state['seed'])
        self.gen = None
        self._gen_state = state['rng']
        return self
