"""Drop-in ``UNet(num_classes, in_dim=3, conv_dim=64)`` whose forward/backward run on libclamd's HIP kernels.

Mirrors the reference module surface (models/unet.py:40-92): same constructor, the same 82 parameters in the same
registration order, the same 136 ``state_dict`` keys ('enc1.0.weight', 'enc2.block.1.weight', 'dec1.block.6.weight',
'last.6.bias', ...), fp32 NCHW in / fp32 NCHW logits out, ``.train()/.eval()`` BatchNorm semantics per BatchNorm module (frozen
statistics: ``bn.eval()`` under ``model.train()``, backward included), autograd-attached.
The child modules (nn.Conv2d, nn.BatchNorm2d, ...) are only PARAMETER CONTAINERS with torch's default init; their own
``forward`` is never called.  ``UNet.forward`` runs the whole network as ONE ``torch.autograd.Function`` whose forward
and backward are fixed schedules of C-ABI kernel launches on NHWC activations (fp32 or bf16) kept in buffers owned by
PyTorch's allocator.  There is no CPU path: calling it with CPU tensors raises.
"""
import math
import os
import weakref

import torch
import torch.nn as nn

from . import _lib
from .ops import cpad      # noqa: F401  (part of this module's surface: the package re-exports it from here)
from .plan import Switches


def _env_tri(name):
    """A switch from the environment: False ('0', 'false'), True ('1', 'true'; any letter case), else 'auto' (unset included)."""
    return {'0': False, 'false': False, '1': True, 'true': True}.get(os.environ.get(name, 'auto').lower(), 'auto')


def _env_flag(name, default=True):
    """... for an on / off switch: anything that is not an off or on spelling leaves the default."""
    v = _env_tri(name)
    return default if v == 'auto' else v


# Fused BN-backward sums in the epilogue of the data-gradient kernel that produces the BN-output gradient:
# 'auto' = where that kernel is the persistent bf16 kernel (sums stay in registers across tiles, one flush per workgroup,
# the saved activation is prefetched under the last K-step); True = everywhere the kernels support it (every dgrad
# launch of the other kernels got 30-80 us slower than the 33-us reduce pass it replaced); False = never.
FUSE_BN_SUMS = _env_tri('CLAMD_FUSE_BN_SUMS')

# fp32 path: forward and data gradient of the 3x3 convolutions by Winograd F(2x2,3x3) (csrc/wino.hip): 2.25x fewer MFMA
# cycles, fp32 transforms (error vs fp64 3.5e-7 against 2.3e-7 for the direct sum).  False = direct implicit GEMM.
WINOGRAD = True
# ... and, where the image width is a multiple of 4, by the hybrid F(2x4,3x3) (csrc/wino24.hip): 3 instead of 4 multiply-adds
# per output (1.17x faster launches, error vs fp64 1e-6).  False = F(2x2,3x3) everywhere.
WINOGRAD24 = True
# ... and the weight gradient too (csrc/wino24_wgrad.hip) where it measures faster: 'auto' = images of at least 64x64
# (tools/wino24_wgrad_ab.py: 1.02-1.04x there, 0.88-1.00x on the deep layers -- both operands are transformed in the loop,
# 3.5 transform VALU per MFMA, so the 25 % fewer MFMAs buy little); True = everywhere it applies; False = F(2x2,3x3).
WINOGRAD24_WGRAD = 'auto'
# ... and, for the wide layers, with the operands transformed ONCE per tensor (csrc/wino24g.hip): the in-kernel transform is
# redone by every output-slab workgroup (8-16x per tile at 512/1024 channels) and costs 2-3.5 VALU per fp32 MFMA; the
# transform-free K loop runs at 0.77-0.90 of the MFMA pipe instead of 0.57-0.66 (tools/wino24g_ab.py).  The transformed
# input (3x the activation) is kept from the forward pass and is also the x-side operand of the weight-gradient GEMM.
# 'auto' = where the transform pass pays for itself (see plan.py); False = never.
PRETRANSFORM = _env_tri('CLAMD_PRETRANSFORM')
# ... and those pre-transformed layers by the 2-D F(4x4,3x3) (csrc/wino44g.hip: 2.25 instead of 3 multiply-adds per output, a transformed
# input of 2.25x instead of 3x the activation; error vs fp64 2-3.5e-6) where a launch has a chip's worth of its 512-pixel x 64-channel work
# items: the 32x32 and 64x64 levels at config 2 (tools/wino44g_ab.py: transform + forward 1.23-1.30x, weight gradient 1.0-1.26x faster
# there; 0.67-0.70x at 16x16, where 128 work items leave half the chip idle).  'auto' = that rule; True = wherever it applies; False = never.
WINOGRAD44 = _env_tri('CLAMD_WINOGRAD44')
# ... and the BatchNorm in front of such a convolution is applied by the transform kernel on load where nothing else reads the
# BatchNorm output (the first unit of enc3/enc4/dec1/dec2/dec3): one HBM pass less per unit.  False = always run clamd_bn_apply.
FOLD_BN_INTO_TRANSFORM = _env_flag('CLAMD_FOLD_BN')
NARROW_DIRECT = _env_flag('CLAMD_NARROW_DIRECT')
WGRAD_TAIL_EARLY = _env_flag('CLAMD_WGRAD_TAIL_EARLY')      # see engine._Engine._conv_bwd
NARROW_PRE_WGRAD = _env_flag('CLAMD_NARROW_PRE_WGRAD')      # the 128-channel layers pre-transformed (forward + weight gradient), see engine.py
# The narrow layers (in-kernel transform / bf16 direct kernels) cannot take the affine on load -- their loops are VALU-bound -- so there
# the BatchNorm between the two convolutions of a block (models/unet.py:13-18) is folded ALGEBRAICALLY into the second one
# (csrc/bnfold.hip): filters packed with scale[ci] once the statistics are final, the shift as a border-class bias table in the
# epilogue, the weight gradient fixed up from the gradient's border sums.  The normalised tensor is never written: the bn_apply pass
# of the first unit of enc1 / enc2 / dec4 / last (268 + 268 MB at level 0 in fp32) leaves the forward pass.  Up to
# FOLD_FILTERS_MAX_CHANNELS input channels: the per-step filter pack is on the critical path, the apply pass shrinks with depth.
# Interleaved A/B (bench.py, ms per step): fp32 21.30 -> 21.08, bf16x3 15.17 -> 14.84; bf16 6.81 = 6.81 in round 3 (the apply passes are half
# the bytes while the pack launch and the border tiles' table lookups cost the same) and 6.489 -> 6.415 in round 4, with the
# channels-in-the-lane epilogue (igemm_pws.hip: the class-4 bias is the accumulator's start, only the lanes of border pixels of border
# tiles add a difference row) and the pack launch at 7 us: every compute dtype folds now.  False = never.
FOLD_BN_INTO_FILTERS = _env_flag('CLAMD_FOLD_FILTERS')
FOLD_FILTERS_MAX_CHANNELS = int(os.environ.get('CLAMD_FOLD_FILTERS_MAX_CHANNELS', '128'))
# fp32 path: the same fold for the OUTPUT of an encoder block -- pooled into the next block, concatenated into the decoder (models/unet.py:80-87)
# -- where both readers are narrow F(2x4) convolutions (enc1 -> enc2's first conv and last's first conv at config 2): the block's second conv
# writes its conv+ReLU output straight into the concat slice, one pass pools it (window minimum where the BatchNorm scale is negative:
# max(s x + t) = s min(x) + t), and the two readers take scale / shift in their filters and bias tables.  The pooled bn_apply pass of enc1
# (603 MB, the largest elementwise pass of the step) becomes a 335 MB pooling pass.
FOLD_POOLED = _env_flag('CLAMD_FOLD_POOLED')
# fp32 path, pre-transformed weight gradients: the gradient-side transform (HBM-bound) on a THIRD stream, so that it runs beside the
# weight-gradient GEMM of the unit before (which leaves 188 registers per SIMD free) instead of in front of its own GEMM on the second
# stream, and that GEMM can start the moment the data gradient of its unit has finished.
WGRAD_XFORM_STREAM = _env_flag('CLAMD_WGRAD_XFORM_STREAM')
# Weight-gradient kernels (and the bias-gradient channel sums of the ConvTranspose / head layers) go to a second HIP stream:
# they are off the critical chain of the backward pass (dgrad -> BatchNorm-backward reduce / finalize / apply -> dgrad ...),
# and the HBM-bound BatchNorm passes of the NEXT unit fit beside a weight-gradient workgroup on the same CU (one wave per
# SIMD, <= 64 registers, <= 8 KB LDS), so they run under the MFMA-bound kernel instead of after it.  Results are unchanged
# (same kernels, same arguments); joined back before backward() returns.  Off while bench.py times single launches.
WGRAD_STREAM = _env_flag('CLAMD_WGRAD_STREAM')      # =0: everything on one stream (kernel-trace profiles)
# The plain filter pack of everything behind enc3 (96 % of the parameters; HBM-bound) on the second stream under enc1-enc3 instead of in
# front of the forward pass (=0: one launch chain on the main stream, as before round 4)
PACK_LATE_STREAM = _env_flag('CLAMD_PACK_LATE_STREAM')
PACK_LATE_AT = int(os.environ.get('CLAMD_PACK_LATE_AT', '2'))      # index of the convolution unit it is released beside (2 = enc2's first)

# bench.py sets this to a list to get per-launch HIP-event timings of the MFMA kernels:
# entries (tag, algorithmic_flops, start_event, end_event, algorithmic_bytes), recorded on the stream the kernel is
# launched on.  Algorithmic bytes of a 3x3 convolution launch = both activations once + the filters once.
KERNEL_TIMING = None


def switches():
    """The planning switches above (plan.Switches), read now: tests and tools/step_ab.py set them as module attributes."""
    return Switches(*(globals()[k] for k in Switches._fields))


def stage_table(num_classes, in_dim=3, conv_dim=64):
    """Structure of models/unet.py:49-72: (name, wrapped_in_block, pool_first, conv/bn module indices, tail)."""
    d = conv_dim
    t = [dict(name='enc1', wrapped=False, pool=False, convs=[(0, 2, in_dim, d), (3, 5, d, d)], tail=None)]
    c = d
    for i in (2, 3, 4):
        t.append(dict(name=f'enc{i}', wrapped=True, pool=True, convs=[(1, 3, c, 2 * c), (4, 6, 2 * c, 2 * c)], tail=None))
        c *= 2
    for i, (cin, mid, cout) in enumerate([(8 * d, 16 * d, 8 * d), (16 * d, 8 * d, 4 * d), (8 * d, 4 * d, 2 * d),
                                          (4 * d, 2 * d, d)], 1):
        t.append(dict(name=f'dec{i}', wrapped=True, pool=False, convs=[(0, 2, cin, mid), (3, 5, mid, mid)],
                      tail=('convT', 6, mid, cout)))
    t.append(dict(name='last', wrapped=False, pool=False, convs=[(0, 2, 2 * d, d), (3, 5, d, d)],
                  tail=('head', 6, d, num_classes)))
    return t


class _NoForward:
    """The LAYERS inside UNet's blocks are parameter containers (torch's default init, the reference's state_dict names).  Their own
    ``forward`` would run stock torch operators (MIOpen) -- a silent fallback this package does not have: it raises.  The BLOCKS
    (models/unet.py:8-38: enc1 ... last, and their ``.block`` sequences) can be called on their own: blocks.py runs them as one
    autograd Function over libclamd kernels."""

    def forward(self, *args, **kwargs):
        raise RuntimeError(f'{type(self).__name__}.forward: the layers of continual-learning_amd.UNet only hold parameters; '
                           'run UNet.forward / UNet.predict, or a whole block (model.enc2(x), model.dec1(x): blocks.py) -- there is no '
                           'stock-torch path for a single layer')


class _Seq(_NoForward, nn.Sequential):
    def forward(self, x):
        spec = getattr(self, '_block_spec', None)
        if spec is None:
            return _NoForward.forward(self, x)
        from . import blocks
        return blocks.run_block(self, spec[0], spec[1], x)


class _Conv2d(_NoForward, nn.Conv2d):
    pass


class _ConvTranspose2d(_NoForward, nn.ConvTranspose2d):
    pass


class _BatchNorm2d(_NoForward, nn.BatchNorm2d):
    pass


class _ReLU(_NoForward, nn.ReLU):
    pass


class _MaxPool2d(_NoForward, nn.MaxPool2d):
    pass


class _Stage(_NoForward, nn.Module):
    """Gives the 'encN.block.K' / 'decN.block.K' key names of models/unet.py:8-38."""

    def __init__(self, layers):
        super().__init__()
        self.block = _Seq(*layers)

    def forward(self, x):
        return self.block(x)


def _stage_modules(st):
    layers = [_MaxPool2d(2, 2)] if st['pool'] else []
    for _, _, cin, cout in st['convs']:
        layers += [_Conv2d(cin, cout, 3, 1, 1), _ReLU(), _BatchNorm2d(cout)]
    if st['tail'] is not None:
        kind, _, cin, cout = st['tail']
        layers.append(_ConvTranspose2d(cin, cout, 2, 2) if kind == 'convT' else _Conv2d(cin, cout, 1, 1))
    return layers


_DTYPES = {'fp32': (_lib.F32, torch.float32), 'float32': (_lib.F32, torch.float32),
           'bf16': (_lib.BF16, torch.bfloat16), 'bfloat16': (_lib.BF16, torch.bfloat16),
           'bf16x3': (_lib.SPLIT, torch.float32)}


class UNet(nn.Module):
    """models/unet.py:40-92.  ``compute_dtype``: 'fp32' (exact-fp32 MFMA, the reference's arithmetic), 'bf16'
    (bf16 activations/packed weights, fp32 accumulation, fp32 master weights and BatchNorm statistics) or 'bf16x3'
    (fp32 activations; every MFMA operand split into bf16 hi+lo, three bf16 MFMAs per product, fp32 accumulation)."""

    def __init__(self, num_classes, in_dim=3, conv_dim=64, compute_dtype='fp32'):
        super().__init__()
        self.num_classes, self.in_dim, self.conv_dim = num_classes, in_dim, conv_dim
        if compute_dtype not in _DTYPES:
            raise ValueError(f'compute_dtype must be one of {sorted(_DTYPES)}')
        self.compute_dtype = compute_dtype
        self._table = stage_table(num_classes, in_dim, conv_dim)
        for st in self._table:
            layers = _stage_modules(st)
            mod = _Stage(layers) if st['wrapped'] else _Seq(*layers)
            (mod.block if st['wrapped'] else mod)._block_spec = (st, _DTYPES[compute_dtype][0])      # stand-alone call of the block: blocks.py
            self.add_module(st['name'], mod)
        self._engines = {}
        self.grad_sync = None          # set by ddp.GradSync to overlap RCCL all-reduce with backward
        self._tuning = None

    @property
    def tuning(self):
        """Kernel-structure selection of THIS model (a `clamd_tuning`, see include/clamd.h), passed to every launch: the
        library has no process-wide knobs.  Fields may be changed between steps (A/B tools, ddp.GradSync)."""
        if self._tuning is None:
            self._tuning = _lib.Tuning()
        return self._tuning

    def _seq(self, st):
        m = getattr(self, st['name'])
        return m.block if st['wrapped'] else m

    def _replicate_for_data_parallel(self):
        """``nn.DataParallel(model)`` (trainer.py:120-122) on ONE device calls the module directly and works as is.  On several
        devices it would replicate this module into threads of one process every forward; the engine (activation buffers,
        streams, flat gradient buffer) belongs to one device, and the reference's scheme is what ddp.GradSync replaces:
        one process per GPU, RCCL all-reduce overlapped with backward."""
        raise RuntimeError('continual-learning_amd.UNet cannot be replicated by nn.DataParallel across devices: run one process per '
                           'GPU (torch.distributed.run) with continual-learning_amd.ddp.init_rccl + ddp.GradSync(model, optimizer)')

    def _engine(self, x):
        """The engine (kernel plan and buffers) of x's shape; built on first use, one shape at a time: activations are sized for it."""
        if not x.is_cuda:
            raise RuntimeError('continual-learning_amd.UNet runs only on an MI355X GPU tensor: there is no CPU fallback')
        if x.dim() != 4 or x.shape[1] != self.in_dim:
            raise ValueError(f'expected input [B,{self.in_dim},H,W], got {tuple(x.shape)}')
        B, _, H, W = x.shape
        assert H % 16 == 0 and W % 16 == 0, 'input size(H, W) must be a multiple of 16 (four 2x2 pools and matching skip concats)'
        key = (B, H, W, x.device.index)
        if key not in self._engines:
            self._engines = {key: _Engine(self, B, H, W, x.device)}
        return self._engines[key]

    def forward(self, x):
        eng = self._engine(x)
        out = _UNetFn.apply(x.contiguous().float(), eng, *self.parameters())
        out._clamd_engine = (weakref.ref(eng), eng.generation)      # lets this package's loss write d logits where the backward pass reads it
        return out

    @torch.no_grad()
    def predict(self, x):
        """``torch.max(self(x), 1)[1]`` (trainer.py:279) without materialising the logits: the arg-max over classes runs
        in the epilogue of the head kernel.  int64 [B,H,W]; every BatchNorm follows its own ``.training``."""
        return self._engine(x).forward(x.contiguous().float(), list(self.parameters()), predict=True)

    MAX_CLASSES = 32      # the head's padded width cpad(K) and the loss kernels' register arrays

    @torch.no_grad()
    def expand_classes(self, n, init='background'):
        """Class-incremental growth of the head (build-defined, parity unpinned): ``last.6`` goes from K to K + n output rows, old rows keep
        their values.  init='background': every new row's weight is a copy of the background row's (row 0) and, with b0 the old background
        bias, the background bias and every new bias become b0 - log(n + 1) -- the softmax of the grown head then gives every old class
        k >= 1 its old probability and splits the old background probability evenly over background and the new classes.  init='default':
        nn.Conv2d's own initialisation for the new rows (global torch RNG).  Parameter order and state_dict keys do not change; the engine
        is dropped (the next forward plans and allocates for the new width).  Returns (old_weight, old_bias, new_weight, new_bias), the
        mapping FusedAdam.replace_params / Consolidation.grow take."""
        n, K = int(n), self.num_classes
        if n <= 0:
            raise ValueError(f'expand_classes: n must be positive, got {n}')
        if K + n > self.MAX_CLASSES:
            raise ValueError(f'expand_classes: {K} + {n} classes exceed the {self.MAX_CLASSES} the head and the loss kernels hold')
        if init not in ('background', 'default'):
            raise ValueError("expand_classes: init must be 'background' or 'default'")
        st = self._table[-1]
        kind, ti, cin, _ = st['tail']
        seq = self._seq(st)
        old = seq[ti]
        new = _Conv2d(cin, K + n, 1, 1).to(device=old.weight.device, dtype=old.weight.dtype)      # torch's init: the 'default' rows
        new.weight[:K].copy_(old.weight)
        new.bias[:K].copy_(old.bias)
        if init == 'background':
            new.weight[K:].copy_(old.weight[:1].expand(n, -1, -1, -1))
            b0 = old.bias[0] - math.log(n + 1)
            new.bias[0] = b0
            new.bias[K:] = b0
        new.train(old.training)
        seq[ti] = new
        st['tail'] = (kind, ti, cin, K + n)      # the same dict is the stand-alone block's spec (blocks.py)
        self.num_classes = K + n
        self._engines = {}
        return old.weight, old.bias, new.weight, new.bias

    def extra_repr(self):
        return f'num_classes={self.num_classes}, in_dim={self.in_dim}, conv_dim={self.conv_dim}, compute={self.compute_dtype}'


def dlogits_sink(logits, B, K, H, W):
    """For loss.CrossEntropyLoss: the engine whose forward produced `logits` (and nothing since), or None.  Its `dl` buffer [B,H,W,Kp] takes a
    second copy of d logits in the head data gradient's own layout; the engine uses it when the gradient autograd hands back is the very
    tensor the loss wrote (same storage, untouched: `dl_src`) and converts that tensor as before otherwise."""
    tag = getattr(logits, '_clamd_engine', None)
    if tag is None:
        return None
    eng, gen = tag[0](), tag[1]
    if eng is None or eng.generation != gen or (eng.B, eng.K, eng.H, eng.W) != (B, K, H, W) or not all(eng.fwd_modes) or eng.dl.device != logits.device:
        return None
    return eng


class _UNetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eng, *params):
        logits = eng.forward(x, params)
        ctx.eng = eng
        ctx.gen = eng.generation
        ctx.nparams = len(params)
        return logits

    @staticmethod
    def backward(ctx, gout):
        eng = ctx.eng
        if ctx.gen != eng.generation:
            raise RuntimeError('UNet.backward: the saved activations were overwritten by a later forward of the same module')
        grads = eng.backward(gout.contiguous().float())
        return (None, None) + tuple(grads)


from .engine import _Engine, _FoldSource, _hbm      # noqa: E402,F401  (last: engine.py reads the switches above from this module when they are used)
