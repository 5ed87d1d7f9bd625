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

from . import _lib, syncbn
from ._lib import call, ptr, tune_ptr
from .ops import PackTable, WinoPackTable, cpad
from .plan import ALGOS, Switches, plan_net

BN_EPS, BN_MOMENTUM = 1e-5, 0.1

# Fused BN-backward sums in the epilogue of the data-gradient kernel that produces the BN-output gradient:
# 'auto' = where that kernel is the persistent bf16 kernel (sums stay in registers across tiles, one flush per workgroup,
# the saved activation is prefetched under the last K-step); True = everywhere the kernels support it (every dgrad
# launch of the other kernels got 30-80 us slower than the 33-us reduce pass it replaced); False = never.
FUSE_BN_SUMS = {'0': False, 'false': False, '1': True, 'true': True}.get(os.environ.get('CLAMD_FUSE_BN_SUMS', 'auto').lower(), 'auto')

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
PRETRANSFORM = os.environ.get('CLAMD_PRETRANSFORM', 'auto')
PRETRANSFORM = {'0': False, 'false': False, '1': True, 'true': True}.get(str(PRETRANSFORM).lower(), 'auto')
# ... and those pre-transformed layers by the 2-D F(4x4,3x3) (csrc/wino44g.hip: 2.25 instead of 3 multiply-adds per output, a transformed
# input of 2.25x instead of 3x the activation; error vs fp64 2-3.5e-6) where a launch has a chip's worth of its 512-pixel x 64-channel work
# items: the 32x32 and 64x64 levels at config 2 (tools/wino44g_ab.py: transform + forward 1.23-1.30x, weight gradient 1.0-1.26x faster
# there; 0.67-0.70x at 16x16, where 128 work items leave half the chip idle).  'auto' = that rule; True = wherever it applies; False = never.
WINOGRAD44 = os.environ.get('CLAMD_WINOGRAD44', 'auto')
WINOGRAD44 = {'0': False, 'false': False, '1': True, 'true': True}.get(str(WINOGRAD44).lower(), 'auto')
# ... and the BatchNorm in front of such a convolution is applied by the transform kernel on load where nothing else reads the
# BatchNorm output (the first unit of enc3/enc4/dec1/dec2/dec3): one HBM pass less per unit.  False = always run clamd_bn_apply.
FOLD_BN_INTO_TRANSFORM = os.environ.get('CLAMD_FOLD_BN', '1') != '0'
NARROW_DIRECT = os.environ.get('CLAMD_NARROW_DIRECT', '1') != '0'
WGRAD_TAIL_EARLY = os.environ.get('CLAMD_WGRAD_TAIL_EARLY', '1') != '0'      # see _Engine._conv_bwd
NARROW_PRE_WGRAD = os.environ.get('CLAMD_NARROW_PRE_WGRAD', '1') != '0'      # the 128-channel layers pre-transformed (forward + weight gradient), see _Engine
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
FOLD_BN_INTO_FILTERS = os.environ.get('CLAMD_FOLD_FILTERS', '1').lower() not in ('0', 'false')
FOLD_FILTERS_MAX_CHANNELS = int(os.environ.get('CLAMD_FOLD_FILTERS_MAX_CHANNELS', '128'))
# fp32 path: the same fold for the OUTPUT of an encoder block -- pooled into the next block, concatenated into the decoder (models/unet.py:80-87)
# -- where both readers are narrow F(2x4) convolutions (enc1 -> enc2's first conv and last's first conv at config 2): the block's second conv
# writes its conv+ReLU output straight into the concat slice, one pass pools it (window minimum where the BatchNorm scale is negative:
# max(s x + t) = s min(x) + t), and the two readers take scale / shift in their filters and bias tables.  The pooled bn_apply pass of enc1
# (603 MB, the largest elementwise pass of the step) becomes a 335 MB pooling pass.
FOLD_POOLED = os.environ.get('CLAMD_FOLD_POOLED', '1') != '0'
# fp32 path, pre-transformed weight gradients: the gradient-side transform (HBM-bound) on a THIRD stream, so that it runs beside the
# weight-gradient GEMM of the unit before (which leaves 188 registers per SIMD free) instead of in front of its own GEMM on the second
# stream, and that GEMM can start the moment the data gradient of its unit has finished.
WGRAD_XFORM_STREAM = os.environ.get('CLAMD_WGRAD_XFORM_STREAM', '1') != '0'
# Weight-gradient kernels (and the bias-gradient channel sums of the ConvTranspose / head layers) go to a second HIP stream:
# they are off the critical chain of the backward pass (dgrad -> BatchNorm-backward reduce / finalize / apply -> dgrad ...),
# and the HBM-bound BatchNorm passes of the NEXT unit fit beside a weight-gradient workgroup on the same CU (one wave per
# SIMD, <= 64 registers, <= 8 KB LDS), so they run under the MFMA-bound kernel instead of after it.  Results are unchanged
# (same kernels, same arguments); joined back before backward() returns.  Off while bench.py times single launches.
WGRAD_STREAM = os.environ.get('CLAMD_WGRAD_STREAM', '1') != '0'      # =0: everything on one stream (kernel-trace profiles)
# The plain filter pack of everything behind enc3 (96 % of the parameters; HBM-bound) on the second stream under enc1-enc3 instead of in
# front of the forward pass (=0: one launch chain on the main stream, as before round 4)
PACK_LATE_STREAM = os.environ.get('CLAMD_PACK_LATE_STREAM', '1') != '0'
PACK_LATE_AT = int(os.environ.get('CLAMD_PACK_LATE_AT', '2'))      # index of the convolution unit it is released beside (2 = enc2's first)

# bench.py sets this to a list to get per-launch HIP-event timings of the MFMA kernels:
# entries (tag, algorithmic_flops, start_event, end_event, algorithmic_bytes), recorded on the stream the kernel is
# launched on.  Algorithmic bytes of a 3x3 convolution launch = both activations once + the filters once.
KERNEL_TIMING = None


def switches():
    """The planning switches above (plan.Switches), read now: tests and tools/step_ab.py set them as module attributes."""
    return Switches(*(globals()[k] for k in Switches._fields))


_TIMED_UNIT = ['', 1.0]   # conv unit being launched and the fraction of its algorithmic FLOPs the kernel executes (Winograd:
#                         # 16/36 or 24/72); only read while KERNEL_TIMING is set (bench.py, tools/layer_table.py)


_SIDE_STREAMS = {}


def _side_stream(dev, n):
    """Side stream n (2: parameter gradients, 3: their input transforms): ONE per device and process, shared by every engine: HIP
    multiplexes streams onto a handful of hardware queues (4 by default) in creation order, and a kernel queues behind whatever shares
    its hardware queue -- a stream per engine would sooner or later land on the queue RCCL's kernels use."""
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), n)
    if key not in _SIDE_STREAMS:
        # default priority: the device offers only (normal, high), and giving either stream the high one changed nothing
        # measurable (tools/cu_steal.py, base and held-CU cases within 0.5 %)
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=dev)
    return _SIDE_STREAMS[key]


def _timed(tag, flops, nbytes, name, *args):
    kt = KERNEL_TIMING
    if kt is None:
        call(name, *args)
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call(name, *args)
    e1.record()
    kt.append((tag, flops, e0, e1, nbytes, _TIMED_UNIT[0], _TIMED_UNIT[1]))


def _hbm(family, nbytes, name, *args):
    """A launch of an HBM-bound kernel family (A5 / A6 BatchNorm and pooling passes, A7 ConvTranspose, A9 head, A10 loss,
    A13 Adam, enc1.0) with its ALGORITHMIC bytes -- every tensor it has to read or write, once: timed per launch by bench.py's instrumented
    steps (`hbm_kernels` on the JSON line), a plain launch otherwise."""
    _timed('hbm:' + family, 0.0, nbytes, name, *args)


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


class _FoldSource:
    """What a folded convolution reads instead of a normalised tensor: the raw tensor (`y`, pitch `cout_p`) and the per-input-channel
    scale / shift (`vec[0]`, `vec[1]`) that live in its filters and bias table -- the interface of the producing _Conv the pair fold uses."""

    def __init__(self, y, pitch, scale, shift):
        self.y, self.cout_p, self.vec, self.apply_in_filters = y, pitch, [scale, shift], False


def _sums_into(c):
    """(y, sums, rows) arguments of a data-gradient launch that accumulates the BatchNorm-backward sums of unit c (plan.Unit.sums_by), or none."""
    return (ptr(c.y), ptr(c.sums), c.sum_rows) if c is not None else (None, None, 0)


class _Conv:
    """One Conv3x3 -> ReLU -> BatchNorm unit and everything it needs in both directions."""
    # read-only views of the plan that bench.py reads (nothing in this package uses them)
    wino = property(lambda u: u.f.wino)
    w24 = property(lambda u: u.plan.fwd in ('f24', 'f24_direct', 'f24_pre', 'f44_pre'))
    f44 = property(lambda u: u.plan.fwd == 'f44_pre')
    pre_f = property(lambda u: u.f.pre)
    pre_d = property(lambda u: u.d is not None and u.d.pre)


class _Engine:
    @property
    def model(self):
        return self._model_ref()

    def __init__(self, model, B, H, W, device):
        lib = _lib.load()
        self._model_ref = weakref.ref(model)      # the model owns its engines; a strong reference back would leave the
        #                                           multi-GB activation buffers to the cyclic garbage collector
        self.B, self.H, self.W, self.dev = B, H, W, device
        self.dcode, self.tdtype = _DTYPES[model.compute_dtype]
        self.pack_late_stream, self.pack_late_at = bool(PACK_LATE_STREAM), int(PACK_LATE_AT)
        self.tuning = model.tuning
        self.NS = lib.clamd_bn_bwd_nsums()
        self.generation = 0
        self.dl_src = None
        self.fwd_modes = ()          # per conv unit: its BatchNorm's .training at the last forward (False = running statistics)
        self.bn_group = None         # process group of the synchronised BatchNorm layers at the last forward (syncbn.py), or None
        self._has_sync = None        # any nn.SyncBatchNorm among the units' modules (None: not looked at yet)
        self._sync_arena = None
        self.esize = 2 if self.dcode == _lib.BF16 else 4      # activation element size in HBM (bf16x3 stores fp32)
        K, d = model.num_classes, model.conv_dim
        self.K, self.Kp = K, cpad(K)
        T = self.tdtype
        dev = device

        def act(level, c):
            return torch.zeros(B, H >> level, W >> level, c, dtype=T, device=dev)

        named = dict(model.named_parameters())
        bufs = dict(model.named_buffers())
        mods = dict(model.named_modules())
        self.param_names = [n for n, _ in model.named_parameters()]
        # flat gradient buffer in REVERSE registration order (= order gradients are produced): contiguous buckets
        sizes = [named[n].numel() for n in self.param_names]
        self.gflat = torch.zeros(sum(sizes), dtype=torch.float32, device=dev)
        # NOTE: no tensor views of the gradients are kept alive here.  Fresh views are handed to autograd at the end
        # of every backward so that AccumulateGrad can adopt them as .grad without a copy (it clones when the
        # incoming gradient has other owners).
        self.goffset, self.gshape, off = {}, {}, 0
        for n in reversed(self.param_names):
            k = named[n].numel()
            self.goffset[n] = (off, k)
            self.gshape[n] = tuple(named[n].shape)
            off += k

        # ---- geometry: stages -> conv units ----------------------------------------------------------
        self.x_in = act(0, cpad(model.in_dim))
        self.stages = []
        C = [d, 2 * d, 4 * d, 8 * d]                      # encoder output channels, levels 0..3
        self.cat = [act(l, 2 * cpad(C[l])) for l in range(4)]
        self.gcat = [act(l, 2 * cpad(C[l])) for l in range(4)]
        self.pool = [act(l + 1, cpad(C[l])) for l in range(4)]
        self.gpool = [act(l + 1, cpad(C[l])) for l in range(4)]

        def unit(prefix, ci, bi, p, xin):
            u = _Conv()
            u.plan, u.name = p, p.name
            u.f, u.d, u.g = ALGOS[p.fwd], p.dgrad and ALGOS[p.dgrad], ALGOS[p.wgrad]      # kernel families of the three directions
            u.w, u.b = named[f'{prefix}.{ci}.weight'], named[f'{prefix}.{ci}.bias']
            u.gamma, u.beta = named[f'{prefix}.{bi}.weight'], named[f'{prefix}.{bi}.bias']
            u.rm, u.rv = bufs[f'{prefix}.{bi}.running_mean'], bufs[f'{prefix}.{bi}.running_var']
            u.nbt = bufs[f'{prefix}.{bi}.num_batches_tracked']
            u.bn, u.bn_train = mods[f'{prefix}.{bi}'], True         # its .training is the unit's BatchNorm mode (read every forward)
            u.bn_parent, u.bn_parent_name, u.bn_key, u.bn_sync = mods[prefix], prefix, str(bi), False      # where the module lives (convert_sync_batchnorm swaps it)
            u.keys = (f'{prefix}.{ci}.weight', f'{prefix}.{ci}.bias', f'{prefix}.{bi}.weight', f'{prefix}.{bi}.bias')
            u.level, u.h, u.w_, u.cin_p, u.cout, u.cout_p = p.level, p.h, p.w, p.cin_p, p.cout, p.cout_p
            u.cin_segs, u.cin = list(p.cin_segs), sum(s[0] for s in p.cin_segs)      # [(logical, physical), ...] one or two segments
            u.xin, u.xin_ldc = xin, xin.shape[-1]
            u.y, u.gz = act(p.level, u.cout_p), act(p.level, u.cout_p)
            u.vx = torch.empty(getattr(lib, u.f.x_elems)(B, u.h, u.w_, u.cin_p), dtype=torch.float32, device=dev) if u.f.pre else None
            u.wf = torch.zeros(u.f.taps * u.cout_p * u.cin_p, dtype=T, device=dev)      # Winograd: [Cin_p/8][16|24|36][Cout_p][8] transformed
            u.wd = None if u.d is None else torch.zeros(u.d.taps * u.cin_p * u.cout_p, dtype=T, device=dev)
            u.bias_p = torch.zeros(u.cout_p, dtype=torch.float32, device=dev)
            u.vec = torch.zeros(7, u.cout_p, dtype=torch.float32, device=dev)   # scale, shift, mean, istd, k0, k1, k2
            u.m_fastest, u.y_ldc = (1 if 9 * u.cout_p > B * u.h * u.w_ else 0), u.cout_p
            u.consumer = u.sum_src = u.fold_src = u.fold_a = None             # BatchNorm placement: wired from the plan below
            u.fused_reduce = p.sums_by is not None
            u.apply_folded = u.apply_in_filters = u.fold_on = u.pool_fold = False
            return u

        ncu = torch.cuda.get_device_properties(dev).multi_processor_count if dev.type == 'cuda' else 256
        self.plan = plan_net(model._table, B, H, W, self.dcode, switches(), ncu)
        plans = iter(self.plan)
        tails = {}
        xin, g_in = self.x_in, None                                # the first convolution's input (and, at enc1, no input gradient)
        for i, st in enumerate(model._table):
            pre = st['name'] + ('.block' if st['wrapped'] else '')
            (c0, b0, _, mid), (c1, b1, _, _) = st['convs']
            pa, pb = next(plans), next(plans)
            k = pa.level
            if i > 4:                                              # behind dec1: the concat [skip | up-convolution] of this level
                xin, g_in = self.cat[k], self.gcat[k]
            ua = act(k, cpad(mid))
            a, b = unit(pre, c0, b0, pa, xin), unit(pre, c1, b1, pb, ua)
            a.out, a.pooled, a.g_in = ua, None, g_in              # g_in: dgrad target of conv a
            b.g_in = act(k, cpad(mid))                            # grad w.r.t. ua
            a.g_src = (b.g_in, b.g_in.shape[-1], None)            # where conv a's BN-output gradient comes from
            if st['tail'] is None:     # encoder: the block output goes to the skip half of the concat buffer and, pooled, to the next stage
                b.out, b.pooled = self.cat[k], self.pool[k]
                b.g_src = (self.gcat[k], self.gcat[k].shape[-1], self.gpool[k])
                a.out_ldc, b.out_ldc = a.out.shape[-1], b.out.shape[-1]
                xin, g_in = self.pool[k], self.gpool[k]
                self.stages.append(dict(kind='enc', convs=(a, b)))
                continue
            b.out, b.pooled, g_ub = act(k, cpad(mid)), None, act(k, cpad(mid))
            b.g_src = (g_ub, g_ub.shape[-1], None)
            a.out_ldc, b.out_ldc = a.out.shape[-1], b.out.shape[-1]
            kind, ti, tcin, tcout = st['tail']
            tail = tails[f'{pre}.{ti}'] = _Conv()
            tail.w, tail.b = named[f'{pre}.{ti}.weight'], named[f'{pre}.{ti}.bias']
            tail.keys = (f'{pre}.{ti}.weight', f'{pre}.{ti}.bias')
            tail.cin, tail.cin_p, tail.cout, tail.cout_p = tcin, cpad(tcin), tcout, cpad(tcout)
            tail.kind, tail.x, tail.g_x, tail.level = kind, b.out, g_ub, k
            tail.consumer, tail.fold_b = None, None
            taps = 4 if kind == 'convT' else 1                     # ConvTranspose2d 2x2 / the 1x1 head
            tail.wf = torch.zeros(taps * tail.cout_p * tail.cin_p, dtype=T, device=dev)
            tail.wd = torch.zeros(tail.cin_p * taps * tail.cout_p, dtype=T, device=dev)
            if kind == 'convT':
                up = self.cat[k - 1]
                tail.y_slice = up[..., tail.cout_p:]               # second half of the concat buffer one level up
                tail.gy_slice = self.gcat[k - 1][..., tail.cout_p:]
                tail.y_ldc = up.shape[-1]
            else:
                self.dl = act(0, self.Kp)
            tail.bias_p = torch.zeros(tail.cout_p, dtype=torch.float32, device=dev)
            self.stages.append(dict(kind='dec', convs=(a, b), tail=tail))
        self.convs = convs = [u for st in self.stages for u in st['convs']]
        self.tails = list(tails.values())                          # ConvTranspose2d x 4, the 1x1 head
        # ---- BatchNorm placement (plan.Unit): one direction only -- a cycle between units would keep the engine's buffers alive until the
        # garbage collector runs
        by = {u.name: u for u in convs}
        for u in convs:
            p = u.plan
            if p.sums_by is not None:      # that launch's epilogue accumulates u's five BatchNorm-backward sums
                u.sum_src = by.get(p.sums_by) or tails[p.sums_by]
                u.sum_src.consumer = u
            if p.fold_src is not None:     # u's input transform applies the BatchNorm in front: its bn_apply pass (and output) disappear
                u.fold_src = by[p.fold_src]
                u.fold_src.apply_folded = True
            if p.fold_a is not None:       # the BatchNorm in front lives in u's filters and border-class bias table (bnfold.hip)
                u.fold_a = by[p.fold_a]
            if p.pool_fold is not None:    # an encoder block's output: conv+ReLU straight into the skip half of the concat buffer
                k, (nxt, dec) = u.level, (by[n] for n in p.pool_fold)
                u.pool_fold, u.apply_in_filters, u.y, u.y_ldc = True, True, self.cat[k], self.cat[k].shape[-1]
                comp = torch.zeros(2, dec.cin_p, dtype=torch.float32, device=dev)  # scale / shift over the decoder conv's input: [block | up-conv]
                comp[0, u.cout_p:] = 1.0
                u.vec = [comp[0, :u.cout_p], comp[1, :u.cout_p]] + list(u.vec[2:])     # rows 4-6 (k0, k1, k2) stay contiguous
                nxt.fold_a = _FoldSource(self.pool[k], self.pool[k].shape[-1], u.vec[0], u.vec[1])
                dec.fold_a = _FoldSource(self.cat[k], self.cat[k].shape[-1], comp[0], comp[1])
            if p.head_fold:                # the 1x1 head behind the last BatchNorm takes it in its filters and bias
                t = self.stages[-1]['tail']
                t.fold_b, u.apply_in_filters = u, True
                t.bias_fold = torch.zeros(t.cout_p, dtype=torch.float32, device=dev)
        for u in [c for c in convs if c.fold_a is not None]:      # a fold reader: the border-class bias table of its epilogue
            u.cb = torch.zeros(9, u.cout_p, dtype=torch.float32, device=dev)
        nfw = max([lib.clamd_bn_fold_wgrad_workspace_bytes(B, u.cout_p) // 4 for u in convs if u.fold_a is not None] + [0])
        self.fold_ws = torch.empty(nfw, dtype=torch.float32, device=dev) if nfw else None
        self._tune_key = None
        self._plan_stat_rows()
        ws = 0
        for u in convs:      # split-K slabs of the weight-gradient kernels: at least the direct kernel's for every unit, whatever the plan
            ws = max(ws, lib.clamd_channel_sum_workspace_bytes(u.cout_p), u.g.wg_ws(lib, B, u.h, u.w_, u.cout_p, u.cin_p, self.dcode),
                     ALGOS['igemm'].wg_ws(lib, B, u.h, u.w_, u.cout_p, u.cin_p, self.dcode))
        for t in self.tails:
            mode = _lib.WGRAD_UP2 if t.kind == 'convT' else _lib.WGRAD_PW
            rp, cp_ = (t.cin_p, t.cout_p) if t.kind == 'convT' else (t.cout_p, t.cin_p)
            ws = max(ws, lib.clamd_wgrad_workspace_bytes(mode, B, H >> t.level, W >> t.level, rp, cp_, self.dcode))
        self.ws = torch.empty(ws // 4 + 16, dtype=torch.float32, device=dev)
        # scratch of the pre-transformed kernels: the transformed gradient of the data-gradient launch (main stream) and the
        # gradient-side operand of the weight-gradient GEMM (second stream); launches on one stream are serialised, so one each
        nvg = max([getattr(lib, u.d.x_elems)(B, u.h, u.w_, u.cout_p) for u in convs if u.d is not None and u.d.pre] + [0])
        nyt = max([getattr(lib, u.g.wg_elems)(B, u.h, u.w_, u.cout_p) for u in convs if u.g.pre] + [0])
        self.vg = torch.empty(nvg, dtype=torch.float32, device=dev) if nvg else None
        self.yt = torch.empty(nyt, dtype=torch.float32, device=dev) if nyt else None
        # third stream + a second operand buffer: the transform of unit u runs while the GEMM of unit u+1 still reads the other buffer
        self.x3_stream = (_side_stream(dev, 3) if (WGRAD_XFORM_STREAM and WGRAD_STREAM and dev.type == 'cuda' and (nyt or nfw)) else None)
        self.yt2 = torch.empty(nyt, dtype=torch.float32, device=dev) if (nyt and self.x3_stream is not None) else None
        self._yt_flip = 0
        self._yt_ev = [None, None]
        self._x3_ev = None
        self.wg_stream = _side_stream(dev, 2) if (WGRAD_STREAM and dev.type == 'cuda') else None
        self._wg_used = False
        self._pack_pending = 0
        self.ws_bytes = ws
        self._build_pack_table()

    # ------------------------------------------------------------------------------------------ statistics rows
    def _plan_stat_rows(self):
        """Partial-row buffers of the deterministic per-channel reductions (include/clamd.h, clamd_stat_rows): every unit
        gets stats [rows][2][Cout_p] (forward launch) and sums [rows][5][Cout_p] (whichever launch produces its five
        BatchNorm-backward sums).  Row counts depend on the kernel structure, i.e. on the tuning: re-planned when it changes."""
        key = tuple(self.tuning.as_dict().values())
        if key == self._tune_key:
            return
        self._tune_key = key
        B, dc, tn, lib = self.B, self.dcode, self.tuning, _lib.load()
        rows = _lib.stat_rows
        sizes, esz = [], []
        for u in self.convs:
            # which kernel runs a fold candidate depends on the tuning: F(2x4) Winograd / the persistent direct kernel take the table
            bb = u.f.border_bias
            u.fold_on = u.fold_a is not None and (bool(lib.clamd_conv3x3_border_bias_ok(B, u.h, u.w_, u.cin_p, u.cout_p, dc, tune_ptr(tn)))
                                                  if bb is None else bb)
            if u.fold_a is not None:
                u.fold_a.apply_in_filters = u.fold_on      # the producer's bn_apply pass is skipped
            u.gz_nrows = 0
            u.stat_rows = rows(u.f.stat_op, B, u.h, u.w_, u.cin_p, u.cout_p, dc, tuning=tn)
            src = u.sum_src
            if src is None:
                u.sum_rows = rows(_lib.OP_BN_BWD_REDUCE, B, u.h, u.w_, 1 if u.g_src[2] is not None else 0, u.cout_p, dc, tuning=tn)
            elif not hasattr(src, 'kind'):     # the 3x3 data-gradient launch of the next conv of this stage (K = its output channels)
                u.sum_rows = rows(src.d.stat_op, B, src.h, src.w_, src.cout_p, src.cin_p, dc, fused_bn=True, tuning=tn)
                # the persistent bf16 kernel takes sum g and sum g y only: the conv-bias gradient then comes from the apply pass
                if lib.clamd_conv3x3_bn_sums(B, src.h, src.w_, src.cout_p, src.cin_p, dc, tune_ptr(tn)) == 2:
                    u.gz_nrows = lib.clamd_bn_bwd_apply_sums_rows(B, u.h, u.w_, u.cout_p)
            elif src.kind == 'head':
                u.sum_rows = rows(_lib.OP_CONV1X1, B, u.h, u.w_, src.cout_p, src.cin_p, dc, fused_bn=True)
            else:                 # ConvTranspose2d data gradient: the launch runs on the convT INPUT grid (= this unit's)
                u.sum_rows = rows(_lib.OP_CONVT2X2_DGRAD, B, u.h, u.w_, src.cin_p, src.cout_p, dc, fused_bn=True)
            sizes.append((u.stat_rows * 2 + u.sum_rows * self.NS + u.gz_nrows) * u.cout_p)
            # eval-mode BatchNorm backward (clamd_bn_bwd_eval): rows [n][3][Cout_p] of the units whose sums no producing launch accumulates;
            # an arena of its own, so the train-mode buffers stay as they were
            u.eval_nrows = 0 if u.fused_reduce else lib.clamd_bn_bwd_eval_rows(B, u.h, u.w_, u.cout_p, 1 if u.g_src[2] is not None else 0)
            if u.eval_nrows < 0:
                _lib.check(u.eval_nrows, 'clamd_bn_bwd_eval_rows')
            esz.append(u.eval_nrows * 3 * u.cout_p)
        self.stat_arena = torch.empty(sum(sizes), dtype=torch.float32, device=self.dev)
        self.eval_arena = torch.empty(sum(esz), dtype=torch.float32, device=self.dev)
        off = eoff = 0
        for u, n, e in zip(self.convs, sizes, esz):
            k, k2 = u.stat_rows * 2 * u.cout_p, u.gz_nrows * u.cout_p
            u.stats = self.stat_arena[off:off + k]
            u.sums = self.stat_arena[off + k:off + n - k2]
            u.gz_rows = self.stat_arena[off + n - k2:off + n] if k2 else None
            u.eval_rows = self.eval_arena[eoff:eoff + e] if e else None
            off, eoff = off + n, eoff + e

    # ------------------------------------------------------------------------------------------ pack table
    def _build_pack_table(self):
        tab = PackTable(self.dcode)
        # ... and the plain pack in two launches too: `tab` = what the first three encoder stages need (and every bias vector), in front of
        # the forward pass; `late` = the 3x3 filters from enc4 on and the ConvTranspose / head filters (96 % of the parameters: 118 MB read,
        # 62 MB written in bf16, 130 us -- HBM-bound) on the second stream under enc1-enc3, waited for in front of enc4's first convolution
        late = PackTable(self.dcode)
        # Winograd filter transforms in two launches per form: "early" = the first three encoder stages (4 % of the parameters,
        # needed 0.3 ms into the forward pass), "late" = everything else (first needed by enc4, 2 ms in): the forward pass waits for
        # a few microseconds of packing instead of for all of it (see forward())
        wtab = {(pl, late): WinoPackTable(pl) for pl in (16, 24, 36) for late in (False, True)}
        for i, u in enumerate(self.convs):
            u.pack_late = i >= 6                                 # units 0-5 = enc1, enc2, enc3
            if u.f.taps == 1:
                tab.head(u.w, u.wf, None, 9 * u.cin, u.cout)     # im2col: [Cout][Cin*9] is already the (c*9 + tap) K order
            elif u.f.wino:
                if u.fold_a is None:
                    wtab[(u.f.taps, u.pack_late)].conv3x3(u.w, u.wf, None, u.cin_segs, u.cout)
                if u.wd is not None:
                    wtab[(u.d.taps, u.pack_late)].conv3x3(u.w, None, u.wd, u.cin_segs, u.cout)
            else:
                (late if u.pack_late else tab).conv3x3(u.w, None if u.fold_a is not None else u.wf, u.wd, u.cin_segs, u.cout)
            tab.vector(u.b, u.bias_p, u.cout)
            if u.fold_a is not None:
                # the forward filters of a fold candidate are packed inside the step, behind the producer's bn_finalize: with its scale
                # (fold on) or plain (a tuning that runs a kernel without the border-class epilogue)
                u.fold_table, u.plain_table = [(WinoPackTable(u.f.taps) if u.f.wino else PackTable(self.dcode)) for _ in range(2)]
                u.fold_table.conv3x3(u.w, u.wf, None, u.cin_segs, u.cout, kscale=u.fold_a.vec[0])
                u.plain_table.conv3x3(u.w, u.wf, None, u.cin_segs, u.cout)
                u.fold_table.finalize(self.dev); u.plain_table.finalize(self.dev)
        for t in self.tails:
            if t.kind == 'convT':
                late.convT(t.w, t.wf, t.wd, t.cin, t.cout)
            elif t.fold_b is not None:      # forward filters inside the step, with the last BatchNorm's scale (see _fwd_fold)
                late.head(t.w, None, t.wd, t.cin, t.cout)
                t.fold_table = PackTable(self.dcode)
                t.fold_table.head(t.w, t.wf, None, t.cin, t.cout, kscale=t.fold_b.vec[0])
                t.fold_table.finalize(self.dev)
            else:
                late.head(t.w, t.wf, t.wd, t.cin, t.cout)
            tab.vector(t.b, t.bias_p, t.cout)
        self.pack_table = tab.finalize(self.dev)
        self.pack_late = late.finalize(self.dev) if late.jobs else None
        self._ev_pack_late = None
        self.wino_early = [t.finalize(self.dev) for (pl, late), t in wtab.items() if t.jobs and not late]
        self.wino_late = [t.finalize(self.dev) for (pl, late), t in wtab.items() if t.jobs and late]
        self._ev_early = torch.cuda.Event() if self.dev.type == 'cuda' else None
        self._param_ptrs = [p.data_ptr() for p in self.model.parameters()]

    def _check_ptrs(self, params):
        cur = [p.data_ptr() for p in params]
        if cur != self._param_ptrs:
            # parameters were re-allocated (.to(), load from a different storage): rebuild the job table
            named = dict(zip(self.param_names, params))
            for u in self.convs:
                u.w, u.b, u.gamma, u.beta = (named[k] for k in u.keys)
            for t in self.tails:
                t.w, t.b = named[t.keys[0]], named[t.keys[1]]
            self._build_pack_table()

    # ------------------------------------------------------------------------------------------ forward
    def forward(self, x, params, predict=False):
        m = self.model
        self._bn_modes()
        if self.bn_group is not None and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('UNet.forward: SyncBatchNorm layers in train mode all-reduce their statistics, which a captured graph cannot '
                               'do; capture an unconverted model or put those layers in eval mode')
        self.generation += 1
        self.dl_src = None
        self._check_ptrs(params)
        s = _lib.stream_ptr()
        B, H, W, dc = self.B, self.H, self.W, self.dcode
        self._plan_stat_rows()
        self.pack_table.run(dc, s)
        # the Winograd filter transforms (454 MB of HBM traffic per step at config 2) are first needed by the SECOND convolution:
        # they run on the second stream under the first layer's im2col / pointwise conv / BatchNorm passes
        self._pack_pending = 0               # 2: neither part waited for yet, 1: the early part has been waited for
        sp = s
        if self.wg_stream is not None and KERNEL_TIMING is None and (self.wino_early or self.wino_late):
            self.wg_stream.wait_stream(torch.cuda.current_stream())
            sp, self._pack_pending = self.wg_stream.cuda_stream, 2
        for t in self.wino_early:
            t.run(sp)
        if self._pack_pending:
            self._ev_early.record(self.wg_stream)        # the late part is enqueued in front of the first Winograd convolution
        else:
            for t in self.wino_late:
                t.run(sp)
        self._ev_pack_late = None
        self._pack_late_pending = self.pack_late is not None      # released beside convolution PACK_LATE_AT (see _release_pack_late)
        if self.convs[0].f.taps == 1:        # im2col
            _hbm('enc1.0', B * H * W * (4 * m.in_dim + self.esize * self.x_in.shape[-1]),
                 'clamd_nchw_im2col3', ptr(x), ptr(self.x_in), self.x_in.shape[-1], B, m.in_dim, H, W, self.x_in.shape[-1], dc, s)
        else:
            call('clamd_nchw_to_nhwc', ptr(x), ptr(self.x_in), self.x_in.shape[-1], B, m.in_dim, H, W,
                 self.x_in.shape[-1], 1.0, dc, s)
        for st in self.stages:
            for u in st['convs']:
                self._fwd_pre(u, s)
                self._fwd_fold(u, s)
                self._fwd_conv(u, u.bn_train, s)
                self._fwd_finalize(u, u.bn_train, s)
                self._fwd_post(u, s)
            t = st.get('tail')
            if t is None:
                continue               # encoder: the pooled output feeds the next stage's first convolution
            self._join_pack_late()
            h, w = H >> t.level, W >> t.level
            tx, tx_ldc, tbias = t.x, t.x.shape[-1], t.bias_p
            if t.fold_b is not None:       # the head reads the last unit's conv+ReLU output: its BatchNorm is in the filters and the bias
                ft, fb = t.fold_table, t.fold_b
                call('clamd_bn_fold_pack', 0, ptr(ft.dev_table), len(ft.jobs), ft.nblocks, dc, ptr(t.w), 1, ptr(fb.vec[1]), ptr(t.b),
                     ptr(t.bias_fold), t.cout, t.cin, t.cout_p, s)
                tx, tx_ldc, tbias = fb.y, fb.cout_p, t.bias_fold
            if t.kind == 'convT':
                _hbm('convT', self.esize * (B * h * w * (t.cin + 4 * t.cout) + 4 * t.cin * t.cout),
                     'clamd_convT2x2_fwd', ptr(t.x), t.x.shape[-1], ptr(t.wf), ptr(t.bias_p), ptr(t.y_slice), t.y_ldc, B, h, w, t.cin_p, t.cout_p, dc, s)
            elif predict and t.cout_p <= 64:      # arg-max fused into the head's epilogue: the logits never reach HBM
                logits = torch.empty(B, H, W, dtype=torch.int64, device=self.dev)
                call('clamd_conv1x1_argmax', ptr(tx), tx_ldc, ptr(t.wf), ptr(tbias), ptr(logits), None, B, h, w,
                     t.cin_p, t.cout_p, self.K, dc, s)
            elif predict:      # more than 64 (padded) classes: the fused epilogue holds one 64-class slab; logits, then arg-max
                lg = torch.empty(B, self.K, H, W, dtype=torch.float32, device=self.dev)
                call('clamd_conv1x1_logits', ptr(tx), tx_ldc, ptr(t.wf), ptr(tbias), ptr(lg), B, h, w,
                     t.cin_p, t.cout_p, self.K, dc, s)
                logits = torch.empty(B, H, W, dtype=torch.int64, device=self.dev)
                call('clamd_argmax_confusion', ptr(lg), None, ptr(logits), None, B, self.K, 1, H, W, s)
            else:
                logits = torch.empty(B, self.K, H, W, dtype=torch.float32, device=self.dev)
                _hbm('head', B * h * w * (self.esize * t.cin + 4 * self.K),
                     'clamd_conv1x1_logits', ptr(tx), tx_ldc, ptr(t.wf), ptr(tbias), ptr(logits), B, h, w, t.cin_p, t.cout_p, self.K, dc, s)
        if self._pack_pending == 2:     # no Winograd layer ran at all: the late part was never enqueued
            for t in self.wino_late:
                t.run(self.wg_stream.cuda_stream)
        if self._pack_pending:          # some part was never waited for (no late Winograd layer in this net): join before returning
            torch.cuda.current_stream().wait_stream(self.wg_stream)
            self._pack_pending = 0
        self._join_pack_late()
        return logits

    def _bn_modes(self):
        """BatchNorm mode per unit, from its own module (torch's semantics: model.train() then bn.eval() freezes that layer's statistics),
        and which units all-reduce their statistics (a train-mode nn.SyncBatchNorm while a process group is initialised, syncbn.py).  The
        module is looked up in its parent every forward: a conversion after the first forward takes effect at the next one."""
        swapped = False
        for u in self.convs:
            bn = u.bn_parent._modules[u.bn_key]
            if bn is not u.bn:
                u.bn, swapped = bn, True
            u.bn_train = bool(bn.training)
        self.fwd_modes = tuple(u.bn_train for u in self.convs)
        if swapped or self._has_sync is None:
            self._has_sync = any(isinstance(u.bn, nn.SyncBatchNorm) for u in self.convs)
        self.bn_group, flags = (None, None) if not self._has_sync else syncbn.resolve([(f'{u.bn_parent_name}.{u.bn_key}', u.bn) for u in self.convs])
        for i, u in enumerate(self.convs):
            u.bn_sync = bool(flags and flags[i])
        if self.bn_group is not None and self._sync_arena is None:
            # per unit: the all-reduced [sum][sum of squares or products][count] and this rank's five backward totals, fp64
            sizes = [(2 * u.cout_p + 1, self.NS * u.cout_p) for u in self.convs]
            self._sync_arena = torch.empty(sum(a + b for a, b in sizes), dtype=torch.float64, device=self.dev)
            if self.x3_stream is not None:      # _x3_allowed asks for the measured queue count: probed here, not inside the backward pass
                from . import ddp
                ddp.hw_queues(self.dev)
            off = 0
            for u, (a, b) in zip(self.convs, sizes):
                u.sync_red, u.sync_tot = self._sync_arena[off:off + a], self._sync_arena[off + a:off + a + b]
                off += a + b

    @staticmethod
    def executed_fraction(u, direction):
        """Multiply-adds the kernel executes per algorithmic (direct-convolution) multiply-add of unit u."""
        a = getattr(u.plan, direction)
        return ALGOS[a].frac if a else 1.0

    def executed_flop_deficit(self):
        """Algorithmic minus executed FLOPs of one train step (3x3 convolutions by Winograd), for bench.py."""
        d = 0.0
        for u in self.convs:
            f = 2.0 * self.B * u.h * u.w_ * 9 * u.cin * u.cout
            for direction in ('fwd', 'wgrad') + (('dgrad',) if u.g_in is not None else ()):
                d += (1.0 - self.executed_fraction(u, direction)) * f
        return d

    def _conv_bytes(self, u):
        """Algorithmic HBM bytes of one 3x3 launch on unit u (forward, data gradient or weight gradient alike): input and
        output activation once each, filters (or their gradient) once."""
        return self.esize * (self.B * u.h * u.w_ * (u.cin + u.cout) + 9 * u.cin * u.cout)

    def _fwd_pre(self, u, s):
        """Input transform of a pre-transformed convolution (wino24g.hip)."""
        if not u.f.pre:
            return
        # the BatchNorm of the unit in front folded into the transform where nothing else reads its output (u.fold_src)
        f = u.fold_src
        xsrc, xldc, fs, fh = (f.y, f.cout_p, f.vec[0], f.vec[1]) if f is not None else (u.xin, u.xin_ldc, None, None)
        _TIMED_UNIT[:] = [u.name + ' fwd', self.executed_fraction(u, 'fwd')]
        _timed('wino_transform', 0.0, u.f.x_bytes * self.B * u.h * u.w_ * u.cin_p, u.f.xform, ptr(xsrc), xldc, ptr(fs), ptr(fh), ptr(u.vx),
               self.B, u.h, u.w_, u.cin_p, s)

    def _fwd_fold(self, u, s):
        """Forward filters of a fold candidate (bnfold.hip): packed here, behind the producer's bn_finalize -- with its scale and the
        border-class bias table when the fold is on, plain otherwise."""
        a = u.fold_a
        if a is None:
            return
        if not u.fold_on:
            u.plain_table.run(stream=s)
            return
        t = u.fold_table        # one launch: the filters times the producer's scale, and the bias table from its shift
        call('clamd_bn_fold_pack', u.f.taps if u.f.wino else 0, ptr(t.dev_table), len(t.jobs), t.nblocks, self.dcode,
             ptr(u.w), 9, ptr(a.vec[1]), ptr(u.b), ptr(u.cb), u.cout, u.cin, u.cout_p, s)

    def _release_pack_late(self):
        """Enqueues the late part of the plain filter pack: on the second stream, free to start with the convolution about to be launched on
        the current one.  Released beside enc2's first convolution, not at the start of the forward pass: the pack is HBM-bound (180 MB in
        bf16) and so are the im2col pass and the 3 -> 64-channel first layer -- beside those it only made them longer (kernel trace, round 4:
        the first layer 64 -> 160 us with the pack running), the 128 x 128 levels leave HBM bandwidth."""
        if not self._pack_late_pending:
            return
        self._pack_late_pending = False
        if self.wg_stream is not None and KERNEL_TIMING is None and self.pack_late_stream:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            self.wg_stream.wait_event(ev)
            self.pack_late.run(self.dcode, self.wg_stream.cuda_stream)
            self._ev_pack_late = torch.cuda.Event()
            self._ev_pack_late.record(self.wg_stream)
        else:
            self.pack_late.run(self.dcode, _lib.stream_ptr())

    def _join_pack_late(self):
        """The late part of the plain filter pack (second stream) is needed from here on."""
        self._release_pack_late()
        if self._ev_pack_late is not None:
            torch.cuda.current_stream().wait_event(self._ev_pack_late)
            self._ev_pack_late = None

    def _fwd_conv(self, u, training, s):
        """conv3x3 + bias + ReLU (+ BatchNorm statistics rows) of unit u."""
        dc, tp = self.dcode, tune_ptr(self.tuning)
        if u.pack_late:
            self._join_pack_late()
        elif u is self.convs[min(self.pack_late_at, len(self.convs) - 1)]:
            self._release_pack_late()
        Bl = self.B
        _TIMED_UNIT[:] = [u.name + ' fwd', self.executed_fraction(u, 'fwd')]
        rows, st, y = u.stat_rows, (u.stats if training else None), u.y
        xin, xin_ldc, bias, relu = u.xin, u.xin_ldc, u.bias_p, 1
        if u.fold_on:      # reads the producer's conv+ReLU output; its BatchNorm lives in the filters and in the bias table
            xin, xin_ldc, bias, relu = u.fold_a.y, u.fold_a.cout_p, u.cb, 3
        flops = 2.0 * Bl * u.h * u.w_ * 9 * u.cin * u.cout
        nbytes = self._conv_bytes(u)
        if u.f.taps == 1:     # im2col
            _hbm('enc1.0', self.esize * Bl * u.h * u.w_ * (u.cin_p + u.cout),
                 'clamd_conv1x1', ptr(xin), u.xin_ldc, ptr(u.wf), ptr(u.bias_p), ptr(y), u.cout_p,
                 ptr(st), None, None, rows, Bl, u.h, u.w_, u.cin_p, u.cout_p, 1, dc, s)
        elif u.f.wino:
            if self._pack_pending == 2 and (u.level >= 1 or u.pack_late):
                # the late transforms (HBM-bound, 0.3 ms) start here, under this MFMA-bound convolution, instead of beside the
                # HBM-bound first-layer kernels -- and, round 5, behind enc1's pooling pass (level >= 1): started under enc1's second
                # convolution they were still running when that pass came up and it took 141 instead of 64 us (r05h trace)
                torch.cuda.current_stream().wait_event(self._ev_early)
                self.wg_stream.wait_stream(torch.cuda.current_stream())
                for t in self.wino_late:
                    t.run(self.wg_stream.cuda_stream)
                self._pack_pending = 1
            if self._pack_pending == 1 and u.pack_late:
                torch.cuda.current_stream().wait_stream(self.wg_stream)
                self._pack_pending = 0
            if u.f.pre:
                _timed('igemm_conv3x3', flops, nbytes, u.f.conv, ptr(u.vx), ptr(u.wf), ptr(u.bias_p), ptr(y), u.cout_p,
                       ptr(st), rows, Bl, u.h, u.w_, u.cin_p, u.cout_p, 1, tp, s)
            else:
                _timed('igemm_conv3x3', flops, nbytes, u.f.conv, ptr(xin), xin_ldc, ptr(u.wf), ptr(bias), ptr(y), u.y_ldc, ptr(st), rows,
                       Bl, u.h, u.w_, u.cin_p, u.cout_p, relu, tp, s)
        else:
            _timed('igemm_conv3x3', flops, nbytes, u.f.conv, ptr(xin), xin_ldc, ptr(u.wf), ptr(bias), ptr(y), u.cout_p,
                   ptr(st), None, None, rows, Bl, u.h, u.w_, u.cin_p, u.cout_p, relu, u.m_fastest, dc, tp, s)

    def _fwd_finalize(self, u, training, s):
        v = u.vec
        if training and u.bn_sync:
            # synchronised BatchNorm: this rank's totals and pixel count, summed over the ranks, then the usual outputs from the global sums
            call('clamd_bn_rows_total', ptr(u.stats), u.stat_rows, 2, u.cout_p, float(self.B * u.h * u.w_), None, ptr(u.sync_red), s)
            syncbn.all_reduce(u.sync_red, self.bn_group)
            call('clamd_bn_finalize_total', ptr(u.sync_red), ptr(u.gamma), ptr(u.beta), ptr(u.rm), ptr(u.rv), ptr(v[0]), ptr(v[1]), ptr(v[2]),
                 ptr(v[3]), u.cout_p, u.cout, BN_MOMENTUM, BN_EPS, ptr(u.nbt), s)
            return
        call('clamd_bn_finalize', ptr(u.stats) if training else None, u.stat_rows, ptr(u.gamma), ptr(u.beta), ptr(u.rm), ptr(u.rv),
             ptr(v[0]), ptr(v[1]), ptr(v[2]), ptr(v[3]), u.cout_p, u.cout, float(self.B * u.h * u.w_), BN_MOMENTUM, BN_EPS,
             ptr(u.nbt) if training else None, s)      # num_batches_tracked += 1 inside the launch (was a torch._foreach_add_ on the critical chain)

    def _fwd_post(self, u, s):
        """BatchNorm apply (+ max-pool, concat placement) of unit u."""
        if u.apply_folded:          # the only reader of the BatchNorm output is the next convolution's input transform
            return
        if u.pool_fold:             # ... or the filters and bias tables of both readers of an encoder block's output: only the pooling is left
            _hbm('bn_fwd', self.esize * self.B * u.h * u.w_ * u.cout * 5 // 4,
                 'clamd_maxpool2x2', ptr(u.y), u.y_ldc, ptr(u.vec[0]), ptr(u.pooled), u.pooled.shape[-1], self.B, u.h, u.w_, u.cout_p, self.dcode, s)
            return
        if u.apply_in_filters:      # ... or its filters and bias table (bnfold.hip)
            return
        v = u.vec
        _hbm('bn_fwd', self.esize * self.B * u.h * u.w_ * u.cout * (9 if u.pooled is not None else 8) // 4,
             'clamd_bn_apply', ptr(u.y), u.cout_p, ptr(v[0]), ptr(v[1]), ptr(u.out), u.out_ldc,
             ptr(u.pooled), u.pooled.shape[-1] if u.pooled is not None else 0, self.B, u.h, u.w_, u.cout_p, self.dcode, s)

    # ------------------------------------------------------------------------------------------ backward
    def _wg_stream_ptr(self):
        """Stream for a parameter-gradient launch whose inputs have just been enqueued on the current stream."""
        if self.wg_stream is None or KERNEL_TIMING is not None:
            return _lib.stream_ptr()
        self.wg_stream.wait_stream(torch.cuda.current_stream())
        self._wg_used = True
        return self.wg_stream.cuda_stream

    def backward(self, gout):
        m = self.model
        s = _lib.stream_ptr()
        self._wg_used = False
        self._x3_fold = False
        self._pack_pending = 0
        self._yt_ev = [None, None]      # events of THIS backward pass only (the previous one was joined before it returned; a captured
        self._x3_ev = None              # graph must not wait on an event recorded outside the capture)
        B, H, W, dc = self.B, self.H, self.W, self.dcode
        if tuple(self.tuning.as_dict().values()) != self._tune_key:
            # the partial-row buffers were planned for the forward's kernel structure
            raise RuntimeError('model.tuning changed between forward and backward: change it between steps (before the forward)')
        if self.bn_group is not None and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('UNet.backward: SyncBatchNorm layers in train mode all-reduce their sums, which a captured graph cannot do')
        p0 = next(iter(m.parameters()))
        if p0.grad is not None:
            lo = self.gflat.data_ptr()
            if lo <= p0.grad.data_ptr() < lo + 4 * self.gflat.numel():
                # the previous gradients are still installed as .grad (no zero_grad since): accumulate semantics
                # need them intact, so this backward writes into a fresh buffer
                if m.grad_sync is not None:
                    # AccumulateGrad would add the new buffer into .grad on this stream while RCCL is still reducing it
                    # on the side stream: refuse instead of racing (the reference zeroes gradients every step, trainer.py:173)
                    raise RuntimeError('gradient accumulation (backward without zero_grad) is not supported together with '
                                       'ddp.GradSync: call optimizer.zero_grad() before every backward')
                self.gflat = torch.empty_like(self.gflat)
        base = self.gflat.data_ptr()
        g = {n: base + 4 * o for n, (o, _) in self.goffset.items()}      # raw device pointers into the flat buffer
        sync = m.grad_sync
        if sync is not None:
            sync.begin()
        self._gp = g
        tp = tune_ptr(self.tuning)
        for st in reversed(self.stages):
            t = st.get('tail')
            if t is not None:
                h, w = H >> t.level, W >> t.level
                if t.kind == 'head':
                    src = self.dl_src
                    if not (src is not None and src[1:] == (gout.data_ptr(), gout._version, self.generation)):
                        # not the tensor this package's loss wrote beside its NHWC copy (another loss, a hook, a sum of gradients): convert
                        call('clamd_nchw_to_nhwc', ptr(gout), ptr(self.dl), self.Kp, B, self.K, H, W, self.Kp, 1.0, dc, s)
                    self.dl_src = None
                    _hbm('head', self.esize * B * h * w * (self.Kp + t.cin),
                         'clamd_conv1x1', ptr(self.dl), self.Kp, ptr(t.wd), None, ptr(t.g_x), t.g_x.shape[-1], None,
                         *_sums_into(t.consumer), B, h, w, t.cout_p, t.cin_p, 0, dc, s)
                    sw = self._wg_stream_ptr()      # parameter gradients on the second stream, behind the data gradient (see _conv_bwd)
                    fb = t.fold_b
                    tx, tx_ldc = (fb.y, fb.cout_p) if fb is not None else (t.x, t.x.shape[-1])
                    _hbm('head', self.esize * B * h * w * (self.Kp + t.cin),
                         'clamd_wgrad', _lib.WGRAD_PW, ptr(self.dl), self.Kp, ptr(tx), tx_ldc, ptr(self.ws),
                         self.ws_bytes, g[t.keys[0]], B, h, w, t.cout_p, t.cin_p, t.cout, t.cin,
                         t.cout, t.cout_p, t.cin, t.cin_p, dc, tp, sw)
                    _hbm('head', 0,                # algorithmically free: d logits was just streamed by the weight gradient above
                         'clamd_channel_sum', ptr(self.dl), self.Kp, g[t.keys[1]], B * h * w, self.Kp, t.cout, dc,
                         ptr(self.ws), self.ws_bytes, tp, sw)
                    if fb is not None:      # the weight gradient ran on the un-normalised tensor: dW = scale * dW + shift * (bias gradient)
                        call('clamd_bn_fold_wgrad_pointwise', g[t.keys[1]], ptr(fb.vec[0]), ptr(fb.vec[1]), g[t.keys[0]], t.cout, t.cin, sw)
                else:
                    ctb = self.esize * (B * h * w * (t.cin + 4 * t.cout) + 4 * t.cin * t.cout)
                    _hbm('convT', ctb,
                         'clamd_convT2x2_dgrad', ptr(t.gy_slice), t.y_ldc, ptr(t.wd), ptr(t.g_x), t.g_x.shape[-1],
                         *_sums_into(t.consumer), B, h, w, t.cin_p, t.cout_p, dc, s)
                    sw = self._wg_stream_ptr()
                    _hbm('convT', ctb,
                         'clamd_wgrad', _lib.WGRAD_UP2, ptr(t.x), t.x.shape[-1], ptr(t.gy_slice), t.y_ldc, ptr(self.ws),
                         self.ws_bytes, g[t.keys[0]], B, h, w, t.cin_p, t.cout_p, t.cin, t.cout,
                         t.cin, t.cin_p, t.cout, t.cout_p, dc, tp, sw)
                    _hbm('convT', 0,               # algorithmically free: the gradient was just streamed by the weight gradient above
                         'clamd_channel_sum', ptr(t.gy_slice), t.y_ldc, g[t.keys[1]], B * 4 * h * w, t.cout_p,
                         t.cout, dc, ptr(self.ws), self.ws_bytes, tp, sw)
            for u in reversed(st['convs']):
                self._conv_bwd(u, s)
            if sync is not None:
                if self._x3_fold:       # the stage's fixed-up weight gradients belong to the bucket: the second stream (which stage_done waits for) joins the third
                    self.wg_stream.wait_stream(self.x3_stream)
                    self._x3_fold = False
                sync.stage_done(self, st)
        if self._x3_fold:
            self.wg_stream.wait_stream(self.x3_stream)
        if self._wg_used:
            torch.cuda.current_stream().wait_stream(self.wg_stream)       # every gradient is complete for whoever comes next
        gf = self.gflat
        return [gf[o:o + k].view(self.gshape[n]) for n, (o, k) in ((n, self.goffset[n]) for n in self.param_names)]

    def _x3_allowed(self):
        """The third stream only where it cannot end up on a hardware queue with RCCL's kernels: HIP multiplexes streams onto a fixed number of
        hardware queues in creation order and a kernel waits behind whatever shares its queue.  A data-parallel rank has the default stream,
        the second and third streams, GradSync's stream and RCCL's: five -- so under ddp.GradSync the third stream needs at least eight queues
        (two rounds of the assignment apart).  Synchronised BatchNorm adds the stream of its own group's communicator (six with GradSync,
        four without): any RCCL stream in play asks for the same eight.  The count is MEASURED (ddp.hw_queues: spin kernels on eight
        streams), not read from GPU_MAX_HW_QUEUES -- the runtime reads that variable once, when it starts."""
        if self.x3_stream is None or self.wg_stream is None or KERNEL_TIMING is not None:
            return False
        if self.model.grad_sync is not None or self.bn_group is not None:
            from . import ddp
            if ddp.hw_queues(self.dev) < 8:
                return False
        # hipStreamEndCapture crashes on this three-stream pattern (ROCm 7.2): a captured step keeps the transforms on the second stream
        return not torch.cuda.is_current_stream_capturing()

    def _conv_bwd(self, u, s):
        B, dc, tp = self.B, self.dcode, tune_ptr(self.tuning)
        v = u.vec
        ga, ga_ldc, gp = u.g_src
        count = float(B * u.h * u.w_)
        g = self._gp
        two = u.fused_reduce and u.gz_nrows > 0      # the producing launch took sum g and sum g y only: d conv-bias = sum g_z, from the apply pass
        if not u.bn_train and not u.fused_reduce:
            # eval-mode BatchNorm (running statistics): g_z = [y>0] scale g needs no reduction -- ONE pass writes it and the rows of
            # sum g, sum g y, sum g_z; the parameter gradients are formed off the critical chain, on the second stream, where this unit's
            # weight gradient and its fold fix-up (which read the conv-bias gradient) follow in stream order
            _hbm('bn_bwd', self.esize * B * u.h * u.w_ * u.cout * (13 if gp is not None else 12) // 4,
                 'clamd_bn_bwd_eval', ptr(ga), ga_ldc, ptr(gp), gp.shape[-1] if gp is not None else 0, ptr(u.y), u.y_ldc,
                 ptr(v[0]), ptr(v[1]), ptr(u.gz), u.cout_p, ptr(u.eval_rows), u.eval_nrows, B, u.h, u.w_, u.cout_p, u.cout, dc, s)
            call('clamd_bn_bwd_eval_finalize', ptr(u.eval_rows), u.eval_nrows, 3, ptr(v[0]), ptr(v[2]), ptr(v[3]), None,
                 g[u.keys[2]], g[u.keys[3]], g[u.keys[1]], u.cout_p, u.cout, self._wg_stream_ptr())
        else:
            if not u.bn_train:
                # eval mode where the producing data-gradient launch already accumulated the sums (DESIGN.md "Frozen BatchNorm"): the apply
                # passes of train mode with k0 = scale, k1 = k2 = 0, which the eval finalize writes from the forward's scale
                call('clamd_bn_bwd_eval_finalize', ptr(u.sums), u.sum_rows, self.NS, ptr(v[0]), ptr(v[2]), ptr(v[3]), ptr(v[4]),
                     g[u.keys[2]], g[u.keys[3]], None if two else g[u.keys[1]], u.cout_p, u.cout, s)
            else:
                if not u.fused_reduce:     # otherwise the five sums were accumulated by the epilogue of the kernel that wrote `ga`
                    _hbm('bn_bwd', 0,                      # algorithmically free: one backward pass reads g and y once (the apply pass below is charged for it)
                         'clamd_bn_bwd_reduce', ptr(ga), ga_ldc, ptr(gp), gp.shape[-1] if gp is not None else 0, ptr(u.y), u.y_ldc,
                         ptr(v[0]), ptr(v[1]), ptr(u.sums), u.sum_rows, B, u.h, u.w_, u.cout_p, dc, tp, s)
                if u.bn_sync:
                    # synchronised BatchNorm: k0, k1, k2 from sum g, sum g y and the count of all ranks (critical chain: the collective sits
                    # between this unit's sums and its apply pass); d gamma, d beta, d conv-bias from this rank's totals, as torch
                    call('clamd_bn_rows_total', ptr(u.sums), u.sum_rows, self.NS, u.cout_p, count, ptr(u.sync_tot), ptr(u.sync_red), s)
                    syncbn.all_reduce(u.sync_red, self.bn_group)
                    call('clamd_bn_bwd_finalize_total', ptr(u.sync_tot), ptr(u.sync_red), ptr(u.gamma), ptr(v[2]), ptr(v[3]), ptr(v[4]),
                         g[u.keys[2]], g[u.keys[3]], None if two else g[u.keys[1]], u.cout_p, u.cout, s)
                else:
                    call('clamd_bn_bwd_finalize', ptr(u.sums), u.sum_rows, ptr(u.gamma), ptr(v[2]), ptr(v[3]), ptr(v[4]), g[u.keys[2]],
                         g[u.keys[3]], None if two else g[u.keys[1]], u.cout_p, u.cout, count, s)
            if two:
                assert gp is None
                _hbm('bn_bwd', self.esize * B * u.h * u.w_ * u.cout * 3,
                     'clamd_bn_bwd_apply_sums', ptr(ga), ga_ldc, ptr(u.y), u.y_ldc, ptr(v[4]), ptr(u.gz), u.cout_p, ptr(u.gz_rows), u.gz_nrows,
                     B, u.h, u.w_, u.cout_p, dc, s)
            else:
                _hbm('bn_bwd', self.esize * B * u.h * u.w_ * u.cout * (13 if gp is not None else 12) // 4,
                     'clamd_bn_bwd_apply', ptr(ga), ga_ldc, ptr(gp), gp.shape[-1] if gp is not None else 0, ptr(u.y), u.y_ldc,
                     ptr(v[0]), ptr(v[1]), ptr(v[4]), ptr(u.gz), u.cout_p, B, u.h, u.w_, u.cout_p, dc, s)
        if len(u.cin_segs) == 2:
            c_seg0, c_seg0p = u.cin_segs[0]
        else:
            c_seg0, c_seg0p = u.cin, u.cin_p
        flops = 2.0 * B * u.h * u.w_ * 9 * u.cin * u.cout
        self._x3_ev = None
        if u.g.pre and self._x3_allowed():
            # gz is complete on the current stream: its weight-gradient transform goes to the third stream NOW (it runs beside whatever
            # weight-gradient GEMM the second stream is in), into the operand buffer the previous GEMM is not reading
            self._yt_flip ^= 1
            self._x3_buf = self.yt2 if self._yt_flip else self.yt
            x3 = self.x3_stream
            x3.wait_stream(torch.cuda.current_stream())
            if self._yt_ev[self._yt_flip] is not None:      # the GEMM that read this buffer last (two pre-transformed units back)
                x3.wait_event(self._yt_ev[self._yt_flip])
            call(u.g.wg_xform, ptr(u.gz), u.cout_p, ptr(self._x3_buf),
                 B, u.h, u.w_, u.cout_p, x3.cuda_stream)
            self._x3_ev = torch.cuda.Event(); self._x3_ev.record(x3)
        def dgrad():
            _TIMED_UNIT[:] = [u.name + ' dgrad', self.executed_fraction(u, 'dgrad')]
            if u.d is None:
                return
            if u.d.pre:
                _timed('wino_transform', 0.0, u.d.x_bytes * B * u.h * u.w_ * u.cout_p, u.d.xform, ptr(u.gz), u.cout_p, None, None, ptr(self.vg),
                       B, u.h, u.w_, u.cout_p, s)
                _timed('igemm_conv3x3', flops, self._conv_bytes(u), u.d.conv, ptr(self.vg), ptr(u.wd), None, ptr(u.g_in), u.g_in.shape[-1], None, 0,
                       B, u.h, u.w_, u.cout_p, u.cin_p, 0, tp, s)
            elif u.d.wino:
                _timed('igemm_conv3x3', flops, self._conv_bytes(u), u.d.conv, ptr(u.gz), u.cout_p, ptr(u.wd), None, ptr(u.g_in), u.g_in.shape[-1], None, 0,
                       B, u.h, u.w_, u.cout_p, u.cin_p, 0, tp, s)
            else:
                _timed('igemm_conv3x3', flops, self._conv_bytes(u), u.d.conv, ptr(u.gz), u.cout_p, ptr(u.wd), None, ptr(u.g_in), u.g_in.shape[-1], None,
                       *_sums_into(u.consumer), B, u.h, u.w_, u.cout_p, u.cin_p, 0, 1 if 9 * u.cin_p > B * u.h * u.w_ else 0, dc, tp, s)

        # The weight gradient may start once the data gradient of the same unit has FINISHED (the second stream's wait is
        # recorded behind it).  Started together, the dispatcher interleaves the workgroups of the two kernels, they end together
        # and the next unit's BatchNorm passes run alone again; started behind it, the weight gradient is what runs beside those
        # passes (tools/trace_gaps.py: 1.80 instead of 2.16 ms per fp32 step without an MFMA kernel).  A/B in one process:
        # bf16 +0.7 %, bf16x3 +1.0 %, fp32 unchanged (the kernels that share the chip with the passes run that much longer).
        # The issue ORDER of the two launches alone makes no difference.
        # ... except for the LAST weight gradients of the backward pass (the level-0 encoder block: nothing of the critical chain is left to run
        # beside them, the step ends with the main stream waiting for the second one -- 249 us in the r05h trace): those start as soon as
        # their gradient is ready, beside their own unit's data gradient
        early = WGRAD_TAIL_EARLY and self.dcode != _lib.BF16 and u.level == 0 and u.name.startswith('enc1')      # (bf16: 6.418 against 6.397 ms: off)
        sw = self._wg_stream_ptr() if early else None
        dgrad()
        if sw is None:
            sw = self._wg_stream_ptr()
        if two:      # off the critical chain: the fixed-order sum of the apply pass's rows, in front of this unit's weight gradient
            call('clamd_rows_sum', ptr(u.gz_rows), u.gz_nrows, g[u.keys[1]], u.cout_p, u.cout, sw)
        if u.g.taps == 1:     # im2col: a pointwise weight gradient
            _hbm('enc1.0', self.esize * B * u.h * u.w_ * (u.cout + u.cin_p),
                 u.g.wgrad, _lib.WGRAD_PW, ptr(u.gz), u.cout_p, ptr(u.xin), u.xin_ldc, ptr(self.ws), self.ws_bytes,
                 g[u.keys[0]], B, u.h, u.w_, u.cout_p, u.cin_p, u.cout, 9 * u.cin, u.cout, u.cout_p, 9 * u.cin, u.cin_p, dc, tp, sw)
            return
        _TIMED_UNIT[:] = [u.name + ' wgrad', self.executed_fraction(u, 'wgrad')]
        xin, xin_ldc = (u.fold_a.y, u.fold_a.cout_p) if u.fold_on else (u.xin, u.xin_ldc)      # a fold candidate reads the raw tensor
        if u.g.pre and self._x3_ev is not None:
            # the gradient-side operand was transformed on the third stream (enqueued when gz became ready, see below)
            self.wg_stream.wait_event(self._x3_ev)
            call(u.g.wgrad, None, u.cout_p, ptr(u.vx), ptr(self._x3_buf), ptr(self.ws), self.ws_bytes,
                 g[u.keys[0]], B, u.h, u.w_, u.cout_p, u.cin_p, u.cout, u.cin, u.cout, u.cout_p, c_seg0, c_seg0p, tp, sw)
            ev = torch.cuda.Event(); ev.record(self.wg_stream)
            self._yt_ev[self._yt_flip] = ev
            self._x3_ev = None
        elif u.g.pre:
            _timed('wgrad_conv3x3', flops, self._conv_bytes(u), u.g.wgrad, ptr(u.gz), u.cout_p, ptr(u.vx), ptr(self.yt), ptr(self.ws), self.ws_bytes,
                   g[u.keys[0]], B, u.h, u.w_, u.cout_p, u.cin_p, u.cout, u.cin, u.cout, u.cout_p, c_seg0, c_seg0p, tp, sw)
        elif u.g.wino:
            _timed('wgrad_conv3x3', flops, self._conv_bytes(u), u.g.wgrad, ptr(u.gz), u.cout_p, ptr(xin), xin_ldc, ptr(self.ws), self.ws_bytes,
                   g[u.keys[0]], B, u.h, u.w_, u.cout_p, u.cin_p, u.cout, u.cin, u.cout, u.cout_p, c_seg0, c_seg0p, tp, sw)
        else:
            _timed('wgrad_conv3x3', flops, self._conv_bytes(u),
                   u.g.wgrad, _lib.WGRAD_CONV3, ptr(u.gz), u.cout_p, ptr(xin), xin_ldc, ptr(self.ws), self.ws_bytes,
                   g[u.keys[0]], B, u.h, u.w_, u.cout_p, u.cin_p, u.cout, u.cin, u.cout, u.cout_p, c_seg0, c_seg0p, dc, tp, sw)
        if u.fold_on:
            # the weight gradient ran on the producer's conv+ReLU output r instead of x = scale * r + shift: dW = scale * dWr + shift * S, S from
            # the border sums of gz and the conv-bias gradient bn_bwd_finalize wrote above (bnfold.hip); same stream, in place
            a = u.fold_a
            fs = sw
            if self._x3_allowed():
                # two latency-bound launches of a few microseconds: on the third stream they run beside the next unit's weight gradient
                # instead of in front of it (the second stream is the longer one at the end of the bf16 backward pass)
                ev = torch.cuda.Event(); ev.record(self.wg_stream)
                self.x3_stream.wait_event(ev)
                fs, self._x3_fold = self.x3_stream.cuda_stream, True
            call('clamd_bn_fold_wgrad', ptr(u.gz), u.cout_p, g[u.keys[1]], ptr(a.vec[0]), ptr(a.vec[1]), g[u.keys[0]], ptr(self.fold_ws),
                 4 * self.fold_ws.numel(), B, u.h, u.w_, u.cout_p, u.cout, u.cin, dc, fs)
