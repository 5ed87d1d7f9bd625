"""The engine behind ``UNet.forward``: the kernel plan (plan.py) of one input shape turned into buffers, typed units and the fixed launch
schedules of the forward and backward pass.  `_Unit` / `_Tail` declare what a convolution unit and a ConvTranspose / head layer own;
`_Streams` owns the side streams and every wait between them; `_Engine` allocates, wires the BatchNorm placement and launches.  The
switches and KERNEL_TIMING are attributes of unet.py (tests, tools and bench.py assign them there) and are read from it when used."""
import weakref
from functools import partial

import torch
import torch.nn as nn

from . import _lib, bnops, convops, syncbn, unet as U
from ._lib import call, ptr, tune_ptr
from .ops import PackTable, WinoPackTable, cpad
from .plan import ALGOS, plan_net

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


def _timed(tag, flops, nbytes, unit, name, *args):
    """A launch; with unet.KERNEL_TIMING set, between two HIP events on the current stream.  `unit` = (conv unit and direction, fraction
    of its algorithmic FLOPs the kernel executes -- Winograd: 16/36 or 24/72): _Unit.tag."""
    kt = U.KERNEL_TIMING
    if kt is None:         # _lib.call written out: the launches of a step come through here, and every Python frame in between is host time per launch
        rc = getattr(_lib.load(), name)(*args)
        if rc:
            _lib.check(rc, name)
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call(name, *args)
    e1.record()
    kt.append((tag, flops, e0, e1, nbytes, unit[0], unit[1]))


def _hbm(family, nbytes, name, *args):
    """A launch of an HBM-bound kernel family (A5 / A6 BatchNorm and pooling passes, A7 ConvTranspose, A9 head, A10 loss,
    A13 Adam, enc1.0) with its ALGORITHMIC bytes -- every tensor it has to read or write, once: timed per launch by bench.py's instrumented
    steps (`hbm_kernels` on the JSON line), a plain launch otherwise."""
    _timed('hbm:' + family, 0.0, nbytes, ('', 1.0), name, *args)


def _hbm_run(family, nbytes):
    """_hbm with family and bytes bound: the `run` of a convops launch."""
    return partial(_timed, 'hbm:' + family, 0.0, nbytes, ('', 1.0))


class _FoldSource:
    """What a folded convolution reads instead of a normalised tensor: the raw tensor (`y`, pitch `cout_p`) and the per-input-channel
    scale / shift (`vec[0]`, `vec[1]`) that live in its filters and bias table -- the interface of the producing _Unit the pair fold uses."""
    __slots__ = ('y', 'cout_p', 'vec', 'apply_in_filters')

    def __init__(self, y, pitch, scale, shift):
        self.y, self.cout_p, self.vec, self.apply_in_filters = y, pitch, [scale, shift], False


def _sums_into(c):
    """convops' `fused`: the data-gradient launch accumulates the BatchNorm-backward sums of unit c (plan.Unit.sums_by), or None."""
    return (ptr(c.y), ptr(c.sums), c.sum_rows) if c is not None else None


class _Declared:
    """Every field is declared in __slots__ and exists from construction on: None until the engine fills it, None for good where unused."""
    __slots__ = ()

    def __init__(self):
        for k in self.__slots__:
            setattr(self, k, None)


class _Unit(_Declared):
    """One Conv3x3 -> ReLU -> BatchNorm unit and everything it needs in both directions."""
    __slots__ = (
        # ---- plan and geometry
        'plan', 'name', 'f', 'd', 'g',      # plan.Unit, module path; plan.ALGOS families of forward, data gradient (None at enc1.0), weight gradient
        'tag',                              # direction -> (name + ' ' + direction, executed fraction of the algorithmic FLOPs), for _timed
        'level', 'h', 'width',              # pooling level and image size there
        'cin', 'cin_p', 'cout', 'cout_p', 'cin_segs',       # logical / padded channels; [(logical, physical), ...] input segments (two behind a concat)
        # ---- parameters (re-read by _check_ptrs) and the BatchNorm module
        'w', 'b', 'gamma', 'beta', 'keys',  # conv weight and bias, BatchNorm weight and bias; their names (offsets into the flat gradient buffer)
        'rm', 'rv', 'nbt',                  # running mean, running variance, num_batches_tracked
        'bn', 'bn_parent', 'bn_parent_name', 'bn_key',      # the BatchNorm module and where it lives (convert_sync_batchnorm swaps it)
        'bn_train', 'bn_sync',              # at the last forward: batch statistics?  all-reduced over the group?
        # ---- buffers
        'xin', 'xin_ldc', 'y', 'y_ldc',     # input activation, conv + ReLU output (saved for backward), their channel pitches
        'out', 'out_ldc', 'pooled',         # BatchNorm output, its pitch, its 2x2 max-pool (encoder block outputs only)
        'gz', 'g_in', 'g_src',              # d y; data-gradient target (None at enc1.0); (d out, its pitch, d pooled or None)
        'vx',                               # pre-transformed input, kept for the weight gradient (None unless f.pre)
        'wf', 'wd', 'bias_p', 'pack_late',  # packed forward / data-gradient (None at enc1.0) filters, padded bias; packed by the late tables?
        'vec',                              # seven [Cout_p] rows: scale, shift, mean, istd, k0, k1, k2 (4-6 contiguous)
        # ---- BatchNorm placement (from the plan; one direction only, no cycles)
        'consumer', 'sum_src', 'fused_reduce',      # unit whose backward sums our data gradient accumulates; _Unit / _Tail that accumulates ours (is not None)
        'fold_src', 'apply_folded',         # unit whose BatchNorm our input transform applies; ours is applied by a reader's transform
        'fold_a', 'fold_on',                # _Unit / _FoldSource whose BatchNorm lives in our filters; whether this tuning's kernel takes it
        'cb', 'fold_table', 'plain_table',  # of a fold reader: border-class bias table, pack tables with / without the producer's scale
        'apply_in_filters', 'pool_fold',    # our BatchNorm lives in the readers' filters; ... of an encoder block output: only the pooling is left
        # ---- per-tuning row counts and views of the statistics arenas (_plan_stat_rows); 0 / None where unused
        'stat_rows', 'stats', 'sum_rows', 'sums',           # forward partial rows [rows][2][Cout_p], backward [rows][5][Cout_p]
        'gz_nrows', 'gz_rows',              # sum g_z rows of the apply pass (the persistent bf16 kernel takes two sums only)
        'eval_nrows', 'eval_rows',          # rows [n][3][Cout_p] of clamd_bn_bwd_eval
        # ---- SyncBatchNorm scratch (fp64, allocated at the first synchronised forward)
        'sync_red', 'sync_tot')             # all-reduced [sum][sum sq or products][count]; this rank's five backward totals
    # read-only views of the plan that bench.py reads (nothing in this package uses them)
    wino = property(lambda u: u.f.wino)
    w24 = property(lambda u: u.plan.fwd in ('f24', 'f24_direct', 'f24_pre', 'f44_pre'))
    f44 = property(lambda u: u.plan.fwd == 'f44_pre')
    pre_f = property(lambda u: u.f.pre)
    pre_d = property(lambda u: u.d is not None and u.d.pre)


class _Tail(_Declared):
    """The layer behind a decoder block's two units: ConvTranspose2d 2x2 ('convT') or the 1x1 head ('head')."""
    __slots__ = (
        'kind', 'level', 'cin', 'cin_p', 'cout', 'cout_p',  # 'convT' | 'head'; pooling level of its INPUT; logical / padded channels
        'w', 'b', 'keys', 'wf', 'wd', 'bias_p',             # weight, bias, their names; packed forward / data-gradient filters, padded bias
        'x', 'g_x',                         # input (the block's BatchNorm output) and the gradient w.r.t. it
        'y_slice', 'gy_slice', 'y_ldc',     # convT: output and its gradient = second half of the concat buffers one level up, their pitch
        'consumer',                         # unit whose backward sums the data gradient accumulates, or None
        'fold_b', 'bias_fold', 'fold_table')    # head: unit whose BatchNorm lives in the filters, the folded bias, the pack table with its scale


class _Streams:
    """The second and third HIP stream of an engine and every wait between the three.  Second stream: parameter gradients and the filter
    packs the forward pass does not need at once.  Third: the gradient-side transforms of the pre-transformed weight gradients and the fold
    fix-ups.  Each operation enqueues the waits / records it names and nothing else; with no side stream (CPU planning, WGRAD_STREAM
    off) or while bench.py times single launches, everything is handed the current stream and no wait is issued."""

    def __init__(self, dev, want_third):
        cuda = dev.type == 'cuda' and bool(U.WGRAD_STREAM)
        self.dev = dev
        self.x3 = _side_stream(dev, 3) if (cuda and U.WGRAD_XFORM_STREAM and want_third) else None      # (created first, as ever: queue assignment)
        self.wg = _side_stream(dev, 2) if cuda else None
        self.late_on_side = bool(U.PACK_LATE_STREAM)
        self._ev_early = torch.cuda.Event() if dev.type == 'cuda' else None
        self._pack_pending = 0              # Winograd filter transforms: 2 = neither part waited for yet, 1 = the early part has been
        self._pack_late_pending, self._ev_pack_late = False, None
        self._wg_used = self._x3_fold = self._third = False
        self._yt_flip, self._yt_ev, self._x3_ev, self._x3_buf = 0, [None, None], None, None

    def _single(self):
        """One stream: no side stream, or bench.py / tools/layer_table.py time every launch alone."""
        return self.wg is None or U.KERNEL_TIMING is not None

    # ---- forward: filter packs
    def start_packs(self, wino_early, wino_late, pack_late, dcode):
        """The Winograd filter transforms (454 MB of HBM traffic per step at config 2) are first needed by the SECOND convolution: the early
        part (enc1-enc3) runs on the second stream under the first layer's im2col / pointwise conv / BatchNorm passes, the late part is
        enqueued in front of the first Winograd convolution (need_wino_filters).  The late plain pack waits for release_late_pack."""
        self._wino_late, self._late, self._dcode = wino_late, pack_late, dcode
        self._pack_pending, sp = 0, _lib.stream_ptr()
        if not self._single() and (wino_early or wino_late):
            self.wg.wait_stream(torch.cuda.current_stream())
            sp, self._pack_pending = self.wg.cuda_stream, 2
        for t in wino_early:
            t.run(sp)
        if self._pack_pending:
            self._ev_early.record(self.wg)
        else:
            for t in wino_late:
                t.run(sp)
        self._ev_pack_late, self._pack_late_pending = None, pack_late is not None

    def release_late_pack(self):
        """Enqueues the late part of the plain filter pack: on the second stream, free to start with the convolution about to be launched on
        the current one.  Released beside enc2's first convolution, not at the start of the forward pass: the pack is HBM-bound (180 MB in
        bf16) and so are the im2col pass and the 3 -> 64-channel first layer -- beside those it only made them longer (kernel trace, round 4:
        the first layer 64 -> 160 us with the pack running), the 128 x 128 levels leave HBM bandwidth."""
        if not self._pack_late_pending:
            return
        self._pack_late_pending = False
        if not self._single() and self.late_on_side:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            self.wg.wait_event(ev)
            self._late.run(self._dcode, self.wg.cuda_stream)
            self._ev_pack_late = torch.cuda.Event()
            self._ev_pack_late.record(self.wg)
        else:
            self._late.run(self._dcode, _lib.stream_ptr())

    def need_late_pack(self):
        """The late part of the plain filter pack is needed from here on."""
        self.release_late_pack()
        if self._ev_pack_late is not None:
            torch.cuda.current_stream().wait_event(self._ev_pack_late)
            self._ev_pack_late = None

    def need_wino_filters(self, u):
        """In front of the Winograd convolution of unit u."""
        if self._pack_pending == 2 and (u.level >= 1 or u.pack_late):
            # the late transforms (HBM-bound, 0.3 ms) start here, under this MFMA-bound convolution, instead of beside the
            # HBM-bound first-layer kernels -- and, round 5, behind enc1's pooling pass (level >= 1): started under enc1's second
            # convolution they were still running when that pass came up and it took 141 instead of 64 us (r05h trace)
            torch.cuda.current_stream().wait_event(self._ev_early)
            self.wg.wait_stream(torch.cuda.current_stream())
            for t in self._wino_late:
                t.run(self.wg.cuda_stream)
            self._pack_pending = 1
        if self._pack_pending == 1 and u.pack_late:
            torch.cuda.current_stream().wait_stream(self.wg)
            self._pack_pending = 0

    def join_forward(self):
        if self._pack_pending == 2:     # no Winograd layer ran at all: the late part was never enqueued
            for t in self._wino_late:
                t.run(self.wg.cuda_stream)
        if self._pack_pending:          # some part was never waited for (no late Winograd layer in this net): join before returning
            torch.cuda.current_stream().wait_stream(self.wg)
            self._pack_pending = 0
        self.need_late_pack()

    # ---- backward
    def start_backward(self, rccl):
        """`rccl`: a collective's stream is in play (ddp.GradSync, or synchronised BatchNorm).  Decides once whether this pass uses the
        third stream -- only where it cannot end up on a hardware queue with RCCL's kernels: HIP multiplexes streams onto a fixed number of
        hardware queues in creation order and a kernel waits behind whatever shares its queue.  A data-parallel rank has the default stream,
        the second and third streams, GradSync's stream and RCCL's: five -- so under ddp.GradSync the third stream needs at least eight queues
        (two rounds of the assignment apart).  Synchronised BatchNorm adds the stream of its own group's communicator (six with GradSync,
        four without): any RCCL stream in play asks for the same eight.  The count is MEASURED (ddp.hw_queues: spin kernels on eight
        streams), not read from GPU_MAX_HW_QUEUES -- the runtime reads that variable once, when it starts."""
        self._wg_used = self._x3_fold = False
        self._pack_pending = 0
        self._yt_ev, self._x3_ev = [None, None], None      # events of THIS backward pass only (the previous one was joined before it returned; a
        #                                                    captured graph must not wait on an event recorded outside the capture)
        self._third = self.x3 is not None and not self._single()
        if self._third and rccl:
            from . import ddp
            self._third = ddp.hw_queues(self.dev) >= 8
        # hipStreamEndCapture crashes on this three-stream pattern (ROCm 7.2): a captured step keeps the transforms on the second stream
        self._third = self._third and not torch.cuda.is_current_stream_capturing()

    def param_grad_stream(self):
        """Stream for a parameter-gradient launch whose inputs have just been enqueued on the current stream."""
        if self._single():
            return _lib.stream_ptr()
        self.wg.wait_stream(torch.cuda.current_stream())
        self._wg_used = True
        return self.wg.cuda_stream

    def gradient_stream(self):
        """The second stream if this backward pass has put parameter gradients on it (ddp.GradSync waits for it), else None."""
        return self.wg if self._wg_used else None

    def wgrad_transform_stream(self, bufs):
        """gz is complete on the current stream: its weight-gradient transform goes to the third stream NOW (it runs beside whatever
        weight-gradient GEMM the second stream is in), into the operand buffer of `bufs` the previous GEMM is not reading.  Returns
        (stream, buffer), or (None, None): transform on the second stream, in front of its GEMM."""
        if not self._third:
            return None, None
        self._yt_flip ^= 1
        self._x3_buf = bufs[self._yt_flip]
        self.x3.wait_stream(torch.cuda.current_stream())
        if self._yt_ev[self._yt_flip] is not None:      # the GEMM that read this buffer last (two pre-transformed units back)
            self.x3.wait_event(self._yt_ev[self._yt_flip])
        return self.x3.cuda_stream, self._x3_buf

    def wgrad_transformed(self):
        self._x3_ev = torch.cuda.Event()
        self._x3_ev.record(self.x3)

    def wgrad_after_transform(self):
        """The second stream's next launch (the GEMM) reads the operand the third stream transformed ..."""
        self.wg.wait_event(self._x3_ev)

    def wgrad_operand_read(self):
        """... and has been enqueued: behind it the buffer is free for the transform two pre-transformed units on."""
        self._yt_ev[self._yt_flip], self._x3_ev = torch.cuda.Event(), None
        self._yt_ev[self._yt_flip].record(self.wg)

    def fold_fixup_stream(self, sw):
        """Stream of a fold fix-up behind the weight gradient on `sw`: two latency-bound launches of a few microseconds: on the third stream
        they run beside the next unit's weight gradient instead of in front of it (the second stream is the longer one at the end of the
        bf16 backward pass)."""
        if not self._third:
            return sw
        ev = torch.cuda.Event()
        ev.record(self.wg)
        self.x3.wait_event(ev)
        self._x3_fold = True
        return self.x3.cuda_stream

    def join_stage(self):
        """A stage's fixed-up weight gradients belong to its bucket: the second stream (which ddp.GradSync.stage_done waits for) joins the third."""
        if self._x3_fold:
            self.wg.wait_stream(self.x3)
            self._x3_fold = False

    def join_backward(self):
        self.join_stage()
        if self._wg_used:
            torch.cuda.current_stream().wait_stream(self.wg)       # every gradient is complete for whoever comes next


class _Engine:
    @property
    def model(self):
        return self._model_ref()

    def __init__(self, model, B, H, W, device):
        lib = _lib.load()
        self._model_ref = weakref.ref(model)      # the model owns its engines; a strong reference back would leave the
        #                                           multi-GB activation buffers to the cyclic garbage collector
        self.B, self.H, self.W, self.dev = B, H, W, device
        self.dcode, self.tdtype = U._DTYPES[model.compute_dtype]
        self.pack_late_at = int(U.PACK_LATE_AT)      # index of the convolution unit the late plain pack is released beside
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
            u = _Unit()
            u.plan, u.name = p, p.name
            u.f, u.d, u.g = ALGOS[p.fwd], p.dgrad and ALGOS[p.dgrad], ALGOS[p.wgrad]      # kernel families of the three directions
            u.w, u.b = named[f'{prefix}.{ci}.weight'], named[f'{prefix}.{ci}.bias']
            u.gamma, u.beta = named[f'{prefix}.{bi}.weight'], named[f'{prefix}.{bi}.bias']
            u.rm, u.rv = bufs[f'{prefix}.{bi}.running_mean'], bufs[f'{prefix}.{bi}.running_var']
            u.nbt = bufs[f'{prefix}.{bi}.num_batches_tracked']
            u.bn, u.bn_train = mods[f'{prefix}.{bi}'], True         # its .training is the unit's BatchNorm mode (read every forward)
            u.bn_parent, u.bn_parent_name, u.bn_key, u.bn_sync = mods[prefix], prefix, str(bi), False
            u.keys = (f'{prefix}.{ci}.weight', f'{prefix}.{ci}.bias', f'{prefix}.{bi}.weight', f'{prefix}.{bi}.bias')
            u.level, u.h, u.width, u.cin_p, u.cout, u.cout_p = p.level, p.h, p.w, p.cin_p, p.cout, p.cout_p
            u.cin_segs, u.cin = list(p.cin_segs), sum(s[0] for s in p.cin_segs)      # [(logical, physical), ...] one or two segments
            u.xin, u.xin_ldc = xin, xin.shape[-1]
            u.y, u.gz = act(p.level, u.cout_p), act(p.level, u.cout_p)
            u.vx = torch.empty(getattr(lib, u.f.x_elems)(B, u.h, u.width, u.cin_p), dtype=torch.float32, device=dev) if u.f.pre else None
            u.wf = torch.zeros(u.f.taps * u.cout_p * u.cin_p, dtype=T, device=dev)      # Winograd: [Cin_p/8][16|24|36][Cout_p][8] transformed
            u.wd = None if u.d is None else torch.zeros(u.d.taps * u.cin_p * u.cout_p, dtype=T, device=dev)
            u.bias_p = torch.zeros(u.cout_p, dtype=torch.float32, device=dev)
            u.vec = list(torch.zeros(7, u.cout_p, dtype=torch.float32, device=dev))
            u.y_ldc = u.cout_p
            u.fused_reduce = p.sums_by is not None                            # BatchNorm placement: wired from the plan below
            u.tag = {k: (f'{p.name} {k}', ALGOS[a].frac if a else 1.0) for k, a in (('fwd', p.fwd), ('dgrad', p.dgrad), ('wgrad', p.wgrad))}
            u.apply_folded = u.apply_in_filters = u.fold_on = u.pool_fold = False
            return u

        ncu = torch.cuda.get_device_properties(dev).multi_processor_count if dev.type == 'cuda' else 256
        self.plan = plan_net(model._table, B, H, W, self.dcode, U.switches(), ncu)
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
            tail = tails[f'{pre}.{ti}'] = _Tail()
            tail.w, tail.b = named[f'{pre}.{ti}.weight'], named[f'{pre}.{ti}.bias']
            tail.keys = (f'{pre}.{ti}.weight', f'{pre}.{ti}.bias')
            tail.cin, tail.cin_p, tail.cout, tail.cout_p = tcin, cpad(tcin), tcout, cpad(tcout)
            tail.kind, tail.x, tail.g_x, tail.level = kind, b.out, g_ub, k
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
                u.vec = [comp[0, :u.cout_p], comp[1, :u.cout_p]] + u.vec[2:]     # rows 4-6 (k0, k1, k2) stay contiguous
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
            ws = max(ws, lib.clamd_channel_sum_workspace_bytes(u.cout_p), u.g.wg_ws(lib, B, u.h, u.width, u.cout_p, u.cin_p, self.dcode),
                     ALGOS['igemm'].wg_ws(lib, B, u.h, u.width, u.cout_p, u.cin_p, self.dcode))
        for t in self.tails:
            ws = max(ws, convops.tail_workspace_bytes(lib, t.kind, B, H >> t.level, W >> t.level, t.cin_p, t.cout_p, self.dcode))
        self.ws = torch.empty(convops.workspace_floats(ws), dtype=torch.float32, device=dev)
        # scratch of the pre-transformed kernels: the transformed gradient of the data-gradient launch (main stream) and the
        # gradient-side operand of the weight-gradient GEMM (second stream); launches on one stream are serialised, so one each
        nvg = max([getattr(lib, u.d.x_elems)(B, u.h, u.width, u.cout_p) for u in convs if u.d is not None and u.d.pre] + [0])
        nyt = max([getattr(lib, u.g.wg_elems)(B, u.h, u.width, u.cout_p) for u in convs if u.g.pre] + [0])
        self.vg = torch.empty(nvg, dtype=torch.float32, device=dev) if nvg else None
        self.yt = torch.empty(nyt, dtype=torch.float32, device=dev) if nyt else None
        # third stream + a second operand buffer: the transform of unit u runs while the GEMM of unit u+1 still reads the other buffer
        self.streams = _Streams(dev, bool(nyt or nfw))
        self.yt2 = torch.empty(nyt, dtype=torch.float32, device=dev) if (nyt and self.streams.x3 is not None) else None
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
            u.fold_on = u.fold_a is not None and (bool(lib.clamd_conv3x3_border_bias_ok(B, u.h, u.width, u.cin_p, u.cout_p, dc, tune_ptr(tn)))
                                                  if bb is None else bb)
            if u.fold_a is not None:
                u.fold_a.apply_in_filters = u.fold_on      # the producer's bn_apply pass is skipped
            u.gz_nrows = 0
            u.stat_rows = rows(u.f.stat_op, B, u.h, u.width, u.cin_p, u.cout_p, dc, tuning=tn)
            src = u.sum_src
            if src is None:
                u.sum_rows = rows(_lib.OP_BN_BWD_REDUCE, B, u.h, u.width, 1 if u.g_src[2] is not None else 0, u.cout_p, dc, tuning=tn)
            elif isinstance(src, _Unit):       # the 3x3 data-gradient launch of the next conv of this stage (K = its output channels)
                u.sum_rows = rows(src.d.stat_op, B, src.h, src.width, src.cout_p, src.cin_p, dc, fused_bn=True, tuning=tn)
                # the persistent bf16 kernel takes sum g and sum g y only: the conv-bias gradient then comes from the apply pass
                if lib.clamd_conv3x3_bn_sums(B, src.h, src.width, src.cout_p, src.cin_p, dc, tune_ptr(tn)) == 2:
                    u.gz_nrows = lib.clamd_bn_bwd_apply_sums_rows(B, u.h, u.width, u.cout_p)
            elif src.kind == 'head':
                u.sum_rows = rows(_lib.OP_CONV1X1, B, u.h, u.width, src.cout_p, src.cin_p, dc, fused_bn=True)
            else:                 # ConvTranspose2d data gradient: the launch runs on the convT INPUT grid (= this unit's)
                u.sum_rows = rows(_lib.OP_CONVT2X2_DGRAD, B, u.h, u.width, src.cin_p, src.cout_p, dc, fused_bn=True)
            sizes.append((u.stat_rows * 2 + u.sum_rows * self.NS + u.gz_nrows) * u.cout_p)
            # eval-mode BatchNorm backward (clamd_bn_bwd_eval): rows [n][3][Cout_p] of the units whose sums no producing launch accumulates;
            # an arena of its own, so the train-mode buffers stay as they were
            u.eval_nrows = 0 if u.fused_reduce else lib.clamd_bn_bwd_eval_rows(B, u.h, u.width, u.cout_p, 1 if u.g_src[2] is not None else 0)
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
        self.wino_early = [t.finalize(self.dev) for (pl, late), t in wtab.items() if t.jobs and not late]
        self.wino_late = [t.finalize(self.dev) for (pl, late), t in wtab.items() if t.jobs and late]
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
        st_ = self.streams
        st_.start_packs(self.wino_early, self.wino_late, self.pack_late, dc)
        if self.convs[0].f.taps == 1:        # im2col
            _hbm('enc1.0', B * H * W * (4 * m.in_dim + self.esize * self.x_in.shape[-1]),
                 'clamd_nchw_im2col3', ptr(x), ptr(self.x_in), self.x_in.shape[-1], B, m.in_dim, H, W, self.x_in.shape[-1], dc, s)
        else:
            call('clamd_nchw_to_nhwc', ptr(x), ptr(self.x_in), self.x_in.shape[-1], B, m.in_dim, H, W, self.x_in.shape[-1], 1.0, dc, s)
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
            st_.need_late_pack()
            h, w = H >> t.level, W >> t.level
            tx, tx_ldc, tbias = t.x, t.x.shape[-1], t.bias_p
            if t.fold_b is not None:       # the head reads the last unit's conv+ReLU output: its BatchNorm is in the filters and the bias
                ft, fb = t.fold_table, t.fold_b
                call('clamd_bn_fold_pack', 0, ptr(ft.dev_table), len(ft.jobs), ft.nblocks, dc, ptr(t.w), 1, ptr(fb.vec[1]), ptr(t.b),
                     ptr(t.bias_fold), t.cout, t.cin, t.cout_p, s)
                tx, tx_ldc, tbias = fb.y, fb.cout_p, t.bias_fold
            if t.kind == 'convT':
                convops.convT_fwd(_hbm_run('convT', self.esize * (B * h * w * (t.cin + 4 * t.cout) + 4 * t.cin * t.cout)),
                                  ptr(t.x), t.x.shape[-1], ptr(t.wf), ptr(t.bias_p), ptr(t.y_slice), t.y_ldc, B, h, w, t.cin_p, t.cout_p, dc, s)
                continue
            head, geo = (ptr(tx), tx_ldc, ptr(t.wf), ptr(tbias)), (B, h, w, t.cin_p, t.cout_p, self.K, dc, s)
            if predict and t.cout_p <= 64:      # arg-max fused into the head's epilogue: the logits never reach HBM
                logits = torch.empty(B, H, W, dtype=torch.int64, device=self.dev)
                convops.head_fwd(call, *head, None, ptr(logits), *geo)
            elif predict:      # more than 64 (padded) classes: the fused epilogue holds one 64-class slab; logits, then arg-max
                lg = torch.empty(B, self.K, H, W, dtype=torch.float32, device=self.dev)
                convops.head_fwd(call, *head, ptr(lg), None, *geo)
                logits = torch.empty(B, H, W, dtype=torch.int64, device=self.dev)
                call('clamd_argmax_confusion', ptr(lg), None, ptr(logits), None, B, self.K, 1, H, W, s)
            else:
                logits = torch.empty(B, self.K, H, W, dtype=torch.float32, device=self.dev)
                convops.head_fwd(_hbm_run('head', B * h * w * (self.esize * t.cin + 4 * self.K)), *head, ptr(logits), None, *geo)
        st_.join_forward()
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
            if self.streams.x3 is not None:     # _Streams.start_backward asks for the measured queue count: probed here, not inside the backward pass
                from . import ddp
                ddp.hw_queues(self.dev)
            off = 0
            for u, (a, b) in zip(self.convs, sizes):
                u.sync_red, u.sync_tot = self._sync_arena[off:off + a], self._sync_arena[off + a:off + a + b]
                off += a + b

    def executed_flop_deficit(self):
        """Algorithmic minus executed FLOPs of one train step (3x3 convolutions by Winograd), for bench.py."""
        d = 0.0
        for u in self.convs:
            f = 2.0 * self.B * u.h * u.width * 9 * u.cin * u.cout
            for direction in ('fwd', 'wgrad') + (('dgrad',) if u.g_in is not None else ()):
                d += (1.0 - u.tag[direction][1]) * f
        return d

    def _conv_bytes(self, u):
        """Algorithmic HBM bytes of one 3x3 launch on unit u (forward, data gradient or weight gradient alike): input and
        output activation once each, filters (or their gradient) once."""
        return self.esize * (self.B * u.h * u.width * (u.cin + u.cout) + 9 * u.cin * u.cout)

    def _fwd_pre(self, u, s):
        """Input transform of a pre-transformed convolution (wino24g.hip)."""
        if not u.f.pre:
            return
        # the BatchNorm of the unit in front folded into the transform where nothing else reads its output (u.fold_src)
        f = u.fold_src
        xsrc, xldc, fs, fh = (f.y, f.cout_p, f.vec[0], f.vec[1]) if f is not None else (u.xin, u.xin_ldc, None, None)
        convops.wino_transform(partial(_timed, 'wino_transform', 0.0, u.f.x_bytes * self.B * u.h * u.width * u.cin_p, u.tag['fwd']), u.f,
                               ptr(xsrc), xldc, ptr(fs), ptr(fh), ptr(u.vx), self.B, u.h, u.width, u.cin_p, s)

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

    def _fwd_conv(self, u, training, s):
        """conv3x3 + bias + ReLU (+ BatchNorm statistics rows) of unit u."""
        if u.pack_late:
            self.streams.need_late_pack()
        elif u is self.convs[min(self.pack_late_at, len(self.convs) - 1)]:
            self.streams.release_late_pack()
        if u.f.wino:
            self.streams.need_wino_filters(u)
        Bl = self.B
        xin, xin_ldc, bias, relu = u.xin, u.xin_ldc, u.bias_p, 1
        if u.fold_on:      # reads the producer's conv+ReLU output; its BatchNorm lives in the filters and in the bias table
            xin, xin_ldc, bias, relu = u.fold_a.y, u.fold_a.cout_p, u.cb, 3
        if u.f.taps == 1:     # im2col: HBM-bound, timed as such
            run = _hbm_run('enc1.0', self.esize * Bl * u.h * u.width * (u.cin_p + u.cout))
        else:
            run = partial(_timed, 'igemm_conv3x3', 2.0 * Bl * u.h * u.width * 9 * u.cin * u.cout, self._conv_bytes(u), u.tag['fwd'])
        convops.conv3x3(run, u.f, ptr(xin), xin_ldc, ptr(u.vx), ptr(u.wf), ptr(bias), ptr(u.y), u.y_ldc, ptr(u.stats if training else None), u.stat_rows,
                        None, Bl, u.h, u.width, u.cin_p, u.cout_p, relu, self.dcode, tune_ptr(self.tuning), s)

    def _fwd_finalize(self, u, training, s):
        # (num_batches_tracked += 1 inside the launch: it was a torch._foreach_add_ on the critical chain)
        bnops.fwd_finalize(u.stats, u.stat_rows, u.gamma, u.beta, u.rm, u.rv, u.nbt, u.vec, u.cout_p, u.cout, float(self.B * u.h * u.width),
                           training, s, u.sync_red if u.bn_sync else None, self.bn_group)

    def _fwd_post(self, u, s):
        """BatchNorm apply (+ max-pool, concat placement) of unit u."""
        if u.apply_folded:          # the only reader of the BatchNorm output is the next convolution's input transform
            return
        if u.pool_fold:             # ... or the filters and bias tables of both readers of an encoder block's output: only the pooling is left
            convops.maxpool(_hbm_run('bn_fwd', self.esize * self.B * u.h * u.width * u.cout * 5 // 4),
                            ptr(u.y), u.y_ldc, ptr(u.vec[0]), ptr(u.pooled), u.pooled.shape[-1], self.B, u.h, u.width, u.cout_p, self.dcode, s)
            return
        if u.apply_in_filters:      # ... or its filters and bias table (bnfold.hip)
            return
        v = u.vec
        convops.bn_apply(_hbm_run('bn_fwd', self.esize * self.B * u.h * u.width * u.cout * (9 if u.pooled is not None else 8) // 4),
                         ptr(u.y), u.cout_p, ptr(v[0]), ptr(v[1]), ptr(u.out), u.out_ldc,
                         ptr(u.pooled), u.pooled.shape[-1] if u.pooled is not None else 0, self.B, u.h, u.width, u.cout_p, self.dcode, s)

    # ------------------------------------------------------------------------------------------ backward
    def backward(self, gout):
        m = self.model
        s = _lib.stream_ptr()
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
        sync, streams = m.grad_sync, self.streams
        streams.start_backward(sync is not None or self.bn_group is not None)
        if sync is not None:
            sync.begin()
        self._gp = g
        tp = tune_ptr(self.tuning)
        for st in reversed(self.stages):
            t = st.get('tail')
            if t is not None:
                h, w = H >> t.level, W >> t.level
                gy, gy_ldc, tx, tx_ldc, fb = t.gy_slice, t.y_ldc, t.x, t.x.shape[-1], t.fold_b
                nbytes = self.esize * (B * h * w * (t.cin + 4 * t.cout) + 4 * t.cin * t.cout)
                if t.kind == 'head':
                    src = self.dl_src
                    if not (src is not None and src[1:] == (gout.data_ptr(), gout._version, self.generation)):
                        # not the tensor this package's loss wrote beside its NHWC copy (another loss, a hook, a sum of gradients): convert
                        call('clamd_nchw_to_nhwc', ptr(gout), ptr(self.dl), self.Kp, B, self.K, H, W, self.Kp, 1.0, dc, s)
                    self.dl_src = None
                    gy, gy_ldc, nbytes = self.dl, self.Kp, self.esize * B * h * w * (self.Kp + t.cin)
                    if fb is not None:      # the folded head read the last unit's conv+ReLU output
                        tx, tx_ldc = fb.y, fb.cout_p
                run = _hbm_run(t.kind, nbytes)
                convops.tail_dgrad(run, t.kind, ptr(gy), gy_ldc, ptr(t.wd), ptr(t.g_x), t.g_x.shape[-1], _sums_into(t.consumer),
                                   B, h, w, t.cin_p, t.cout_p, dc, s)
                sw = self.streams.param_grad_stream()      # parameter gradients on the second stream, behind the data gradient (see _conv_bwd)
                convops.tail_wgrad(run, t.kind, ptr(tx), tx_ldc, ptr(gy), gy_ldc, ptr(self.ws), self.ws_bytes, g[t.keys[0]],
                                   B, h, w, t.cin, t.cin_p, t.cout, t.cout_p, dc, tp, sw)
                # algorithmically free: the gradient was just streamed by the weight gradient above
                convops.tail_bias_grad(_hbm_run(t.kind, 0), t.kind, ptr(gy), gy_ldc, g[t.keys[1]], B, h, w, t.cout, t.cout_p, dc,
                                       ptr(self.ws), self.ws_bytes, tp, sw)
                if fb is not None:      # the weight gradient ran on the un-normalised tensor: dW = scale * dW + shift * (bias gradient)
                    call('clamd_bn_fold_wgrad_pointwise', g[t.keys[1]], ptr(fb.vec[0]), ptr(fb.vec[1]), g[t.keys[0]], t.cout, t.cin, sw)
            for u in reversed(st['convs']):
                self._conv_bwd(u, s)
            if sync is not None:
                streams.join_stage()
                sync.stage_done(self, st)
        streams.join_backward()
        gf = self.gflat
        return [gf[o:o + k].view(self.gshape[n]) for n, (o, k) in ((n, self.goffset[n]) for n in self.param_names)]

    def _conv_bwd(self, u, s):
        B, dc, tp, streams = self.B, self.dcode, tune_ptr(self.tuning), self.streams
        v, g = u.vec, self._gp
        ga, ga_ldc, gp = u.g_src
        gp_ldc = gp.shape[-1] if gp is not None else 0
        count = float(B * u.h * u.width)
        dgamma, dbeta, dbias = g[u.keys[2]], g[u.keys[3]], g[u.keys[1]]
        two = u.fused_reduce and u.gz_nrows > 0      # the producing launch took sum g and sum g y only: d conv-bias = sum g_z, from the apply pass
        if not u.bn_train and not u.fused_reduce:
            # eval-mode BatchNorm (running statistics): g_z = [y>0] scale g needs no reduction -- ONE pass writes it and the rows of
            # sum g, sum g y, sum g_z; the parameter gradients are formed off the critical chain, on the second stream, where this unit's
            # weight gradient and its fold fix-up (which read the conv-bias gradient) follow in stream order
            convops.bn_bwd_eval(_hbm_run('bn_bwd', self.esize * B * u.h * u.width * u.cout * (13 if gp is not None else 12) // 4),
                                ptr(ga), ga_ldc, ptr(gp), gp_ldc, ptr(u.y), u.y_ldc,
                                ptr(v[0]), ptr(v[1]), ptr(u.gz), u.cout_p, ptr(u.eval_rows), u.eval_nrows, B, u.h, u.width, u.cout_p, u.cout, dc, s)
            bnops.bwd_eval_finalize(u.eval_rows, u.eval_nrows, 3, v, False, dgamma, dbeta, dbias, u.cout_p, u.cout, streams.param_grad_stream())
        else:
            if not u.bn_train:
                # eval mode where the producing data-gradient launch already accumulated the sums (DESIGN.md "Frozen BatchNorm"): the apply
                # passes of train mode with k0 = scale, k1 = k2 = 0, which the eval finalize writes from the forward's scale
                bnops.bwd_eval_finalize(u.sums, u.sum_rows, self.NS, v, True, dgamma, dbeta, None if two else dbias, u.cout_p, u.cout, s)
            else:
                if not u.fused_reduce:     # otherwise the five sums were accumulated by the epilogue of the kernel that wrote `ga`
                    # algorithmically free: one backward pass reads g and y once (the apply pass below is charged for it)
                    convops.bn_bwd_reduce(_hbm_run('bn_bwd', 0), ptr(ga), ga_ldc, ptr(gp), gp_ldc, ptr(u.y), u.y_ldc,
                                          ptr(v[0]), ptr(v[1]), ptr(u.sums), u.sum_rows, B, u.h, u.width, u.cout_p, dc, tp, s)
                bnops.bwd_finalize(u.sums, u.sum_rows, self.NS, u.gamma, v, dgamma, dbeta, None if two else dbias, u.cout_p, u.cout, count, s,
                                   (u.sync_tot, u.sync_red) if u.bn_sync else None, self.bn_group)
            if two:
                assert gp is None
                convops.bn_bwd_apply_sums(_hbm_run('bn_bwd', self.esize * B * u.h * u.width * u.cout * 3),
                                          ptr(ga), ga_ldc, ptr(u.y), u.y_ldc, ptr(v[4]), ptr(u.gz), u.cout_p, ptr(u.gz_rows), u.gz_nrows,
                                          B, u.h, u.width, u.cout_p, dc, s)
            else:
                convops.bn_bwd_apply(_hbm_run('bn_bwd', self.esize * B * u.h * u.width * u.cout * (13 if gp is not None else 12) // 4),
                                     ptr(ga), ga_ldc, ptr(gp), gp_ldc, ptr(u.y), u.y_ldc,
                                     ptr(v[0]), ptr(v[1]), ptr(v[4]), ptr(u.gz), u.cout_p, B, u.h, u.width, u.cout_p, dc, s)
        c_seg0, c_seg0p = u.cin_segs[0] if len(u.cin_segs) == 2 else (u.cin, u.cin_p)
        flops, nbytes = 2.0 * B * u.h * u.width * 9 * u.cin * u.cout, self._conv_bytes(u)
        gz_arg, yt = ptr(u.gz), self.yt       # a pre-transformed weight gradient transforms gz into yt itself, in front of its GEMM ...
        if u.g.pre:                           # ... unless the third stream does: then the GEMM takes no gz and reads the buffer it was given
            sx, buf = streams.wgrad_transform_stream((self.yt, self.yt2))
            if sx is not None:
                convops.wgrad_transform(call, u.g, gz_arg, u.cout_p, ptr(buf), B, u.h, u.width, u.cout_p, sx)
                streams.wgrad_transformed()
                gz_arg, yt = None, buf
        # The weight gradient may start once the data gradient of the same unit has FINISHED (the second stream's wait is
        # recorded behind it).  Started together, the dispatcher interleaves the workgroups of the two kernels, they end together
        # and the next unit's BatchNorm passes run alone again; started behind it, the weight gradient is what runs beside those
        # passes (tools/trace_gaps.py: 1.80 instead of 2.16 ms per fp32 step without an MFMA kernel).  A/B in one process:
        # bf16 +0.7 %, bf16x3 +1.0 %, fp32 unchanged (the kernels that share the chip with the passes run that much longer).
        # The issue ORDER of the two launches alone makes no difference.
        # ... except for the LAST weight gradients of the backward pass (the level-0 encoder block: nothing of the critical chain is left to run
        # beside them, the step ends with the main stream waiting for the second one -- 249 us in the r05h trace): those start as soon as
        # their gradient is ready, beside their own unit's data gradient
        early = U.WGRAD_TAIL_EARLY and dc != _lib.BF16 and u.level == 0 and u.name.startswith('enc1')      # (bf16: 6.418 against 6.397 ms: off)
        sw = streams.param_grad_stream() if early else None
        if u.d is not None:
            tag, gi = u.tag['dgrad'], u.g_in
            if u.d.pre:       # the transformed gradient is used once and not kept
                convops.wino_transform(partial(_timed, 'wino_transform', 0.0, u.d.x_bytes * B * u.h * u.width * u.cout_p, tag), u.d,
                                       ptr(u.gz), u.cout_p, None, None, ptr(self.vg), B, u.h, u.width, u.cout_p, s)
            convops.conv3x3(partial(_timed, 'igemm_conv3x3', flops, nbytes, tag), u.d, ptr(u.gz), u.cout_p, ptr(self.vg), ptr(u.wd), None,
                            ptr(gi), gi.shape[-1], None, 0, _sums_into(u.consumer), B, u.h, u.width, u.cout_p, u.cin_p, 0, dc, tp, s)
        if sw is None:
            sw = streams.param_grad_stream()
        if two:      # off the critical chain: the fixed-order sum of the apply pass's rows, in front of this unit's weight gradient
            call('clamd_rows_sum', ptr(u.gz_rows), u.gz_nrows, dbias, u.cout_p, u.cout, sw)
        if u.g.taps == 1:     # im2col: a pointwise weight gradient, HBM-bound and timed as such
            run = _hbm_run('enc1.0', self.esize * B * u.h * u.width * (u.cout + u.cin_p))
        else:
            run = partial(_timed, 'wgrad_conv3x3', flops, nbytes, u.tag['wgrad'])
        xin, xin_ldc = (u.fold_a.y, u.fold_a.cout_p) if u.fold_on else (u.xin, u.xin_ldc)      # a fold candidate reads the raw tensor
        if gz_arg is None:
            streams.wgrad_after_transform()
        convops.wgrad3x3(run, u.g, gz_arg, u.cout_p, ptr(xin), xin_ldc, ptr(u.vx), ptr(yt), ptr(self.ws), self.ws_bytes, g[u.keys[0]],
                         B, u.h, u.width, u.cout_p, u.cin_p, u.cout, u.cin, c_seg0, c_seg0p, dc, tp, sw)
        if gz_arg is None:
            streams.wgrad_operand_read()
        if u.fold_on:
            # the weight gradient ran on the producer's conv+ReLU output r instead of x = scale * r + shift: dW = scale * dWr + shift * S, S from
            # the border sums of gz and the conv-bias gradient bn_bwd_finalize wrote above (bnfold.hip); behind it, in place
            a = u.fold_a
            call('clamd_bn_fold_wgrad', ptr(u.gz), u.cout_p, dbias, ptr(a.vec[0]), ptr(a.vec[1]), g[u.keys[0]], ptr(self.fold_ws),
                 4 * self.fold_ws.numel(), B, u.h, u.width, u.cout_p, u.cout, u.cin, dc, streams.fold_fixup_stream(sw))
