"""Kernel plan of the UNet engine: which kernel runs each 3x3 convolution unit in each direction, and where each unit's BatchNorm
is applied and reduced.  Host-only: no tensors, no device (the 2^32-byte descriptor limits ask libclamd's size functions, which
answer on any machine).  ALGOS is the one place that maps a kernel family to its entry points, argument layout, packed filters and sizes."""
from collections import namedtuple
from typing import NamedTuple, Optional

from . import _lib
from .ops import cpad


class Algo(NamedTuple):
    layout: str                    # argument layout of its launches: 'pointwise' | 'direct' | 'wino' | 'pre' (convops.py assembles them)
    conv: str                      # forward / data-gradient launch
    wgrad: str                     # weight-gradient launch
    taps: int                      # packed filter taps: 1 pointwise (PackTable.head), 9 direct (PackTable.conv3x3), 16/24/36 Winograd planes
    stat_op: int                   # clamd_stat_rows op of its launches
    frac: float                    # multiply-adds executed per algorithmic (direct-convolution) multiply-add
    wg_ws: object                  # weight-gradient workspace bytes (lib, B, H, W, Rp, Cp, dcode)
    border_bias: Optional[bool] = False   # the forward launch takes a folded BatchNorm's border-class bias table; None: ask the tuning
    bn_sums: bool = False          # the data-gradient launch can accumulate the BatchNorm-backward sums of the unit in front
    xform: Optional[str] = None    # pre-transformed (wino24g.hip / wino44g.hip): input transform of the forward image / data-gradient operand,
    x_elems: Optional[str] = None  # its element count, and the bytes it moves per input element (reads it once, writes 3x / 2.25x its size)
    x_bytes: int = 0
    wg_xform: Optional[str] = None  # ... the gradient-side transform of the weight-gradient GEMM and its element count
    wg_elems: Optional[str] = None

    wino = property(lambda a: a.taps > 9)
    pre = property(lambda a: a.xform is not None)


ALGOS = {
    'im2col': Algo('pointwise', 'clamd_conv1x1', 'clamd_wgrad', 1, _lib.OP_CONV1X1, 1.0,
                   lambda lib, B, H, W, rp, cp, dc: lib.clamd_wgrad_workspace_bytes(_lib.WGRAD_PW, B, H, W, rp, cp, dc)),
    'igemm': Algo('direct', 'clamd_conv3x3', 'clamd_wgrad', 9, _lib.OP_CONV3X3, 1.0,
                  lambda lib, B, H, W, rp, cp, dc: lib.clamd_wgrad_workspace_bytes(_lib.WGRAD_CONV3, B, H, W, rp, cp, dc), border_bias=None, bn_sums=True),
    'f22': Algo('wino', 'clamd_conv3x3_winograd', 'clamd_wgrad_winograd', 16, _lib.OP_CONV3X3_WINOGRAD, 16 / 36,
                lambda lib, B, H, W, rp, cp, dc: lib.clamd_wgrad_winograd_workspace_bytes(rp, cp)),
    'f24': Algo('wino', 'clamd_conv3x3_winograd24', 'clamd_wgrad_winograd24', 24, _lib.OP_CONV3X3_WINOGRAD24, 24 / 72,
                lambda lib, B, H, W, rp, cp, dc: lib.clamd_wgrad_winograd24_workspace_bytes(rp, cp), border_bias=True),
    'f24_direct': Algo('wino', 'clamd_conv3x3_winograd24_direct_filters', None, 24, _lib.OP_CONV3X3_WINOGRAD24, 24 / 72, None, border_bias=True),
    'f24_pre': Algo('pre', 'clamd_conv3x3_winograd24_pre', 'clamd_wgrad_winograd24_pre', 24, _lib.OP_CONV3X3_WINOGRAD24, 24 / 72,
                    lambda lib, B, H, W, rp, cp, dc: lib.clamd_wgrad_winograd24_pre_workspace_bytes(B, H, W, rp, cp),
                    xform='clamd_winograd24_transform_input', x_elems='clamd_winograd24_input_elems', x_bytes=16,
                    wg_xform='clamd_wgrad_winograd24_pre_transform', wg_elems='clamd_wgrad_winograd24_pre_operand_elems'),
    'f44_pre': Algo('pre', 'clamd_conv3x3_winograd44_pre', 'clamd_wgrad_winograd44_pre', 36, _lib.OP_CONV3X3_WINOGRAD44, 36 / 144,
                    lambda lib, B, H, W, rp, cp, dc: lib.clamd_wgrad_winograd44_pre_workspace_bytes(B, H, W, rp, cp),
                    xform='clamd_winograd44_transform_input', x_elems='clamd_winograd44_input_elems', x_bytes=13,
                    wg_xform='clamd_wgrad_winograd44_pre_transform', wg_elems='clamd_wgrad_winograd44_pre_operand_elems'),
}
F24 = ('f24', 'f24_direct')        # F(2x4) with the transform inside the kernel: writes at any pitch, takes a bias table under every tuning

Switches = namedtuple('Switches', 'WINOGRAD WINOGRAD24 WINOGRAD24_WGRAD PRETRANSFORM WINOGRAD44 NARROW_DIRECT NARROW_PRE_WGRAD '   # of unet.py
                                 'FOLD_BN_INTO_TRANSFORM FOLD_BN_INTO_FILTERS FOLD_FILTERS_MAX_CHANNELS FOLD_POOLED FUSE_BN_SUMS')


# One 3x3 convolution unit: its geometry (cin_segs: ((logical, physical), ...), two segments for a concat input), the kernels of its
# three directions (keys of ALGOS; dgrad None: the first unit of the net has no input gradient) and where its BatchNorm goes, by name:
#   sums_by    the unit / tail layer whose data-gradient launch accumulates its five BatchNorm-backward sums (None: a reduce pass)
#   fold_src   the unit in front whose BatchNorm its input transform applies
#   fold_a     the unit in front whose BatchNorm is folded into its filters and border-class bias table (bnfold.hip)
#   pool_fold  (pooled reader, concat reader): an encoder block output whose BatchNorm lives in both readers' filters
#   head_fold  its BatchNorm lives in the 1x1 head's filters
Unit = namedtuple('Unit', 'name level h w cin_segs cin_p cout cout_p fwd dgrad wgrad sums_by fold_src fold_a pool_fold head_fold',
                  defaults=(None, None, None, None, False))


def _choose(lib, sw, B, h, w, cin_segs, cout_p, first, dcode, ncu):
    """(fwd, dgrad, wgrad) of one 3x3 unit."""
    cin, cin_p = sum(s[0] for s in cin_segs), sum(s[1] for s in cin_segs)
    # first conv (Cin = 3): 3x3 neighbourhood folded into 27 (->32) channels, conv runs as a pointwise GEMM
    if first and 9 * cin <= cpad(9 * cin) == cin_p:
        return 'im2col', None, 'im2col'
    # Winograd tiles are 2x2 outputs inside 8x16 / 16x16-pixel workgroup tiles: nothing to gain below 8x8 images
    if not (sw.WINOGRAD and dcode == _lib.F32 and (h | w) % 2 == 0 and min(h, w) >= 8):
        return 'igemm', None if first else 'igemm', 'igemm'
    if not (sw.WINOGRAD24 and w % 4 == 0):          # forward / data gradient by F(2x4,3x3)
        return 'f22', None if first else 'f22', 'f22'
    wg24 = min(h, w) >= 64 if sw.WINOGRAD24_WGRAD == 'auto' else bool(sw.WINOGRAD24_WGRAD)     # ... weight gradient
    # ... data gradient: F(2x4) tiles are 256 pixels x 64 (input) channels; a launch with at most half a chip of them runs
    # the F(2x2) kernel instead, whose 128-pixel tiles give twice the work items (1024 -> 512 @16x16, the data gradient of
    # dec1.block.0: 128 items, 238 us against 160 us, tools/wino24_ab.py)
    items24 = B * ((h + 7) // 8 * ((w + 31) // 32) if w >= 32 else (h + 15) // 16 * ((w + 15) // 16)) * ((cin_p + 63) // 64)
    dg24 = not (2 * items24 <= ncu)
    # pre-transformed operands (wino24g.hip).  Weight gradient: both channel counts multiples of 256 (a wave owns a 128 x 128
    # block, a workgroup 256 x 256).  Forward: >= 256 input channels, and either the image is needed by the weight gradient
    # anyway or there are enough output channels to amortise the transform pass (its cost grows with Cin, the kernel's gain
    # with Cin x Cout: 512 -> 256 @64x64 loses 6 %, 256 -> 128 @128x128 26 %, tools/wino24g_ab.py).  Data gradient: the
    # same with the roles of the channel counts exchanged; the transformed gradient is used once and not kept.
    pt = sw.PRETRANSFORM
    # F(4x4,3x3) applies where the launch fills the chip with (16x32-pixel tile block, 64-channel slab) work items (WINOGRAD44)
    blocks44 = B * h * w // 512                       # FULL tile blocks (a 16x16 image fills half of a 32x16 block)
    ok44 = lambda slab_ch, in_ch: (bool(sw.WINOGRAD44) and h % 4 == 0 and w % 4 == 0 and slab_ch % 64 == 0
                                   and (sw.WINOGRAD44 is True or blocks44 * (slab_ch // 64) >= ncu)
                                   and lib.clamd_winograd44_input_elems(B, h, w, in_ch) * 4 < (1 << 32))
    wg_pre = bool(pt) and cin_p % 256 == 0 and cout_p % 256 == 0
    fwd_pre = bool(pt) and cin_p >= 64 and cout_p % 64 == 0 and (
        pt is True or (cin_p >= 256 and (wg_pre or 2 * cout_p > cin_p)) or (cin_p >= 128 and cout_p >= 2 * cin_p))
    # one buffer descriptor spans a whole transformed tensor: below 2^32 bytes (config 2: <= 0.4 GB; 512 x 512 bs32 fp32: 3.2 GB)
    fits = lambda c: lib.clamd_winograd24_input_elems(B, h, w, c) * 4 < (1 << 32)
    fwd_pre = fwd_pre and fits(cin_p)
    wg_pre = wg_pre and fwd_pre and lib.clamd_wgrad_winograd24_pre_operand_elems(B, h, w, cout_p) * 4 // 24 < (1 << 32)
    dg_pre = bool(pt) and dg24 and not first and cout_p >= 64 and cin_p % 64 == 0 and fits(cout_p) and (
        pt is True or (cout_p >= 256 and (2 * cin_p > cout_p or (2 * cin_p == cout_p and cin_p >= 256))))
    # ... the 128-channel layers too (round 5: enc2.block.4, enc3.block.1, dec4 at config 2): their weight gradients ran the
    # in-kernel-transform kernel at 0.42-0.50 of the pipe; with channel counts that are multiples of 128 the plane GEMM runs them as
    # 128 x 128 wave tiles (wave-level stream-K) on the forward image, so forward AND weight gradient go pre-transformed F(4x4) and the
    # BatchNorm in front is applied by the transform (FOLD_BN_INTO_TRANSFORM) instead of by folded filters and a border-class table
    if (pt == 'auto' and sw.WINOGRAD44 and not (fwd_pre and wg_pre) and min(cin_p, cout_p) >= 128
            and cin_p % 128 == 0 and cout_p % 128 == 0 and ok44(cout_p, cin_p) and sw.NARROW_PRE_WGRAD):
        fwd_pre = wg_pre = True
    fwd44 = fwd_pre and ok44(cout_p, cin_p)            # forward (and, with wg_pre, the weight gradient: it reads the forward image)
    # ... and the data gradients of the NARROW layers whose launch has at least 128 output (= this unit's input) channels: transform of
    # the gradient + transform-free F(4x4) loop against the in-kernel-transform F(2x4) kernel, tools/wino44_narrow_ab.py: 64 -> 128
    # @256x256 1.07x, 128 -> 128 @128x128 1.08x, 128 -> 256 @128x128 1.26x, 256 -> 128 @64x64 1.21x (128 -> 64 and 64 -> 64: 0.83-0.85x)
    if (pt == 'auto' and not dg_pre and dg24 and not first and cin_p >= 128 and cout_p >= 64 and cin_p % 64 == 0
            and sw.WINOGRAD44 and ok44(cin_p, cout_p)):
        dg_pre = True
    dg44 = dg_pre and ok44(cin_p, cout_p)            # data gradient
    if fwd44 and wg_pre:
        wg_pre = lib.clamd_wgrad_winograd44_pre_operand_elems(B, h, w, cout_p) * 4 // 36 < (1 << 32)
    # 64 input channels (8 chunks per tile): the in-kernel-transform kernel with the filters loaded straight into the operand
    # registers (wino24h_kernel) is 4-6 % faster there and 1-4 % slower on longer K loops (tools/wino24h_ab.py)
    fwd_narrow = sw.NARROW_DIRECT and not fwd_pre and cin_p == 64 and cout_p % 64 == 0
    dg_narrow = sw.NARROW_DIRECT and dg24 and not dg_pre and cout_p == 64 and cin_p % 64 == 0
    fpre = 'f44_pre' if fwd44 else 'f24_pre'
    fwd = fpre if fwd_pre else ('f24_direct' if fwd_narrow else 'f24')
    dgrad = None if first else (('f44_pre' if dg44 else 'f24_pre') if dg_pre else ('f24_direct' if dg_narrow else ('f24' if dg24 else 'f22')))
    return fwd, dgrad, (fpre if wg_pre else ('f24' if wg24 else 'f22'))


def plan_net(table, B, H, W, dcode, sw, ncu=256):
    """One Unit per 3x3 convolution of unet.stage_table `table` (two per stage, in order) at input [B, *, H, W]."""
    lib = _lib.load()
    units = []
    for i, st in enumerate(table):              # enc1-enc4 at levels 0-3, dec1 at level 4, dec2-dec4 and last back up at 3-0
        level, pre = (i if i < 4 else 8 - i), st['name'] + ('.block' if st['wrapped'] else '')
        (c0, _, cin, mid), (c1, _, _, _) = st['convs']
        segs = ((cin // 2, cpad(cin // 2)),) * 2 if i > 4 else ((cin, cpad(cin)),)       # behind dec1: [skip | up-convolution]
        for ci, segs in ((c0, segs), (c1, ((mid, cpad(mid)),))):
            h, w, first = H >> level, W >> level, i == 0 and ci == c0
            fwd, dgrad, wgrad = _choose(lib, sw, B, h, w, segs, cpad(mid), first, dcode, ncu)
            units.append(dict(name=f'{pre}.{ci}', level=level, h=h, w=w, cin_segs=segs, cin_p=sum(s[1] for s in segs), cout=mid,
                              cout_p=cpad(mid), fwd=fwd, dgrad=dgrad, wgrad=wgrad))
        a, b = units[-2:]
        # b's data-gradient launch (K = b's output channels) also reduces a's BatchNorm-backward sums: not the Winograd kernels, which have no such
        # epilogue (round 4: built with two sums in the statistics registers, measured 21.06 -> 21.11 ms per step, removed: the reduce passes it
        # replaces run beside a weight gradient); 'auto' = the persistent bf16 kernel: <= 256 input channels, K-steps in pairs (64 channels)
        auto = dcode == _lib.BF16 and b['cout_p'] <= 256 and b['cout_p'] % 64 == 0
        if ALGOS[b['dgrad']].bn_sums and (auto if sw.FUSE_BN_SUMS == 'auto' else sw.FUSE_BN_SUMS):
            a['sums_by'] = b['name']
        if st['tail'] is not None and sw.FUSE_BN_SUMS is True:     # b's gradient comes from the tail's data-gradient kernel
            b['sums_by'] = f"{pre}.{st['tail'][1]}"
        # a's BatchNorm output is read by b's convolution (forward) and by b's weight gradient only: when both run on b's transformed
        # input, the affine is applied by the transform itself and a's bn_apply pass (and its output) disappears
        if sw.FOLD_BN_INTO_TRANSFORM and ALGOS[b['fwd']].pre and ALGOS[b['wgrad']].pre:
            b['fold_src'] = a['name']
        # ... and where b transforms inside its kernel (or is a bf16 direct kernel): the algebraic fold of bnfold.hip
        elif sw.FOLD_BN_INTO_FILTERS and not ALGOS[b['fwd']].pre and min(b['h'], b['w']) >= 2 and b['cin_p'] <= sw.FOLD_FILTERS_MAX_CHANNELS:
            b['fold_a'] = a['name']
        # ... and the 1x1 head behind the last BatchNorm: pointwise, no border classes -- in every compute dtype
        if st['tail'] is not None and st['tail'][0] == 'head' and sw.FOLD_BN_INTO_FILTERS and b['cout_p'] <= sw.FOLD_FILTERS_MAX_CHANNELS:
            b['head_fold'] = True
    for k in range(3):
        # ... and the output of an encoder block with two narrow F(2x4) readers (FOLD_POOLED): static (fp32 Winograd kernels take the
        # border-class table under every tuning), because the raw tensor then lives where the normalised one would
        b, nxt, dec = units[2 * k + 1], units[2 * k + 2], units[2 * (8 - k)]      # dec: the decoder convolution reading the concat of level k
        if (sw.FOLD_POOLED and sw.FOLD_BN_INTO_FILTERS and dcode == _lib.F32 and b['fwd'] in F24 and b['cout'] == b['cout_p']
                and all(c['fwd'] in F24 and c['cin_p'] <= sw.FOLD_FILTERS_MAX_CHANNELS and all(lg == ph for lg, ph in c['cin_segs'])
                        for c in (nxt, dec))):
            b['pool_fold'] = (nxt['name'], dec['name'])
    return tuple(Unit(**u) for u in units)
