"""GPU: the cross-entropy + soft Dice loss (clamd_ce_dice_fwd_bwd, csrc/loss.hip) per element over the grid its dispatch can launch, then
the criterion module, the hand-over of d logits to the UNet's backward pass and the trainer.

Method of test_loss_grid_gpu.py: every case calls the C ABI directly -- outputs poisoned inside guard bands, the workspace poisoned -- and
compares with tests/dice_ref.py in float64 on the same inputs (autograd through the loss; never another call into libclamd.so):
    |d logits - grad_scale * ref| <= c * 2^-24 * s_px        for every element,
    s_px = grad_scale * (w_ce / max(N, 1) + 2 max_k (|a_gk| + c_gk)) on a valid pixel of group g, from the reference's float64 coefficients;
a pixel with s_px == 0 is exactly zero.  The loss parts keep 1e-5 * max(1, |ref|), loss3[0] == loss3[1] + loss3[2] as an fp32 sum, both label
counters exact, the NHWC copy is the converted NCHW gradient bit for bit with channels K .. 31 zero, two calls give the same bits.
How c was obtained: every case also evaluates the header's closed form in torch float32 (dice_ref.closed_form on float32 logits: softmax
relative to the pixel's maximum, the sums by torch.sum) and prints `fp32 r` = max |err| / (2^-24 * s_px) of that restatement beside `kernel
r`; C_BOUND is the largest `fp32 r` over this file's cases (RESTATEMENT_MAX, recorded in DESIGN.md) times 4 -- expf / logf a few ulp off
torch's, the order of the sums -- rounded up to a power of two.  A kernel above the bound is a finding in loss.hip.

Grid: workgroup = (image, chunk); an image has cpi = min(ceil(items / 256), 2048 // B) chunks of 256 lanes, items = H W / 4 quads in the
four-pixel form and H W pixels in the one-pixel form; a capped workgroup loops.
  dice_sums_kernel / dice_grad_kernel<8|16|24|32, 4, NT>   test_class_boundaries K = 1,8 | 9,16 | 17,24 | 25,32, every NT, 2 x 8 x 12
  several images inside what would be one wave            test_several_images: B = 6, 4 x 4 (six workgroups of four live lanes)
  <32, 1, NT>                                             test_one_pixel_form: 5 x 7 and 3 x 3; misaligned logits, d logits, labels at 8 x 12
  second trip                                             test_second_trip: 9 x 484 x 484 and 1 x 725 x 725 (numbers in its docstring)"""
import math
from types import SimpleNamespace

import pytest
import torch

import dice_ref
from test_loss_grid_gpu import EPS, GUARD, NHWC, POISON, _check_nhwc, _guarded, _guards_intact

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
# the largest fp32-restatement ratio over this file's cases (torch float32 closed form against float64 autograd; every case prints its own) ...
RESTATEMENT_MAX = 2.52      # measured 2.51 to two places: background only, first_class 1 (test_degenerate_sets); _check holds every case to it
# ... times 4, rounded up to a power of two
C_BOUND = 2.0 ** math.ceil(math.log2(4.0 * RESTATEMENT_MAX))
BOUNDARY_K = [1, 8, 9, 16, 17, 24, 25, 32]
OPTS = dict(w_ce=1.0, w_dice=1.0, smooth=1e-5, first_class=0, present_only=True, per_image=False)


@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    C._lib.load()
    return C


# ------------------------------------------------------------------------------------------------------------------------------ inputs
def _case(K, B, H, W, scale, seed=0, ign=-100):
    """Class K - 1 absent from the whole batch (K >= 2), class 1 absent from image 0 (K >= 3); ignored pixels, an out-of-range label
    (K + 2) and a negative non-ignore one (-7), planted as test_loss_grid_gpu._case plants them."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, K, H, W, generator=g) * scale
    y = torch.randint(0, max(K - 1, 1), (B, H, W), generator=g)
    if K >= 3:
        y[0][y[0] == 1] = 0
    y[0, 0, :3] = ign; y[0, 1, 0] = K + 2; y[-1, -1, -1] = -7
    return SimpleNamespace(K=K, B=B, H=H, W=W, ign=ign, z=z, y=y, zd=z.to(DEV), yd=y.to(DEV))


def _opts(**kw):
    return dict(OPTS, **kw)


# --------------------------------------------------------------------------------------------------------------------------- reference
def _reference(cs, o):
    kw = dict(o, ignore_index=cs.ign)
    zz = cs.zd.double().requires_grad_()
    tot, ce, dice = dice_ref.dice_ce(zz, cs.yd, **kw)
    g64, = torch.autograd.grad(tot, zz)
    g32 = dice_ref.closed_form(cs.zd, cs.yd, **kw)
    s1, nvalid, nbad = dice_ref.pixel_scale(cs.zd.double(), cs.yd, 1.0, **kw)
    live = (s1 > 0)[:, None].expand_as(g64)
    r32 = float(((g32.double() - g64).abs() / (EPS * s1[:, None]))[live].max()) if bool(live.any()) else 0.0
    return SimpleNamespace(l3=[float(tot.detach()), float(ce.detach()), float(dice.detach())], g=g64, s1=s1, live=live, nvalid=nvalid, nbad=nbad, r32=r32)


# ----------------------------------------------------------------------------------------------------------------------------- the ABI
def _abi(C, cs, o, gs=1.0, variant=NHWC[0], z=None, y=None, d_shift=0):
    """One call of clamd_ce_dice_fwd_bwd -> loss3, d logits, NHWC copy or None, N_valid, N_bad.  d logits and the copy live inside poisoned
    buffers whose guard bands are checked here; the workspace is poisoned (NaN bits) and exactly as large as the library asks."""
    lib, ptr, s = C._lib, C._lib.ptr, C._lib.stream_ptr()
    L = lib.load()
    B, K, H, W = cs.B, cs.K, cs.H, cs.W
    z = cs.zd if z is None else z
    y = cs.yd if y is None else y
    wsb = L.clamd_ce_dice_workspace_bytes(B, K, H, W, int(o['per_image']))
    assert wsb > 0 and wsb % 4 == 0
    off = L.clamd_ce_bad_label_count_offset() // 4
    wbuf, ws = _guarded((wsb // 4,), torch.float32, fill=float('nan'))
    dbuf, d = _guarded((B, K, H, W), torch.float32, fill=float('nan'), shift=d_shift)
    l3 = torch.full((3,), float('nan'), device=DEV)
    name, dcode, ldc = variant
    nbuf = nh = None
    if name is not None:
        nbuf, nh = _guarded((B, H, W, ldc), C.ops.TORCH_DT[dcode])
    lib.call('clamd_ce_dice_fwd_bwd', ptr(z), ptr(y), ptr(d), ptr(nh), ldc, dcode, ptr(l3), ptr(ws), wsb, B, K, H, W, cs.ign,
             float(o['w_ce']), float(o['w_dice']), float(o['smooth']), int(o['first_class']), int(o['present_only']), int(o['per_image']),
             float(gs), s)
    torch.cuda.synchronize()
    assert _guards_intact(dbuf, d), 'a store outside d logits'
    assert _guards_intact(wbuf, ws), 'a store outside the workspace'
    if nh is not None:
        assert _guards_intact(nbuf, nh), 'a store outside the NHWC copy'
    counts = ws[off - 1:off + 1].view(torch.int32).tolist()
    return SimpleNamespace(l3=l3, d=d, nh=nh, nvalid=counts[0], nbad=counts[1])


def _check(what, got, ref, gs=1.0):
    """The per-element bound, the exact zeros, the loss parts, their fp32 sum, the counters."""
    assert (got.nvalid, got.nbad) == (ref.nvalid, ref.nbad), (what, got.nvalid, got.nbad, ref.nvalid, ref.nbad)
    errs = [abs(float(a) - b) / max(1.0, abs(b)) for a, b in zip(got.l3, ref.l3)]
    assert bool(torch.isfinite(got.d).all()), what
    nz = int((got.d[~ref.live] != 0).sum())
    ratio = (got.d.double() - gs * ref.g).abs() / (EPS * gs * ref.s1[:, None])
    rk = float(ratio[ref.live].max()) if bool(ref.live.any()) else 0.0
    print(f'{what}: fp32 r {ref.r32:.2f}, kernel r {rk:.2f} (c {C_BOUND:g}), loss rel errors {["%.1e" % e for e in errs]}')
    assert ref.r32 <= RESTATEMENT_MAX, (what, 'the restatement ratio c was derived from has grown: derive c again', ref.r32)
    assert rk <= C_BOUND, (what, rk, C_BOUND, ref.r32)
    assert nz == 0, f'{what}: {nz} non-zero elements on pixels without a gradient'
    assert max(errs) < 1e-5, (what, errs, got.l3.tolist(), ref.l3)
    assert torch.equal(got.l3[0], got.l3[1] + got.l3[2]), (what, got.l3.tolist())


def _same_bits(a, b):
    return torch.equal(a.d.view(torch.int32), b.d.view(torch.int32)) and torch.equal(a.l3.view(torch.int32), b.l3.view(torch.int32))


def _all_variants(C, what, cs, o, ref, gs=1.0, variants=NHWC, **kw):
    """The entry point without and with every NHWC copy: each call against the reference, the copies against the converted gradient, and
    d logits / loss the same bits whatever the copy and from one call to the next.  -> the call without a copy."""
    first = None
    for v in variants:
        got = _abi(C, cs, o, gs, v, **kw)
        _check(f'{what} nhwc {v[0]}/{v[2]}', got, ref, gs)
        if v[0] is not None:
            _check_nhwc(C, what, got, v, cs.K)
        if first is None:
            first = got
        else:
            assert _same_bits(got, first), (what, v)
    return first


# ------------------------------------------------------------------------------------------- class-count boundaries, four pixels per thread
@pytest.mark.parametrize('first_class', [0, 1])
@pytest.mark.parametrize('per_image', [False, True])
@pytest.mark.parametrize('K', BOUNDARY_K)
def test_class_boundaries(C, K, per_image, first_class):
    """2 x 8 x 12: 24 quads per image, one workgroup per image with 232 dead lanes (three whole waves); every NHWC variant."""
    for scale in (3.0, 30.0):
        cs = _case(K, 2, 8, 12, scale, seed=K)
        o = _opts(per_image=per_image, first_class=first_class)
        ref = _reference(cs, o)
        assert ref.nbad == 2
        _all_variants(C, f'K{K} x{scale} per_image{int(per_image)} first{first_class}', cs, o, ref)
    o2 = _opts(per_image=per_image, first_class=first_class, present_only=False, w_ce=0.5, w_dice=2.0, smooth=1.0)
    _all_variants(C, f'K{K} all classes, weights, smooth 1', cs, o2, _reference(cs, o2), gs=0.375, variants=(NHWC[0], NHWC[3], NHWC[6]))


@pytest.mark.parametrize('per_image', [False, True])
def test_several_images(C, per_image):
    """B = 6, 4 x 4: the 24 quads a single wave of ce4_kernel covers; here six workgroups, each inside its image."""
    for K in (5, 21):
        cs = _case(K, 6, 4, 4, 3.0, seed=K + 100)
        o = _opts(per_image=per_image)
        _all_variants(C, f'6x4x4 K{K} per_image{int(per_image)}', cs, o, _reference(cs, o), variants=(NHWC[0], NHWC[3], NHWC[6]))


# --------------------------------------------------------------------------------------------------------------- one pixel per thread
def _shifted(t, shift=1):
    """A copy of t that starts `shift` elements behind a 64-byte boundary."""
    buf = torch.zeros(t.numel() + 16 + shift, dtype=t.dtype, device=DEV)
    base = (-buf.data_ptr() // buf.element_size()) % (64 // buf.element_size())
    v = buf[base + shift:base + shift + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 64 == shift * buf.element_size()
    return v


@pytest.mark.parametrize('per_image', [False, True])
@pytest.mark.parametrize('K', [8, 17, 32])
def test_one_pixel_form(C, K, per_image):
    """H * W % 4 != 0 (2 x 5 x 7 and 2 x 3 x 3), and 8 x 12 with logits, d logits or labels off the four-pixel form's alignment (4 bytes
    behind a 16-byte boundary; labels 8 bytes behind a 32-byte boundary): <32, 1, NT> of both per-pixel passes."""
    o = _opts(per_image=per_image, first_class=1)
    for H, W in ((5, 7), (3, 3)):
        cs = _case(K, 2, H, W, 3.0, seed=K + H)
        _all_variants(C, f'{H}x{W} K{K}', cs, o, _reference(cs, o))
    cs = _case(K, 2, 8, 12, 30.0, seed=K)
    ref = _reference(cs, o)
    aligned = _abi(C, cs, o)
    for what, kw in (('logits', dict(z=_shifted(cs.zd))), ('labels', dict(y=_shifted(cs.yd))), ('d logits', dict(d_shift=1))):
        if what == 'labels':
            assert kw['y'].data_ptr() % 32 == 8
        got = _all_variants(C, f'8x12 K{K} misaligned {what}', cs, o, ref, variants=(NHWC[0], NHWC[2], NHWC[3], NHWC[5]), **kw)
        # the same pixels in another summation order: the loss agrees to rounding, no bit-equality is claimed
        assert max(abs(float(a) - float(b)) for a, b in zip(got.l3, aligned.l3)) < 1e-5


# ------------------------------------------------------------------------------------------------------------------- degenerate sets
@pytest.mark.parametrize('per_image', [False, True])
def test_degenerate_sets(C, per_image):
    cs = _case(5, 2, 8, 12, 3.0, seed=3)
    variants = (NHWC[0], NHWC[3])
    # every pixel ignored: total 0, gradient 0 -- with and without present_only, with smooth 0 too (D == 0: dice 1)
    gone = SimpleNamespace(**{**vars(cs), 'y': torch.full_like(cs.y, cs.ign), 'yd': torch.full_like(cs.yd, cs.ign)})
    for kw in (dict(), dict(present_only=False), dict(present_only=False, smooth=0.0)):
        o = _opts(per_image=per_image, **kw)
        ref = _reference(gone, o)
        got = _all_variants(C, f'all ignored {kw}', gone, o, ref, variants=variants)
        assert ref.nvalid == 0 and got.l3.tolist() == [0.0, 0.0, 0.0] and float(got.d.abs().max()) == 0.0
    # present_only with no class at or above first_class present: the Dice term is 0 and has no gradient
    bg = cs.y.clone()
    bg[(bg >= 0) & (bg < 5)] = 0
    only_bg = SimpleNamespace(**{**vars(cs), 'y': bg, 'yd': bg.to(DEV)})
    o = _opts(per_image=per_image, first_class=1)
    got = _all_variants(C, 'background only, first_class 1', only_bg, o, _reference(only_bg, o), variants=variants)
    assert float(got.l3[2]) == 0.0 and float(got.l3[1]) > 0
    o0 = _opts(per_image=per_image, first_class=1, w_ce=0.0)       # ... and without the CE term nothing is left: s_px == 0 everywhere
    got = _all_variants(C, 'background only, first_class 1, w_ce 0', only_bg, o0, _reference(only_bg, o0), variants=variants)
    assert got.l3.tolist() == [0.0, 0.0, 0.0] and float(got.d.abs().max()) == 0.0
    # smooth = 0; w_dice = 0 (the CE reference within the bound; no bit-equality with the counted kernel is claimed); w_ce = 0
    for kw in (dict(smooth=0.0), dict(smooth=0.0, present_only=False), dict(w_dice=0.0), dict(w_ce=0.0), dict(w_ce=0.0, present_only=False)):
        o = _opts(per_image=per_image, **kw)
        ref = _reference(cs, o)
        got = _all_variants(C, f'{kw}', cs, o, ref, variants=variants)
        if kw.get('w_dice') == 0.0:
            assert float(got.l3[2]) == 0.0
            plain = torch.nn.functional.cross_entropy(cs.zd.double(), torch.where((cs.yd >= 0) & (cs.yd < 5), cs.yd, torch.full_like(cs.yd, cs.ign)),
                                                      ignore_index=cs.ign)
            assert abs(float(got.l3[0]) - float(plain)) < 1e-5 * max(1.0, float(plain))
        if kw.get('w_ce') == 0.0:
            assert float(got.l3[1]) == 0.0


# ------------------------------------------------------------------------------------------------------- the capped grid's second trip
@pytest.mark.parametrize('B,H,W,per_image', [(9, 484, 484, True), (1, 725, 725, False)])
def test_second_trip(C, B, H, W, per_image):
    """The smallest shapes at which the grid rule caps the chunks of an image, so that a workgroup loops, once per pass structure:
    9 x 484 x 484, four pixels per lane: 58,564 quads per image want 229 workgroups, the cap is 2048 // 9 = 227 -- chunks 0 and 1 of every
    image take a second trip, chunk 1 with 196 live lanes; 2043 partial rows.  1 x 725 x 725, one pixel per lane: 525,625 pixels want 2054
    workgroups, the cap is 2048 -- chunks 0 .. 5 loop, chunk 5 with 57 live lanes.  Twice: the same bits.  The four-pixel case also with the
    bf16 copy (the LDS exchange: two barriers inside the strided loop), at pitch 32 and 64."""
    cs = _case(5, B, H, W, 3.0, seed=B)
    o = _opts(per_image=per_image)
    ref = _reference(cs, o)
    what = f'second trip {B}x{H}x{W}'
    got = _abi(C, cs, o)
    _check(what, got, ref)
    assert _same_bits(_abi(C, cs, o), got), what + ': two runs differ'
    if H * W % 4 == 0:
        for v in (NHWC[3], NHWC[4]):
            nh = _abi(C, cs, o, variant=v)
            _check(f'{what} nhwc {v[0]}/{v[2]}', nh, ref)
            _check_nhwc(C, what, nh, v, cs.K)
            assert _same_bits(nh, got), (what, v)


# ----------------------------------------------------------------------------------------------------------------------- the criterion
def test_module_under_autograd(C):
    """DiceCrossEntropyLoss on plain tensors: the reference's loss and gradient, an upstream gradient other than 1, parts and bad_labels."""
    cs = _case(7, 3, 10, 12, 3.0, seed=11)
    for kw in (dict(), dict(ce_weight=0.5, dice_weight=2.0, smooth=1e-3, include_background=False, present_only=False, per_image=True)):
        crit = C.DiceCrossEntropyLoss(**kw)
        o = dict(w_ce=crit.ce_weight, w_dice=crit.dice_weight, smooth=crit.smooth, first_class=0 if crit.include_background else 1,
                 present_only=crit.present_only, per_image=crit.per_image)
        ref = _reference(cs, o)
        plain = None
        for up in (1.0, -2.5):
            z = cs.zd.clone().requires_grad_()
            loss = crit(z, cs.yd)
            (loss * up).backward()
            torch.cuda.synchronize()
            assert abs(float(loss.detach()) - ref.l3[0]) < 1e-5 * max(1.0, abs(ref.l3[0]))
            assert [float(v) for v in crit.parts] == pytest.approx(ref.l3, rel=1e-5, abs=1e-5) and int(crit.bad_labels) == 2
            if plain is None:                   # upstream gradient 1: d logits as the kernel wrote it, under the file's bound
                plain = z.grad.clone()
                ratio = (plain.double() - ref.g).abs() / (EPS * ref.s1[:, None])
                rk = float(ratio[ref.live].max())
                print(f'module {kw}: kernel r {rk:.2f}')
                assert ref.r32 <= RESTATEMENT_MAX and rk <= C_BOUND and float(plain[~ref.live].abs().max()) == 0.0
            else:                               # any other: that tensor times the upstream gradient, one fp32 product per element
                assert torch.equal(z.grad, plain * torch.tensor(up, dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError, match='labels shape'):
        crit(cs.zd, cs.yd[:, :5])


def _net_and_batch(C, seed=9):
    torch.manual_seed(seed)
    m = C.UNet(4, 3, 4, compute_dtype='fp32').to(DEV).train()
    x = torch.from_numpy(C.synth.images(8, 2, 3, 32, 32)).to(DEV)
    y = torch.from_numpy(C.synth.labels(8, 2, 32, 32, 4)).to(DEV)
    y[0, :2] = -100
    return m, x, y


def test_hand_over_to_the_unet(C, monkeypatch):
    """d logits reaches the UNet's backward pass as the NHWC copy the gradient pass wrote (eng.dl_src is set) and, with the hand-over off,
    as the NCHW tensor the engine converts: the same parameter gradients bit for bit in fp32."""
    crit = C.DiceCrossEntropyLoss(per_image=True)

    def run():
        m, x, y = _net_and_batch(C)
        out = m(x)
        eng = next(iter(m._engines.values()))
        loss = crit(out, y)
        taken = eng.dl_src is not None
        loss.backward()
        torch.cuda.synchronize()
        return torch.cat([p.grad.flatten() for p in m.parameters()]).clone(), taken, out.detach().clone(), float(loss)

    ga, taken_a, out, la = run()
    monkeypatch.setattr(C.loss, 'HANDOVER', False)
    gb, taken_b, _, lb = run()
    assert taken_a and not taken_b and la == lb
    assert torch.equal(ga.view(torch.int32), gb.view(torch.int32)) and bool(ga.any())
    _, y = _net_and_batch(C)[1:]
    ref = dice_ref.dice_ce(out.double(), y, per_image=True)[0]
    assert abs(la - float(ref)) < 1e-5 * max(1.0, abs(float(ref)))


def _data(C, nc=4):
    return [(torch.from_numpy(C.synth.images(7, 2, 3, 32, 32, first_image=2 * i)),
             torch.from_numpy(C.synth.labels(7, 2, 32, 32, nc, first_image=2 * i))) for i in range(2)]


def test_trainer_with_ce_dice(C, tmp_path):
    data = _data(C)
    mk = lambda: C.default_config(loss='ce_dice', dice_weight=0.5, dice_include_background=False, conv_dim=4, num_classes=4, n_iters=3, lr=1e-3,
                                  compute_dtype='fp32', stats_every=1)
    torch.manual_seed(5)
    tr = C.Trainer(data, mk())
    assert isinstance(tr.c_loss, C.DiceCrossEntropyLoss) and type(tr.likelihood_loss) is C.CrossEntropyLoss
    kw = dict(w_ce=1.0, w_dice=0.5, smooth=1e-5, first_class=1, present_only=True, per_image=False)
    losses = []
    for _ in range(2):
        for x, y in data:
            out, loss = tr.train_step(x.to(DEV), y.to(DEV))
            ref = float(dice_ref.dice_ce(out.detach().double(), y.to(DEV), **kw)[0])
            assert abs(float(loss) - ref) <= 1e-5 * abs(ref), (float(loss), ref)
            parts = [float(v) for v in tr.c_loss.parts]
            assert parts[1] > 0 and parts[2] > 0 and int(tr.c_loss.bad_labels) == 0
            losses.append(float(loss))
    assert all(math.isfinite(v) for v in losses) and losses[-1] != losses[0]
    # a checkpoint round trip is unaffected: one more step of the uninterrupted run against a fresh Trainer that loaded the file, bit for bit
    tr.save_network('unet', 'e1', 0, str(tmp_path))
    x, y = data[0][0].to(DEV), data[0][1].to(DEV)
    _, la = tr.train_step(x, y)
    tr2 = C.Trainer(data, mk())
    assert tr2.load_network('unet', 'e1', str(tmp_path))
    _, lb = tr2.train_step(x, y)
    assert float(la) == float(lb)
    for (k, a), (_, b) in zip(tr.model.state_dict().items(), tr2.model.state_dict().items()):
        assert torch.equal(a, b), k
    # importance estimation keeps the plain log-likelihood; a task-2 step with POD on top of the criterion runs
    cons = tr.estimate_importance(data, max_batches=1)
    assert cons is not None
    with pytest.raises(ValueError, match='distill_lambda > 0'):
        tr.begin_task2(2)
    tr.begin_task2(2, distill_lambda=0.0, pod_lambda=0.5)
    w0 = torch.cat([p.detach().flatten() for p in tr.model.parameters()]).clone()
    out, loss = tr.train_step(x, y)
    ref = float(dice_ref.dice_ce(out.detach().double(), y, **kw)[0])
    assert math.isfinite(float(loss)) and float(loss) >= ref - 1e-5 * abs(ref)          # the POD term is >= 0 and adds on top
    assert [float(v) for v in tr.c_loss.parts][0] == pytest.approx(ref, rel=1e-5)
    w1 = torch.cat([p.detach().flatten() for p in tr.model.parameters()])
    assert bool(torch.isfinite(w1).all()) and not torch.equal(w0, w1)
