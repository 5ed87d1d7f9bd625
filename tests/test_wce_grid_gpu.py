"""GPU: clamd_ce_class_fwd_bwd (class weights, label smoothing, the focal term; csrc/loss.hip) per element, over the grid its dispatch can
launch, by the method of tests/test_loss_grid_gpu.py.

Every case calls the C ABI directly, d logits and the NHWC copy inside poisoned guard bands, and compares with tests/wce_ref.py in float64:
    |d logits - grad_scale * ref| <= c * 2^-24 * grad_scale * s_px        for every element,
s_px = nu_b / D * ((1 - eps) w_y f + eps W / K) with the floor 2^-40 nu_b w_y / D (a confidently right focal pixel has f in the fp32 denormal
range); a pixel with s_px == 0 (invalid, nu_b == 0, or w_y == 0 without smoothing) is exactly zero.  The loss parts keep
1e-5 * max(1, |ref|), out3[0] == out3[1] + out3[2] as an fp32 sum, both label counters are exact.
How c was obtained: every case also evaluates wce_ref.wce -- the closed form -- in torch float32 and prints `fp32 r` = max |err| /
(2^-24 * s_px) of that restatement beside `kernel r`.  RESTATEMENT_MAX[mode] is the largest `fp32 r` over this file's cases (evaluated on the
CPU; recorded in DESIGN.md), C_BOUND = that times 4, rounded up to a power of two.  Autograd through q^gamma * t in float32 is NOT the
yardstick: it cancels terms gamma * t times larger than the result.

Instantiations ce4c_kernel<KMAX, NPX, NT, MODE> and the cases that reach them (NT = none / fp32 / bf16 / bf16x3, pitch 32 and 64, looped
inside every case marked *):
  <8|16|24|32, 4, NT, MODE>   test_class_boundaries K = 1,8 | 9,16 | 17,24 | 25,32 at 3 x 8 x 12 *, without and with image weights; one wave
                              over several images at 6 x 4 x 4
  <32, 1, NT, MODE>           test_one_pixel_form at 2 x 5 x 7 *; the misaligned views of test_class_boundaries
  second trip of the grid     test_capped_grid: 9 x 484 x 484 (2059 -> 2048 workgroups, + the bf16 exchange) and 1 x 725 x 725 (2054 -> 2048)
  class_count_rows_kernel<4|1>   every case (the counters are exact); <1> by the odd sizes and by a misaligned label view."""
import math
from types import SimpleNamespace

import pytest
import torch

import wce_ref
from test_loss_grid_gpu import BOUNDARY_K, DEV, EPS, NHWC, NU, POISON, _abi, _check_nhwc, _guarded, _guards_intact, _misaligned

pytestmark = pytest.mark.gpu

# mode -> (label_smoothing, focal_gamma)
MODES = {'weights': (0.0, 0.0), 'smoothing': (0.1, 0.0), 'focal': (0.0, 2.0)}
# largest fp32-restatement ratio per mode over this file's cases ('focal': gamma 0.5, 2 and 5) ...
RESTATEMENT_MAX = {'weights': 6.6, 'smoothing': 7.3, 'focal': 22.9}      # focal: 17.3 at gamma 2, 8.5 at 0.5, 22.9 at 5
# ... times 4, rounded up to a power of two
C_BOUND = {k: 2.0 ** math.ceil(math.log2(4.0 * v)) for k, v in RESTATEMENT_MAX.items()}


@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    C._lib.load()
    return C


def _weights(K, seed):
    """K class weights in [0.25, 2.75): some above 1, and one exactly 0 (class K // 2) when there is more than one class."""
    w = 0.25 + 2.5 * torch.rand(K, generator=torch.Generator().manual_seed(1000 + seed))
    if K > 1:
        w[K // 2] = 0.0
    return w


def _case(K, B, H, W, scale, seed=0, ign=-100, dev=DEV):
    """Inputs of one case: ignored pixels, an out-of-range label (K + 2), a negative non-ignore one (-7); weights with a zero; image weights
    that differ, one 0.0, some > 1."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, K, H, W, generator=g) * scale
    y = torch.randint(0, K, (B, H, W), generator=g)
    y[0, 0, :3] = ign; y[0, 1, 0] = K + 2; y[-1, -1, -1] = -7
    return SimpleNamespace(K=K, B=B, H=H, W=W, ign=ign, zd=z.to(dev), yd=y.to(dev), wd=_weights(K, seed).to(dev), nud=torch.tensor(NU[:B]).to(dev))


def _reference(cs, mode, nu=False, gamma=None, w=None):
    eps, g = MODES[mode]
    g = g if gamma is None else gamma
    w = cs.wd if w is None else w
    kw = dict(nu=cs.nud if nu else None, eps=eps, gamma=g, ignore_index=cs.ign)
    r = wce_ref.wce(cs.zd.double(), cs.yd, w.double(), **kw)
    r32 = wce_ref.wce(cs.zd, cs.yd, w, **kw)
    r.live = (r.s_px > 0)[:, None].expand_as(r.grad)
    r.r32 = float(((r32.grad.double() - r.grad).abs() / (EPS * r.s_px[:, None]))[r.live].max()) if bool(r.live.any()) else 0.0
    r.mode, r.eps, r.gamma, r.nu, r.w = mode, eps, g, nu, w
    r.l3 = [float(v) for v in r.l3]
    return r


def _wabi(C, cs, ref, gs=1.0, variant=NHWC[0], z=None, y=None):
    """One call of clamd_ce_class_fwd_bwd with the reference's weights and mode -> loss3, d logits, NHWC copy or None, N_valid, N_bad."""
    lib, ptr, s = C._lib, C._lib.ptr, C._lib.stream_ptr()
    L = lib.load()
    B, K, H, W = cs.B, cs.K, cs.H, cs.W
    z = cs.zd if z is None else z
    y = cs.yd if y is None else y
    wsb = L.clamd_ce_class_workspace_bytes()
    off = L.clamd_ce_bad_label_count_offset() // 4
    ws = torch.full((wsb // 4,), float('nan'), device=DEV)
    dbuf, d = _guarded((B, K, H, W), torch.float32, fill=float('nan'))
    l3 = torch.full((3,), float('nan'), device=DEV)
    name, dcode, ldc = variant
    nbuf = nh = None
    if name is not None:
        nbuf, nh = _guarded((B, H, W, ldc), C.ops.TORCH_DT[dcode])
    lib.call('clamd_ce_class_fwd_bwd', ptr(z), ptr(y), ptr(ref.w), ptr(cs.nud if ref.nu else None), ptr(d), ptr(nh), ldc, dcode, ptr(l3),
             ptr(ws), wsb, B, K, H, W, cs.ign, float(ref.eps), float(ref.gamma), float(gs), s)
    torch.cuda.synchronize()
    assert _guards_intact(dbuf, d), 'a store outside d logits'
    if nh is not None:
        assert _guards_intact(nbuf, nh), 'a store outside the NHWC copy'
    counts = ws[off - 1:off + 1].view(torch.int32).tolist()
    return SimpleNamespace(l3=l3, d=d, nh=nh, nvalid=counts[0], nbad=counts[1])


def _check(what, got, ref, gs=1.0):
    c = C_BOUND[ref.mode]
    assert (got.nvalid, got.nbad) == (ref.nvalid, ref.nbad), (what, got.nvalid, got.nbad, ref.nvalid, ref.nbad)
    errs = [abs(float(a) - b) / max(1.0, abs(b)) for a, b in zip(got.l3, ref.l3)]
    assert bool(torch.isfinite(got.d).all()), what
    nz = int((got.d[~ref.live] != 0).sum())
    ratio = (got.d.double() - gs * ref.grad).abs() / (EPS * gs * ref.s_px[:, None])
    rk = float(ratio[ref.live].max()) if bool(ref.live.any()) else 0.0
    print(f'{what}: fp32 r {ref.r32:.2f}, kernel r {rk:.2f} (c {c:g}), loss rel errors {["%.1e" % e for e in errs]}')
    assert rk <= c, (what, rk, c, ref.r32)
    assert nz == 0, f'{what}: {nz} non-zero elements on pixels without a gradient'
    assert max(errs) < 1e-5, (what, errs)
    assert torch.equal(got.l3[0], got.l3[1] + got.l3[2]), (what, got.l3.tolist())
    if ref.eps == 0.0:
        assert float(got.l3[2]) == 0.0, what


def _same_bits(a, b):
    return torch.equal(a.d.view(torch.int32), b.d.view(torch.int32)) and torch.equal(a.l3.view(torch.int32), b.l3.view(torch.int32))


def _all_variants(C, what, cs, ref, gs=1.0, variants=NHWC):
    """Without and with every NHWC copy: each call against the reference, the copies against the converted gradient, d logits / loss the
    same bits whatever the copy.  -> the call without a copy."""
    first = None
    for v in variants:
        got = _wabi(C, cs, ref, gs, v)
        _check(f'{what} nhwc {v[0]}/{v[2]}', got, ref, gs)
        if v[0] is not None:
            _check_nhwc(C, what, got, v, cs.K)
        if first is None:
            first = got
        else:
            assert _same_bits(got, first), (what, v)
    return first


# ------------------------------------------------------------------------------------------- class-count boundaries, four pixels per thread
@pytest.mark.parametrize('scale', [3.0, 30.0])
@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('K', BOUNDARY_K)
def test_class_boundaries(C, K, mode, scale):
    """3 x 8 x 12 = 72 quads (one workgroup, 184 dead lanes), without and with image weights; a misaligned view takes the one-pixel kernel:
    the same arithmetic per pixel; one wave over several images at 6 x 4 x 4."""
    cs = _case(K, 3, 8, 12, scale, seed=K)
    for nu in (False, True):
        ref = _reference(cs, mode, nu)
        assert ref.nbad == 2
        what = f'{mode} K{K} x{scale} nu{int(nu)}'
        got = _all_variants(C, what, cs, ref)
        zs = _misaligned(cs.zd)
        for v in (NHWC[0], NHWC[3]):
            mis = _wabi(C, cs, ref, variant=v, z=zs)
            _check(f'{what} misaligned nhwc {v[0]}', mis, ref)
            assert torch.equal(mis.d.view(torch.int32), got.d.view(torch.int32)), what
            if v[0] is not None:
                _check_nhwc(C, what + ' misaligned', mis, v, K)
    cs6 = _case(K, 6, 4, 4, scale, seed=K + 100)
    _all_variants(C, f'{mode} K{K} x{scale} 6x4x4', cs6, _reference(cs6, mode, True), variants=(NHWC[0], NHWC[3], NHWC[6]))


# --------------------------------------------------------------------------------------------------------------- one pixel per thread
@pytest.mark.parametrize('scale', [3.0, 30.0])
@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('K', [8, 17, 32])
def test_one_pixel_form(C, K, mode, scale):
    """H * W % 4 != 0 (2 x 5 x 7): ce4c_kernel<32, 1, NT, MODE> and the one-label count."""
    cs = _case(K, 2, 5, 7, scale, seed=K)
    for nu in (False, True):
        _all_variants(C, f'{mode} 5x7 K{K} x{scale} nu{int(nu)}', cs, _reference(cs, mode, nu))


@pytest.mark.parametrize('scale', [3.0, 30.0])
@pytest.mark.parametrize('gamma', [0.5, 5.0])
def test_focal_exponents(C, gamma, scale):
    for B, H, W in ((3, 8, 12), (2, 5, 7)):
        cs = _case(21, B, H, W, scale, seed=int(gamma * 2))
        _all_variants(C, f'focal gamma {gamma} x{scale} {H}x{W}', cs, _reference(cs, 'focal', True, gamma=gamma), variants=(NHWC[0], NHWC[3]))


# ------------------------------------------------------------------------------------------------------------------------ arguments
@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('ign', [-100, 255])
def test_ignore_index(C, ign, mode):
    for B, H, W in ((3, 8, 12), (2, 5, 7)):
        cs = _case(21, B, H, W, 3.0, seed=ign % 7, ign=ign)
        ref = _reference(cs, mode, True)
        assert int((cs.yd == ign).sum()) >= 3 and ref.nbad == 2
        _all_variants(C, f'{mode} ign {ign} {H}x{W}', cs, ref, variants=(NHWC[0], NHWC[3]))
    # a misaligned label view alone: the one-label count and the one-pixel kernel, the same gradient
    cs = _case(21, 3, 8, 12, 3.0, seed=3, ign=ign)
    ref = _reference(cs, mode, False)
    ys = torch.zeros(cs.yd.numel() + 8, dtype=torch.int64, device=DEV)[1:1 + cs.yd.numel()].view(cs.yd.shape)
    ys.copy_(cs.yd)
    assert ys.data_ptr() % 32 == 8
    a, b = _wabi(C, cs, ref), _wabi(C, cs, ref, y=ys)
    _check(f'{mode} misaligned labels', b, ref)
    assert torch.equal(a.d.view(torch.int32), b.d.view(torch.int32))


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('gs', [0.375, 3.0])
def test_grad_scale_at_the_abi(C, gs, mode):
    """d logits against grad_scale x the reference under the same per-element bound; the loss values do not move."""
    for B, H, W in ((3, 8, 12), (2, 5, 7)):
        cs = _case(21, B, H, W, 3.0, seed=4)
        ref = _reference(cs, mode, True)
        got = _all_variants(C, f'{mode} {H}x{W} grad_scale {gs}', cs, ref, gs=gs, variants=(NHWC[0], NHWC[3], NHWC[5]))
        assert torch.equal(got.l3, _wabi(C, cs, ref).l3)


# ------------------------------------------------------------------------------------------------------- the capped grid's second trip
@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('B,H,W', [(9, 484, 484), (1, 725, 725)])
def test_capped_grid(C, B, H, W, mode):
    """More work items than 2048 workgroups x 256 lanes: 9 x 484 x 484 = 527,076 quads (2059 workgroups wanted); 725 x 725 = 525,625 pixels
    (2054 wanted).  Twice: the same bits.  The four-pixel case also with the bf16 copy (the LDS exchange, barriers inside the strided loop)."""
    cs = _case(5, B, H, W, 3.0, seed=B)
    ref = _reference(cs, mode, True)
    what = f'capped {mode} {B}x{H}x{W}'
    got = _wabi(C, cs, ref)
    _check(what, got, ref)
    assert _same_bits(_wabi(C, cs, ref), got), what + ': two runs differ'
    if H * W % 4 == 0:
        for v in (NHWC[3], NHWC[4]):
            nh = _wabi(C, cs, ref, variant=v)
            _check(f'{what} nhwc {v[0]}/{v[2]}', nh, ref)
            _check_nhwc(C, what, nh, v, cs.K)
            assert _same_bits(nh, got), (what, v)
            again = _wabi(C, cs, ref, variant=v)
            assert _same_bits(again, nh) and torch.equal(again.nh.view(torch.int16), nh.nh.view(torch.int16)), (what, v, 'two runs differ')


# ------------------------------------------------------------------------------------------------------------------- D == 0
@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('B,H,W', [(3, 8, 12), (2, 5, 7)])
def test_zero_denominator(C, B, H, W, mode):
    """Nothing valid, and every valid pixel on a class of weight 0 (with smoothing those pixels would have a term, over D == 0): the loss
    parts and every gradient exactly zero, the NHWC copy too."""
    cs = _case(5, B, H, W, 3.0, seed=2)
    ignored = SimpleNamespace(**{**vars(cs), 'yd': torch.full_like(cs.yd, cs.ign)})
    w0 = torch.zeros(5, device=DEV); w0[4] = 2.0
    zero_class = SimpleNamespace(**{**vars(cs), 'yd': cs.yd.clamp(max=3)})
    for what, c, w in (('all ignored', ignored, cs.wd), ('zero-weight classes', zero_class, w0)):
        ref = _reference(c, mode, True, w=w)
        assert float(ref.D) == 0.0 and ref.l3 == [0.0, 0.0, 0.0]
        for v in (NHWC[0], NHWC[1], NHWC[3]):
            got = _wabi(C, c, ref, variant=v)
            assert (got.nvalid, got.nbad) == (ref.nvalid, ref.nbad)
            assert got.l3.tolist() == [0.0, 0.0, 0.0] and int((got.d != 0).sum()) == 0, (what, mode, v)
            if got.nh is not None:
                assert int((got.nh[..., :32].float() != 0).sum()) == 0 and bool((got.nh[..., 32:] == POISON).all())


# ------------------------------------------------------------------------------------------- bit equality with the existing kernels
def _plain_case(cs, nu):
    """The same inputs in the shape tests/test_loss_grid_gpu.py's _abi reads."""
    return SimpleNamespace(K=cs.K, c_old=1, B=cs.B, H=cs.H, W=cs.W, lam=0.0, T=2.0, ign=cs.ign, zd=cs.zd, zod=None, yd=cs.yd, nud=nu)


@pytest.mark.parametrize('K', BOUNDARY_K)
def test_unit_weights_are_the_plain_kernels_bit_for_bit(C, K):
    """Every w_k == 1.0f, eps = gamma = 0: d logits, every NHWC copy and the three loss words of clamd_ce_count + clamd_ce_fwd_bwd_counted
    without image weights and of clamd_ce_fwd_bwd_weighted with them; the one-pixel forms of the two weighted entry points as well."""
    ones = torch.ones(K, device=DEV)
    for B, H, W, gs in ((3, 8, 12, 1.0), (3, 40, 52, 0.375), (2, 5, 7, 3.0)):
        cs = _case(K, B, H, W, 3.0, seed=K + H)
        for nu in (False, True):
            if not nu and H * W % 4:
                continue                                                  # clamd_ce_fwd_bwd_counted has no one-pixel form
            ref = _reference(cs, 'weights', nu, w=ones)
            for v in NHWC:
                new = _wabi(C, cs, ref, gs, v)
                old = _abi(C, 'weighted' if nu else 'counted', _plain_case(cs, cs.nud), gs, v)
                assert _same_bits(new, old), (K, H, nu, v, new.l3.tolist(), old.l3.tolist())
                assert (new.nvalid, new.nbad) == (old.nvalid, old.nbad)
                if v[0] is not None:
                    wd = torch.int16 if v[1] == 1 else torch.int32
                    assert torch.equal(new.nh.view(wd), old.nh.view(wd)), (K, H, nu, v)


def test_unit_weights_on_the_capped_grid(C):
    cs = _case(5, 9, 484, 484, 3.0, seed=9)
    ones = torch.ones(5, device=DEV)
    for nu in (False, True):
        ref = _reference(cs, 'weights', nu, w=ones)
        for v in (NHWC[0], NHWC[3]):
            assert _same_bits(_wabi(C, cs, ref, variant=v), _abi(C, 'weighted' if nu else 'counted', _plain_case(cs, cs.nud), 1.0, v)), (nu, v)


# ------------------------------------------------------------------------------------------------------------------------ errors
def test_error_returns(C):
    cs = _case(5, 2, 8, 12, 3.0)
    ref = _reference(cs, 'weights')
    for kw, needle in ((dict(eps=1.0), 'label_smoothing'), (dict(eps=-0.1), 'label_smoothing'), (dict(gamma=-1.0), 'focal_gamma'),
                       (dict(gamma=float('inf')), 'focal_gamma'), (dict(eps=0.1, gamma=2.0), 'both non-zero'),
                       (dict(w=None), 'class_weight')):
        r = SimpleNamespace(**{**vars(ref), **kw})
        with pytest.raises(RuntimeError, match=needle):
            _wabi(C, cs, r)
    K33 = SimpleNamespace(**{**vars(cs), 'K': 33})
    with pytest.raises(RuntimeError, match='classes'):
        _wabi(C, K33, ref)
