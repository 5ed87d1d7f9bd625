"""GPU: the per-pixel loss kernels of csrc/loss.hip, per element, over the grid their dispatch can launch.

Every case calls the C ABI directly and compares with a float64 evaluation of include/clamd.h's formulas on the same inputs (torch
autograd through weighted_ce / unbiased_losses / cross-entropy + temperature KL; never another call into libclamd.so):
    |d logits - grad_scale * ref| <= c * 2^-24 * s_px        for every element,
s_px the pixel's gradient scale (the sum of the coefficients that multiply a probability difference: grad_scale * nu_b / max(N, 1) on a
valid pixel, plus grad_scale * lam / (T * B*H*W) for clamd_ce_fwd_bwd's distillation term, plus grad_scale * lam / (c_old * B*H*W) for the
unbiased one); a pixel with s_px == 0 is exactly zero.  The loss parts keep 1e-5 * max(1, |ref|), out3[0] == out3[1] + out3[2] as an fp32
sum, both label counters exact.
How c was obtained: every case also evaluates the SAME formulas in torch float32 (_restatement: autograd through log_softmax on float32
tensors; for the unbiased pair the header's closed-form gradients from torch.softmax over each group -- every softmax relative to its own
maximum) and prints `fp32 r` = max |err| / (2^-24 * s_px) of that restatement beside `kernel r`; C_BOUND[entry point] is the largest `fp32 r` over this file's cases (RESTATEMENT_MAX, recorded in DESIGN.md) times 4 -- expf /
logf a few ulp off torch's, the kernel's sequential sum -- rounded up to a power of two.  A kernel above the bound is a finding in loss.hip.

Instantiations (KMAX, KOLD, NPX, NT) and the cases that reach them, each against the reference (NT = none / fp32 / bf16 / bf16x3 is looped
inside every case marked *, pitch 32 and 64):
  ce4_kernel<8|16|24|32, 4, NT, false>       test_plain_class_boundaries K = 1,8 | 9,16 | 17,24 | 25,32 *            (clamd_ce_fwd_bwd_counted)
  ce4_kernel<8|16|24|32, 4, NT, true>        the same test, clamd_ce_fwd_bwd_weighted *; one wave over several images: B = 6, 4x4
  ce4_kernel<32, 1, NT, true>                test_one_pixel_form K = 8, 17, 32 *; the misaligned views of test_plain_class_boundaries
  ce4u_kernel<KMAX, 0, 4, NT>                test_unbiased_class_boundaries, lam = 0: (8,8) (16,16) (24,9) (32,32) ... *
  ce4u_kernel<KMAX, 16, 4, NT>               ... with distillation: (8,8) | (9,1) (16,16) | (17,16) (24,9) | (32,1) *
  ce4u_kernel<24|32, 32, 4, NT>              ... (21,17) | (25,17) (32,32) *
  ce4u_kernel<32, 0|32, 1, NT>               test_one_pixel_form *, the misaligned views of test_unbiased_class_boundaries, the rebase case
  ce_kernel<32>                              test_temperature_distillation (K = 9, 17, 32; c_old = 1, K // 2, K); misaligned plain calls
  second trip of the capped grid             test_capped_grid: ce4 (plain, weighted), ce4u at 9 x 484 x 484 (2059 -> 2048 workgroups, + the
                                             bf16 exchange path); ce_kernel, ce4<32,1>, ce4u<32,32,1> at 1 x 725 x 725 (2054 -> 2048)."""
import copy
import math
from types import SimpleNamespace

import pytest
import torch

from test_incremental_cpu import unbiased_losses
from test_pseudo_label_cpu import weighted_ce

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
EPS = 2.0 ** -24
# largest fp32-restatement ratio per entry point over this file's cases (torch float32 against float64; every case prints its own) ...
RESTATEMENT_MAX = {'counted': 8.4, 'weighted': 8.0, 'unbiased': 8.8, 'ce': 5.8}
# ... times 4, rounded up to a power of two
C_BOUND = {k: 2.0 ** math.ceil(math.log2(4.0 * v)) for k, v in RESTATEMENT_MAX.items()}
POISON = 7.5                                                          # exact in bf16 too
GUARD = 64                                                            # elements: 256 bytes of fp32, 128 of bf16
NU = [1.75, 0.0, 0.4, 1.0, 2.5, 0.7, 1.25, 0.05, 0.9]                 # per-image weights: they differ, one 0.0, some > 1
NHWC = [(None, 0, 0)] + [(n, d, p) for n, d in (('fp32', 0), ('bf16', 1), ('bf16x3', 2)) for p in (32, 64)]      # (name, dtype code, pitch)
BOUNDARY_K = [1, 8, 9, 16, 17, 24, 25, 32]
BOUNDARY_UNBIASED = [(8, 8), (9, 1), (16, 16), (17, 16), (21, 17), (24, 9), (25, 17), (32, 32), (32, 1)]


@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    C._lib.load()
    return C


# ------------------------------------------------------------------------------------------------------------------------------ inputs
def _case(K, c_old, B, H, W, scale, seed=0, ign=-100, lam=10.0, T=2.0):
    """The inputs of one case, on the host and on the device: ignored pixels, an out-of-range label (K + 2), a negative non-ignore one (-7)."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, K, H, W, generator=g) * scale
    zo = torch.randn(B, c_old + (1 if c_old < K else 0), H, W, generator=g) * scale
    y = torch.randint(0, K, (B, H, W), generator=g)
    y[0, 0, :3] = ign; y[0, 1, 0] = K + 2; y[-1, -1, -1] = -7
    nu = torch.tensor(NU[:B])
    cs = SimpleNamespace(K=K, c_old=c_old, B=B, H=H, W=W, lam=lam, T=T, ign=ign, z=z, zo=zo, y=y, nu=nu)
    return _to_device(cs)


def _to_device(cs):
    cs.zd, cs.zod, cs.yd, cs.nud = cs.z.to(DEV), cs.zo.to(DEV), cs.y.to(DEV), cs.nu.to(DEV)
    return cs


def _with(cs, **kw):
    c2 = copy.copy(cs)
    for k, v in kw.items():
        setattr(c2, k, v)
    return c2


def _has_kd(entry, cs):
    return entry in ('unbiased', 'ce') and cs.lam > 0


# --------------------------------------------------------------------------------------------------------------------------- reference
def _evaluate(entry, cs, dtype):
    """{total, ce, kd} and d total / d logits of include/clamd.h's formulas in `dtype`, on the device.  float64: the reference.  float32: the
    restatement c is derived from -- the same functions, the logits taken relative to the pixel's maximum first."""
    zz = cs.zd.to(dtype, copy=True).requires_grad_()
    zin = zz if dtype == torch.float64 else zz - zz.amax(1, keepdim=True).detach()
    zo = cs.zod.to(dtype)
    if entry == 'unbiased':
        tot, ce, kd = unbiased_losses(zin, cs.yd, zo if cs.lam > 0 else None, cs.c_old, cs.lam, cs.ign)
    else:
        nu = cs.nud if entry == 'weighted' else torch.ones(cs.B, device=DEV)
        ce = weighted_ce(zin, cs.yd, nu, cs.ign)
        kd = ce.new_zeros(())
        if _has_kd(entry, cs):
            lp = torch.log_softmax(zo[:, :cs.c_old] / cs.T, 1)
            lq = torch.log_softmax(zin[:, :cs.c_old] / cs.T, 1)
            kd = cs.lam * (lp.exp() * (lp - lq)).sum(1).mean()
        tot = ce + kd
    g, = torch.autograd.grad(tot, zz)
    return [float(tot.detach()), float(ce.detach()), float(kd.detach())], g


def _restatement(entry, cs):
    """d logits of the same formulas in float32, every softmax relative to its own maximum (what a plain fp32 evaluation can reach).  The
    plain, weighted and temperature-distilled losses: autograd through log_softmax.  The unbiased pair: the closed forms of include/clamd.h,
    softmax_all - [y < c_old] softmax_old - [y >= c_old] onehot and softmax_all - q_0 softmax_bgnew - q_k, from torch.softmax over each
    group (autograd through logsumexp differences would take exp(z - LSE(group)) with the LSE rounded at its own magnitude)."""
    if entry != 'unbiased':
        return _evaluate(entry, cs, torch.float32)[1]
    z, y, K, c = cs.zd, cs.yd, cs.K, cs.c_old
    valid = (y != cs.ign) & (y >= 0) & (y < K)
    yc = y.clamp(0, K - 1)
    sm = torch.softmax(z, 1)
    sub = torch.nn.functional.one_hot(yc, K).permute(0, 3, 1, 2).float()
    old = torch.zeros_like(z)
    old[:, :c] = torch.softmax(z[:, :c], 1)
    g = (sm - torch.where((yc < c)[:, None], old, sub)) * (valid[:, None] / max(int(valid.sum()), 1))
    if _has_kd(entry, cs):
        q = torch.softmax(cs.zod[:, :c], 1)
        t = torch.zeros_like(z)
        bg = [0] + list(range(c, K))
        t[:, bg] = q[:, :1] * torch.softmax(z[:, bg], 1)
        t[:, 1:c] = q[:, 1:]
        g = g + (sm - t) * (cs.lam / (c * cs.B * cs.H * cs.W))
    return g


def _pixel_scale(entry, cs, gs):
    """s_px [B,H,W] in float64, and the two label counters."""
    y = cs.yd
    inr = (y >= 0) & (y < cs.K)
    valid = (y != cs.ign) & inr
    nvalid, nbad = int(valid.sum()), int(((y != cs.ign) & ~inr).sum())
    nu = cs.nud.double() if entry == 'weighted' else torch.ones(cs.B, dtype=torch.float64, device=DEV)
    s = gs * nu[:, None, None] * valid / max(nvalid, 1)
    if _has_kd(entry, cs):
        s = s + gs * cs.lam / ((cs.T if entry == 'ce' else cs.c_old) * cs.B * cs.H * cs.W)
    return s, nvalid, nbad


def _reference(entry, cs):
    ref3, g64 = _evaluate(entry, cs, torch.float64)
    g32 = _restatement(entry, cs)
    s1, nvalid, nbad = _pixel_scale(entry, cs, 1.0)
    live = (s1 > 0)[:, None].expand_as(g64)
    r32 = float(((g32.double() - g64).abs() / (EPS * s1[:, None]))[live].max()) if bool(live.any()) else 0.0
    return SimpleNamespace(entry=entry, l3=ref3, g=g64, s1=s1, live=live, nvalid=nvalid, nbad=nbad, r32=r32,
                           zero_grad=entry == 'unbiased' and cs.c_old == cs.K and not _has_kd(entry, cs))


# ----------------------------------------------------------------------------------------------------------------------------- the ABI
def _guarded(shape, dtype, fill=None, shift=0):
    """A tensor of `shape` as an interior slice of a larger poisoned buffer (16-byte alignment kept unless `shift` elements are asked for)."""
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD + shift,), POISON, dtype=dtype, device=DEV)
    view = buf[GUARD + shift:GUARD + shift + n].view(shape)
    assert view.data_ptr() % 64 == (shift * buf.element_size()) % 64
    if fill is not None:
        view.fill_(fill)
    return buf, view


def _guards_intact(buf, view):
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool((buf[:lo] == POISON).all()) and bool((buf[lo + view.numel():] == POISON).all())


def _misaligned(t):
    """A copy of t that starts 4 bytes past a 16-byte boundary."""
    _, v = _guarded(tuple(t.shape), t.dtype, shift=1)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _abi(C, entry, cs, gs=1.0, variant=NHWC[0], z=None):
    """One call of the entry point (after clamd_ce_count where it needs one) -> loss3, d logits, NHWC copy or None, N_valid, N_bad.
    d logits and the copy live inside poisoned buffers whose guard bands are checked here."""
    lib, ptr, s = C._lib, C._lib.ptr, C._lib.stream_ptr()
    L = lib.load()
    B, K, H, W = cs.B, cs.K, cs.H, cs.W
    z = cs.zd if z is None else z
    wsb = L.clamd_ce_workspace_bytes()
    off = L.clamd_ce_bad_label_count_offset() // 4                     # the totals pair {valid, bad}: the bad-label counter is its second word
    ws = torch.full((wsb // 4,), float('nan'), device=DEV)
    dbuf, d = _guarded((B, K, H, W), torch.float32, fill=float('nan'))
    l3 = torch.full((3,), float('nan'), device=DEV)
    name, dcode, ldc = variant
    nbuf = nh = None
    if name is not None:
        nbuf, nh = _guarded((B, H, W, ldc), C.ops.TORCH_DT[dcode])
    zo = cs.zod if _has_kd(entry, cs) else None
    kt = 0 if zo is None else zo.shape[1]
    if entry == 'ce':
        assert nh is None
        lib.call('clamd_ce_fwd_bwd', ptr(z), ptr(cs.yd), ptr(zo), kt, cs.c_old, float(cs.T), float(cs.lam if zo is not None else 0.0), ptr(d), ptr(l3),
                 ptr(ws), wsb, B, K, H, W, cs.ign, float(gs), s)
    else:
        lib.call('clamd_ce_count', ptr(cs.yd), B, K, H, W, cs.ign, ptr(ws), wsb, s)
        tail = (ptr(d), ptr(nh), ldc, dcode, ptr(l3), ptr(ws), wsb, B, K, H, W, cs.ign, float(gs), s)
        if entry == 'counted':
            lib.call('clamd_ce_fwd_bwd_counted', ptr(z), ptr(cs.yd), *tail)
        elif entry == 'weighted':
            lib.call('clamd_ce_fwd_bwd_weighted', ptr(z), ptr(cs.yd), ptr(cs.nud), *tail)
        else:
            lib.call('clamd_ce_unbiased_fwd_bwd', ptr(z), ptr(cs.yd), ptr(zo), kt, cs.c_old, float(cs.lam), *tail)
    torch.cuda.synchronize()
    assert _guards_intact(dbuf, d), f'{entry}: a store outside d logits'
    if nh is not None:
        assert _guards_intact(nbuf, nh), f'{entry}: a store outside the NHWC copy'
    counts = ws[off - 1:off + 1].view(torch.int32).tolist()
    return SimpleNamespace(l3=l3, d=d, nh=nh, nvalid=counts[0], nbad=counts[1])


def _check(what, got, ref, gs=1.0, bound=None):
    """The per-element bound, the exact zeros, the loss parts, their fp32 sum, the counters."""
    c = C_BOUND[ref.entry] if bound is None else bound
    assert (got.nvalid, got.nbad) == (ref.nvalid, ref.nbad), (what, got.nvalid, got.nbad, ref.nvalid, ref.nbad)
    errs = [abs(float(a) - b) / max(1.0, abs(b)) for a, b in zip(got.l3, ref.l3)]
    assert bool(torch.isfinite(got.d).all()), what
    dead = got.d[~ref.live]
    nz = int((dead != 0).sum())
    if ref.zero_grad:
        # no new classes and no distillation: the reference gradient is exactly zero, the kernel subtracts two fp32 roundings of one number
        m, lim = float(got.d.abs().max()), 8 * EPS * gs / max(ref.nvalid, 1)
        print(f'{what}: zero reference gradient, max |d logits| {m:.3e} (bound {lim:.3e}), loss rel errors {errs}')
        assert m <= lim, (what, m, lim)
    else:
        ratio = (got.d.double() - gs * ref.g).abs() / (EPS * gs * ref.s1[:, None])
        rk = float(ratio[ref.live].max()) if bool(ref.live.any()) else 0.0
        print(f'{what}: fp32 r {ref.r32:.2f}, kernel r {rk:.2f} (c {c:g}), loss rel errors {["%.1e" % e for e in errs]}')
        assert rk <= c, (what, rk, c, ref.r32)
    assert nz == 0, f'{what}: {nz} non-zero elements on pixels without a gradient'
    assert max(errs) < 1e-5, (what, errs)
    assert torch.equal(got.l3[0], got.l3[1] + got.l3[2]), (what, got.l3.tolist())


def _check_nhwc(C, what, got, variant, K):
    """The copy is the converted NCHW gradient bit for bit, channels K .. 31 zero, channels >= 32 of a wider pitch untouched."""
    name, dcode, ldc = variant
    conv = C.ops.to_nhwc(got.d, dcode, cp=32)
    w = torch.int16 if dcode == 1 else torch.int32
    nbad = int((conv.view(w) != got.nh[..., :32].contiguous().view(w)).sum())
    assert nbad == 0, (what, name, ldc, nbad)
    vals = C.ops.split_decode(got.nh[..., :32].contiguous()) if dcode == 2 else got.nh[..., :32].float()
    assert float(vals[..., K:].abs().max() if K < 32 else 0.0) == 0.0, (what, name, 'channels K .. 31')
    assert bool((got.nh[..., 32:] == POISON).all()), (what, name, 'channels >= 32 of the pitch')


def _same_bits(a, b):
    return torch.equal(a.d.view(torch.int32), b.d.view(torch.int32)) and torch.equal(a.l3.view(torch.int32), b.l3.view(torch.int32))


def _all_variants(C, what, entry, cs, ref, gs=1.0, variants=NHWC):
    """The entry point without and with every NHWC copy: each call against the reference, the copies against the converted gradient, and
    d logits / loss the same bits whatever the copy.  -> the call without a copy."""
    first = None
    for v in variants:
        got = _abi(C, entry, cs, gs, v)
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
@pytest.mark.parametrize('K', BOUNDARY_K)
def test_plain_class_boundaries(C, K, scale):
    """clamd_ce_fwd_bwd_counted / _weighted at 3 x 40 x 52 (1560 quads: 7 workgroups, the last with 24 live lanes), and the relations that
    hold by construction."""
    cs = _case(K, 1, 3, 40, 52, scale, seed=K)
    refc, refw = _reference('counted', cs), _reference('weighted', cs)
    counted = _all_variants(C, f'counted K{K} x{scale}', 'counted', cs, refc)
    weighted = _all_variants(C, f'weighted K{K} x{scale}', 'weighted', cs, refw)
    assert refw.nbad == 2 and float(weighted.l3[2]) == 0.0
    # unit weights; c_old == 1 without distillation; the all-in-one entry point on aligned tensors: the counted loss bit for bit
    assert _same_bits(_abi(C, 'weighted', _to_device(_with(cs, nu=torch.ones(3)))), counted)
    assert _same_bits(_abi(C, 'unbiased', _with(cs, c_old=1, lam=0.0)), counted)
    assert _same_bits(_abi(C, 'ce', _with(cs, lam=0.0)), counted)
    # a misaligned view: the one-pixel variants.  Weighted: the same arithmetic per pixel (d logits bit-equal, the loss over another grid)
    zs = _misaligned(cs.zd)
    for v in (NHWC[0], NHWC[3]):
        got = _abi(C, 'weighted', cs, variant=v, z=zs)
        _check(f'weighted K{K} x{scale} misaligned nhwc {v[0]}', got, refw)
        assert torch.equal(got.d.view(torch.int32), weighted.d.view(torch.int32))
        if v[0] is not None:
            _check_nhwc(C, 'weighted misaligned', got, v, K)
    _check(f'ce K{K} x{scale} misaligned (ce_kernel)', _abi(C, 'ce', _with(cs, lam=0.0), z=zs), _reference('ce', _with(cs, lam=0.0)))
    # one wave over several images
    cs6 = _case(K, 1, 6, 4, 4, scale, seed=K + 100)
    _all_variants(C, f'weighted K{K} x{scale} 6x4x4', 'weighted', cs6, _reference('weighted', cs6), variants=(NHWC[0], NHWC[3], NHWC[6]))


@pytest.mark.parametrize('scale', [3.0, 30.0])
@pytest.mark.parametrize('kd', [False, True])
@pytest.mark.parametrize('K,c_old', BOUNDARY_UNBIASED)
def test_unbiased_class_boundaries(C, K, c_old, kd, scale):
    cs = _case(K, c_old, 3, 40, 52, scale, seed=K + c_old, lam=10.0 if kd else 0.0)
    ref = _reference('unbiased', cs)
    what = f'unbiased K{K} c{c_old} kd{int(kd)} x{scale}'
    got = _all_variants(C, what, 'unbiased', cs, ref)
    assert ref.nbad == 2 and (kd or float(got.l3[2]) == 0.0)
    zs = _misaligned(cs.zd)
    for v in (NHWC[0], NHWC[4]):
        mis = _abi(C, 'unbiased', cs, variant=v, z=zs)
        _check(f'{what} misaligned nhwc {v[0]}', mis, ref)
        assert torch.equal(mis.d.view(torch.int32), got.d.view(torch.int32)), what
        if v[0] is not None:
            _check_nhwc(C, what + ' misaligned', mis, v, K)


@pytest.mark.parametrize('scale', [3.0, 30.0])
@pytest.mark.parametrize('K,c_old', [(K, c) for K in (9, 17, 32) for c in (1, K // 2, K)])
def test_temperature_distillation(C, K, c_old, scale):
    """clamd_ce_fwd_bwd with old logits: ce_kernel, one pixel per thread, at 3 x 9 x 31 (837 pixels: 4 workgroups, the last with 69)."""
    cs = _case(K, c_old, 3, 9, 31, scale, seed=K + c_old, lam=0.7, T=2.0)
    _check(f'ce+kd K{K} c{c_old} x{scale}', _abi(C, 'ce', cs), _reference('ce', cs))


# --------------------------------------------------------------------------------------------------------------- one pixel per thread
@pytest.mark.parametrize('scale', [3.0, 30.0])
@pytest.mark.parametrize('K', [8, 17, 32])
def test_one_pixel_form(C, K, scale):
    """H * W % 4 != 0 (2 x 7 x 9): ce4_kernel<32, 1, NT, true>, ce4u_kernel<32, 0 | 32, 1, NT>, and ce_kernel for the plain loss."""
    c_old = K // 2
    cs = _case(K, c_old, 2, 7, 9, scale, seed=K)
    _all_variants(C, f'weighted 7x9 K{K} x{scale}', 'weighted', cs, _reference('weighted', cs))
    _all_variants(C, f'unbiased+kd 7x9 K{K} c{c_old} x{scale}', 'unbiased', cs, _reference('unbiased', cs))
    cs0 = _with(cs, lam=0.0)
    _all_variants(C, f'unbiased 7x9 K{K} c{c_old} x{scale}', 'unbiased', cs0, _reference('unbiased', cs0))
    _check(f'ce 7x9 K{K} x{scale}', _abi(C, 'ce', cs0), _reference('ce', cs0))
    with pytest.raises(RuntimeError, match='clamd_ce_fwd_bwd'):          # the counted entry point has no one-pixel form and says so
        _abi(C, 'counted', cs)


# ------------------------------------------------------------------------------------------------------- the capped grid's second trip
@pytest.mark.parametrize('entry,B,H,W', [('counted', 9, 484, 484), ('weighted', 9, 484, 484), ('unbiased', 9, 484, 484),
                                         ('ce', 1, 725, 725), ('weighted', 1, 725, 725), ('unbiased', 1, 725, 725)])
def test_capped_grid(C, entry, B, H, W):
    """More work items than 2048 workgroups x 256 lanes: 9 x 484 x 484 = 527,076 quads (2059 workgroups wanted: 0 .. 10 take a second trip,
    workgroup 10 with 228 live lanes); 725 x 725 = 525,625 pixels (2054 wanted).  Twice: the same bits.  The four-pixel cases also with the
    bf16 copy (the LDS exchange, two barriers inside the strided loop), at pitch 32 and 64."""
    cs = _case(5, 3, B, H, W, 3.0, seed=B, lam=10.0 if entry == 'unbiased' else 0.7)
    ref = _reference(entry, cs)
    what = f'capped {entry} {B}x{H}x{W}'
    got = _abi(C, entry, cs)
    _check(what, got, ref)
    assert _same_bits(_abi(C, entry, cs), got), what + ': two runs differ'
    if H * W % 4 == 0:
        for v in (NHWC[3], NHWC[4]):
            nh = _abi(C, entry, cs, variant=v)
            _check(f'{what} nhwc {v[0]}/{v[2]}', nh, ref)
            _check_nhwc(C, what, nh, v, cs.K)
            assert _same_bits(nh, got), (what, v)
            again = _abi(C, entry, cs, variant=v)
            assert _same_bits(again, nh) and torch.equal(again.nh.view(torch.int16), nh.nh.view(torch.int16)), (what, v, 'two runs differ')


# ---------------------------------------------------------------------------------------------- a single workgroup with a tail, guarded
@pytest.mark.parametrize('entry', ['counted', 'weighted', 'unbiased'])
def test_single_block_with_tail(C, entry):
    """2 x 8 x 12 = 48 quads: one workgroup, 208 dead lanes (three whole waves).  A stray store by a dead lane lands in a guard band or in
    the poisoned channels of a pitch-64 copy."""
    for K, c_old in ((5, 3), (21, 17)):
        cs = _case(K, c_old, 2, 8, 12, 3.0, seed=K)
        _all_variants(C, f'{entry} 2x8x12 K{K}', entry, cs, _reference(entry, cs))


# ------------------------------------------------------------------------------------------------------------------------ arguments
@pytest.mark.parametrize('ign', [-100, 255, 0])
def test_ignore_index(C, ign):
    """VOC's 255 and an in-range ignore class (0: the reference drops those pixels; they still distil)."""
    cs = _case(21, 11, 3, 40, 52, 3.0, seed=ign % 7, ign=ign)
    assert int((cs.y == ign).sum()) >= 3
    for entry, c in (('counted', cs), ('weighted', cs), ('unbiased', cs), ('unbiased', _with(cs, lam=0.0))):
        ref = _reference(entry, c)
        assert ref.nbad == 2
        got = _all_variants(C, f'{entry} ign {ign} lam {c.lam}', entry, c, ref, variants=(NHWC[0], NHWC[3]))
        if ign == 0 and entry == 'unbiased':
            on_ignored = got.d.permute(0, 2, 3, 1)[cs.yd == 0]
            assert bool((on_ignored != 0).any()) == (c.lam > 0), 'ignored pixels take part in the distillation term and in nothing else'
    c1 = _with(cs, K=21, c_old=11, B=2, H=7, W=9, z=cs.z[:2, :, :7, :9].contiguous(), zo=cs.zo[:2, :, :7, :9].contiguous(), y=cs.y[:2, :7, :9].contiguous(),
               nu=cs.nu[:2])
    c1 = _to_device(c1)
    for entry in ('weighted', 'unbiased', 'ce'):
        c = _with(c1, lam=0.7) if entry == 'ce' else c1
        _check(f'{entry} 7x9 ign {ign}', _abi(C, entry, c), _reference(entry, c))


@pytest.mark.parametrize('gs', [0.375, 3.0])
def test_grad_scale_at_the_abi(C, gs):
    """d logits against grad_scale x the reference under the same per-element bound; the loss values do not move."""
    for B, H, W in ((3, 40, 52), (2, 7, 9)):
        cs = _case(21, 11, B, H, W, 3.0, seed=4)
        for entry in ('counted', 'weighted', 'unbiased', 'ce'):
            if entry == 'counted' and H * W % 4:
                continue
            c = _with(cs, lam=0.7) if entry == 'ce' else cs
            ref = _reference(entry, c)
            variants = (NHWC[0],) if entry == 'ce' else (NHWC[0], NHWC[3], NHWC[5])
            got = _all_variants(C, f'{entry} {H}x{W} grad_scale {gs}', entry, c, ref, gs=gs, variants=variants)
            assert torch.equal(got.l3, _abi(C, entry, c).l3)
        plain = _with(cs, lam=0.0)
        if H * W % 4 == 0:
            assert _same_bits(_abi(C, 'ce', plain, gs), _abi(C, 'counted', plain, gs))
        else:
            _check(f'ce plain {H}x{W} grad_scale {gs}', _abi(C, 'ce', plain, gs), _reference('ce', plain), gs)


# ------------------------------------------------------------------------------------------------------------- the rebase branch, mixed
def test_rebase_is_selected_per_pixel(C):
    """K = 21, c_old = 11 with distillation.  New-class logits + 200 where (h W + w) % 4 is 1 or 2 (the old group underflows: `nO` on pixels
    with an old label), old non-background logits + 400 where it is 3 (background and the new classes underflow: `nN`), nothing where it is
    0: the four pixels of every lane take different branches of the per-component selection."""
    for B, H, W in ((2, 16, 20), (2, 7, 9)):
        cs = _case(21, 11, B, H, W, 3.0, seed=5)
        m = (torch.arange(H * W) % 4).view(1, 1, H, W)
        cs.z[:, 11:] += 200.0 * ((m == 1) | (m == 2))
        cs.z[:, 1:11] += 400.0 * (m == 3)
        _to_device(cs)
        old_label = (cs.y >= 0) & (cs.y < 11)
        assert all(bool((old_label & (m[0] == r)).any()) for r in range(4))
        ref = _reference('unbiased', cs)
        what = f'rebase {H}x{W}'
        got = _all_variants(C, what, 'unbiased', cs, ref, variants=(NHWC[0], NHWC[1], NHWC[3], NHWC[4]))
        mis = _abi(C, 'unbiased', cs, variant=NHWC[3], z=_misaligned(cs.zd))
        _check(what + ' misaligned', mis, ref)
        _check_nhwc(C, what + ' misaligned', mis, NHWC[3], 21)
        assert torch.equal(mis.d.view(torch.int32), got.d.view(torch.int32))
        cs0 = _with(cs, lam=0.0)
        _check(what + ' without kd', _abi(C, 'unbiased', cs0), _reference('unbiased', cs0))
