"""GPU: the BatchNorm and pooling passes of csrc/elementwise.hip, per element, over the grid their launchers can start.

Every case calls the C ABI directly.  Every output sits in a poisoned buffer (Act / _rows: guard bands in front and behind, the pitch gap of
a concat neighbour, extra rows behind the partial rows) that must come back bit-identical outside the written region; every launch runs
twice and must give the same bits.  References are float64 torch / numpy evaluations of include/clamd.h's formulas on the same inputs,
never another call into libclamd.so.  A failure reports the worst element's index and its error / bound.

Bounds, derived from the arithmetic (EPS = 2^-24: half an fp32 ulp, relative) and from Vec8<T>::store in csrc/common.hip.h:
  storage of an fp32 value v:  fp32 none;  bf16 (rne, 8 significant bits) 2^-8 |v|;  bf16x3 hi = rne(v), lo = rne(v - hi), read back as
      the fp32 sum hi + lo: 2^-8 * 2^-8 |v| for lo, + EPS (1 + 2^-16) |v| for the sum              -> STORE_REL[dtype] * |v|
  bn_apply   u = fmaf(y, scale, shift): one rounding, EPS |u| (+ 2^-50 (|y scale| + |shift|) for the float64 reference's own sum);
      stored: + STORE_REL (|u| + that)
  g_z        = fmaf(k0, g, i), i = fmaf(k1, y, k2) under y > 0: EPS |i| for the inner value, EPS (|r| + EPS |i|) for the result
      (r = k0 g + k1 y + k2), + 2^-50 (|k0 g| + |k1 y| + |k2|) for the float64 reference's own roundings; stored: + STORE_REL (|r| + that).
      The pooled forms add gp to ga in fp32 first: the reference forms the same fp32 sum (one rne add, exact restatement).
  eval g_z   = scale * g: EPS |r|; stored as above.  Exactly +0 (all bits) where y <= 0 and in channels >= C.
  pooling    the maximum is taken on the fp32 value u BEFORE storage: the reference forms u with the kernel's rounding exactly (_fma32:
      the double product of two floats is exact, TwoSum gives the residual of the double sum, a tie of the final rounding is resolved by
      it), so pooled == storage(max u) and the routed gradient goes to the first maximum, bit for bit.  Pooled inputs are multiples of 1/4
      (exact ties inside the windows) times |scale| >= 0.5: two window values are equal or at least 1/8 apart; every case asserts that no
      window holds two different values within their bounds of each other.
  sums       exact-integer cases (ga, gp, y integers in [-4, 4], scale in {+-0.5, +-1, +-2}, integer shift, k012 in {+-0.5, +-1, +-2}): every
      term is a multiple of 1/2 with |term| <= 32 (bn_bwd_reduce, bn_bwd_eval, channel_sum: at most 65638 pixels) or <= 18
      (bn_bwd_apply_sums: at most 131769), so every partial sum is a multiple of 1/2 below 2^23, exact in fp32 in any order: the rows,
      added in float64, EQUAL the int64 reference.  Random-valued cases: n * EPS * sum |terms| per channel, n the pixels per channel
      (n - 1 additions and one product rounding per term, first order).
  finalizes  float64 header formulas on the exact integer totals (the variance from exact rational arithmetic): one fp32 ulp of the value
      + 2^-50 * the sum of the absolute terms of the expression (var, shift, the running statistics, k1, k2, dgamma, dbias cancel), the
      variance's share propagated through 1 / sqrt(var + eps) by its derivative.

Kernels, instantiations (T = float | bf16_t | split_t looped by every test marked *) and the loop paths reached:
  bn_apply_kernel<T, false|true>           test_bn_apply * Cp 32 .. 2048 (G = 4 .. 256), pitch Cp and 2 Cp, 2 x 5 x 7 plain (odd H, W; 70 G
                                           items: a partial last workgroup) and 2 x 6 x 10 pooled: one trip.  test_second_trip: plain
                                           Cp 2048 bf16x3 1 x 91 x 93 (8463 > 8192 pixels: workgroups 0 .. 270 make a second trip) and
                                           Cp 256 fp32 1 x 257 x 257 (66049 > 65536: the hoisted channel group with G = 32); pooled Cp 2048
                                           bf16 1 x 182 x 186 (8463 pooled pixels) -- bf16 carries the large pooled cases
  bn_bwd_apply_kernel<T, false|true>       test_bn_bwd_apply *, the same shapes; test_second_trip the same three, the pooled one also without ga
  bn_bwd_apply_sums_kernel<T>              test_bn_bwd_apply_sums *: random values (g_z within its bound, rows within n EPS sum |g_z|) and
                                           integer values (g_z and the row totals exact); test_second_trip Cp 2048 fp32 1 x 45 x 47 (2115 >
                                           2048 pixels) and Cp 32 bf16 1 x 363 x 363 (131769 > 131072), each random and integer: 18 x 131769
                                           < 2^23 half-units, so the integer totals are still exact there
  bn_bwd_eval_kernel<T, false|true>        test_bn_bwd_eval * C < Cp; the paired loop (plain) and the single loop (pooled); Cp 1024 at
                                           1 x 24 x 24 (576 > 512 pixels: pixel rows 0 .. 63 of the only trip have a second pixel),
                                           1 x 34 x 34 (1156: a pair trip, then a single one) and pooled 1 x 48 x 48 (576 windows, two trips)
  maxpool2x2_kernel<T, false|true>         test_maxpool2x2 *, test_second_trip Cp 2048 bf16 1 x 182 x 186
  bn_bwd_reduce_kernel<T, false>           test_bn_bwd_reduce_exact *: grids of 1 .. 3 workgroups forced through Tuning(bn_reduce_blocks):
                                           one trip without a second pixel | every pixel row with its second | the second for some pixel
                                           rows of a workgroup only | a pair trip then an odd last trip | both
  bn_bwd_reduce_kernel<T, true>            the same test, pooled: one, two and three trips of one window, with and without ga
  channel_sum_kernel<T>                    test_channel_sum_exact *: Tuning(chsum_blocks) 1 .. 3, one to three trips, C < Cp;
                                           test_channel_sum_random *: normal values (bf16x3 with a live lo plane), 2 workgroups, three trips
  sum_partial_rows<1|2|3|5>                test_rows_*: nrows 1, RL - 1, RL, RL + 1 (tail loop only), 3 RL + 1, 4 RL (one unrolled trip, no
                                           tail), 4 RL + 1, 8 RL + 3, the producers' cap; RL = 128 | 64 | 42 | 25
  bn_finalize[_total]_kernel, bn_rows_total_kernel<2|5>, bn_bwd_finalize[_total]_kernel, bn_bwd_eval_finalize_kernel<3|5>,
  channel_sum_final_kernel                 test_rows_* and test_finalize_special_channels (mean 1000 / variance 1e-4, count == 1, C < Cp,
                                           num_batches_tracked at Cp 2048)
Cross-form identities, bit for bit (test_cross_form_identities *): bn_bwd_apply == bn_bwd_apply_sums' g_z; eval g_z == bn_bwd_apply with
k012 = (scale [c < C], 0, 0) -- on gradients without exact zeros: scale * 0 is -0 for a negative scale where fmaf(scale, 0, +0) is +0;
maxpool2x2 on the stored u == bn_apply's pooled output, with scales of both signs and with positive scales only (bf16x3: the same fp32 values hi + lo; the kernel splits the sum again, and where
lo is exactly half an ulp of hi two pairs hold one number)."""
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from grid_util import DEV, EPS, EXTRA_ROWS, GUARD, STORE_REL, Act, Rows, _per_element, _raw, _store_round, _twice

pytestmark = pytest.mark.gpu

DT = [('fp32', 0), ('bf16', 1), ('bf16x3', 2)]
CPS = [32, 64, 256, 2048]


@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    C._lib.load()
    return C


# ------------------------------------------------------------------------------------------------------------------------------ buffers
def _sync():
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _normal(g, shape, dcode, zeros=0.25):
    """Standard normal, a quarter exact zeros, rounded to what the storage holds."""
    x = torch.randn(shape, generator=g, device=DEV)
    if zeros:
        x = torch.where(torch.rand(shape, generator=g, device=DEV) < zeros, torch.zeros_like(x), x)
    return _store_round(x, dcode)


def _quarters(g, shape):
    """Normal values rounded to multiples of 1/4 in [-4, 4] (exact in every storage): ties inside most 2x2 windows, a tenth exact zeros."""
    return (torch.randn(shape, generator=g, device=DEV) * 4).round().clamp(-16, 16) / 4


def _ints(g, shape):
    return torch.randint(-4, 5, shape, generator=g, device=DEV).float()


def _signed(g, n, lo, hi):
    """n values of both signs with lo <= |v| <= hi."""
    v = lo + (hi - lo) * torch.rand(n, generator=g, device=DEV)
    return torch.where(torch.rand(n, generator=g, device=DEV) < 0.5, -v, v)


def _choice(g, n, vals):
    return torch.tensor(vals, device=DEV)[torch.randint(0, len(vals), (n,), generator=g, device=DEV)]


# -------------------------------------------------------------------------------------------------------------------------- references
def _fma32(a, b, c):
    """fmaf(a, b, c) of fp32 tensors with its single rounding, exactly: p = a b is exact in float64, TwoSum gives s + err == p + c, s -> fp32
    differs from the rounding of the exact sum only where s sits on an fp32 rounding tie, which err resolves."""
    p, cd = a.double() * b.double(), c.double()
    s = p + cd
    bb = s - p
    err = (p - (s - bb)) + (cd - bb)
    r = s.float()
    d = s - r.double()
    inf = torch.full_like(r, float('inf'))
    nb = torch.nextafter(r, torch.where(d > 0, inf, -inf))
    tie = (d != 0) & (d == nb.double() - s)
    return torch.where(tie & (err != 0) & ((err > 0) == (d > 0)), nb, r)


def _windows(x, B, H, W):
    """[B H W, c] -> [B H/2 W/2, 4, c], window element q = 2 dy + dx."""
    c = x.shape[-1]
    return x.view(B, H // 2, 2, W // 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(B * (H // 2) * (W // 2), 4, c)


def _unwindows(w, B, H, W):
    c = w.shape[-1]
    return w.view(B, H // 2, W // 2, 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(B * H * W, c)


def _first_max(w):
    """[n, 4, c] -> bool [n, 4, c]: the first maximum of each window."""
    is_max = w == w.max(1, keepdim=True).values
    return is_max & (is_max.cumsum(1) == 1)


def _assert_decidable(what, w, bound):
    """No window holds two different values within their bounds of each other."""
    for i in range(4):
        for j in range(i + 1, 4):
            d = (w[:, i].double() - w[:, j].double()).abs()
            n = int(((d != 0) & (d <= bound[:, i] + bound[:, j])).sum())
            assert n == 0, f'{what}: {n} windows the reference cannot decide'


def _route(gp, u32, B, H, W):
    """gp [pooled pixels, c] at the first maximum of u32's windows, zero elsewhere -> [B H W, c] (fp32)."""
    wu = _windows(u32, B, H, W)
    _assert_decidable('route', wu, EPS * wu.double().abs())
    return _unwindows(torch.where(_first_max(wu), gp[:, None, :].expand(-1, 4, -1), torch.zeros((), device=gp.device)).contiguous(), B, H, W)


def _bound_fma(u64, dcode, terms):
    e = EPS * u64.abs() + 2.0 ** -50 * terms                       # the second part: the float64 reference's own rounding of the sum
    return e + STORE_REL[dcode] * (u64.abs() + e)


def _ref_gz(k012, gu32, y, dcode):
    """g_z = [y > 0] (k0 g + k1 y + k2) in float64, and its bound."""
    k0, k1, k2 = (k.double() for k in k012)
    g, yy = gu32.double(), y.double()
    i = k1 * yy + k2
    r = k0 * g + i
    e = EPS * i.abs() + EPS * (r.abs() + EPS * i.abs()) + 2.0 ** -50 * ((k0 * g).abs() + (k1 * yy).abs() + k2.abs())
    live = y > 0
    zero = torch.zeros_like(r)
    return torch.where(live, r, zero), torch.where(live, e + STORE_REL[dcode] * (r.abs() + e), zero)


def _same_bits(a, b):
    return torch.equal(_raw(a.view[:, :a.cp].contiguous()), _raw(b.view[:, :b.cp].contiguous()))


# --------------------------------------------------------------------------------------------------------------------- streaming kernels
def _bn_apply_case(C, what, dcode, cp, B, H, W, pool, pin, pout, seed, positive=False):
    L, s = C._lib, C._lib.stream_ptr()
    g, npix = _gen(seed), B * H * W
    y = _quarters(g, (npix, cp)) if pool else _normal(g, (npix, cp), dcode)
    sc, sh = _signed(g, cp, 0.5, 2.0), torch.randn(cp, generator=g, device=DEV)
    sc = sc.abs() if positive else sc
    ya = Act(C, npix, cp, pin * cp, dcode, y)

    def launch():
        out = Act(C, npix, cp, pout * cp, dcode)
        pooled = Act(C, npix // 4, cp, pin * cp, dcode) if pool else None
        L.call('clamd_bn_apply', ya.ptr, ya.ldc, L.ptr(sc), L.ptr(sh), out.ptr, out.ldc, pooled.ptr if pool else None,
               pooled.ldc if pool else 0, B, H, W, cp, dcode, s)
        _sync()
        return [out, pooled] if pool else [out]

    outs = _twice(what, launch)
    u64 = y.double() * sc.double() + sh.double()
    _per_element(what + ' out', ('bn_apply', dcode), outs[0].get(), u64, _bound_fma(u64, dcode, (y.double() * sc.double()).abs() + sh.double().abs()))
    if pool:
        wu = _windows(_fma32(y, sc.expand_as(y), sh.expand_as(y)), B, H, W)
        _assert_decidable(what, wu, EPS * wu.double().abs())
        assert torch.equal(outs[1].get(), _store_round(wu.max(1).values, dcode)), what + ': pooled != storage(max u)'
    return SimpleNamespace(y=ya, sc=sc, sh=sh, out=outs[0], pooled=outs[1] if pool else None)


def _bn_bwd_apply_case(C, what, dcode, cp, B, H, W, pool, pin, pout, seed, with_ga=True, sums=False, integer=False):
    """clamd_bn_bwd_apply, or (sums) clamd_bn_bwd_apply_sums with its rows.  integer (plain form): ga, y integers in [-4, 4], k012 in
    {+-0.5, +-1, +-2}: g_z is a multiple of 1/2 with |g_z| <= 18, exact in every storage, and every partial sum of up to 2^23 / 18 = 466033
    pixels is a multiple of 1/2 below 2^23, exact in fp32 in any order: g_z and the row totals EQUAL the reference."""
    L, s = C._lib, C._lib.stream_ptr()
    g, npix = _gen(seed), B * H * W
    y = _quarters(g, (npix, cp)) if pool else _normal(g, (npix, cp), dcode)
    ga = _normal(g, (npix, cp), dcode) if with_ga else None
    gp = _normal(g, (npix // 4, cp), dcode) if pool else None
    sc, sh = _signed(g, cp, 0.5, 2.0), torch.randn(cp, generator=g, device=DEV)
    k012 = torch.randn(3, cp, generator=g, device=DEV)
    if integer:
        assert not pool and with_ga and npix * 18 < 2 ** 23
        y, ga = _ints(g, (npix, cp)), _ints(g, (npix, cp))
        k012 = _choice(g, 3 * cp, [-2.0, -1.0, -0.5, 0.5, 1.0, 2.0]).view(3, cp).contiguous()
    ya, gaa = Act(C, npix, cp, cp, dcode, y), Act(C, npix, cp, pin * cp, dcode, ga) if with_ga else None
    gpa = Act(C, npix // 4, cp, pin * cp, dcode, gp) if pool else None
    nrows = L.load().clamd_bn_bwd_apply_sums_rows(B, H, W, cp) if sums else 0

    def launch():
        gz = Act(C, npix, cp, pout * cp, dcode)
        if sums:
            rows = Rows(nrows, cp)
            L.call('clamd_bn_bwd_apply_sums', gaa.ptr, gaa.ldc, ya.ptr, ya.ldc, L.ptr(k012), gz.ptr, gz.ldc, rows.ptr, nrows, B, H, W, cp, dcode, s)
        else:
            L.call('clamd_bn_bwd_apply', gaa.ptr if with_ga else None, gaa.ldc if with_ga else 0, gpa.ptr if pool else None, gpa.ldc if pool else 0,
                   ya.ptr, ya.ldc, L.ptr(sc) if pool else None, L.ptr(sh) if pool else None, L.ptr(k012), gz.ptr, gz.ldc, B, H, W, cp, dcode, s)
        _sync()
        return [gz, rows] if sums else [gz]

    outs = _twice(what, launch)
    gu = ga if with_ga else torch.zeros_like(y)
    if pool:
        gu = gu + _route(gp, _fma32(y, sc.expand_as(y), sh.expand_as(y)), B, H, W)          # the kernel's own fp32 add
    ref, bound = _ref_gz(k012, gu, y, dcode)
    name = 'bn_bwd_apply_sums' if sums else 'bn_bwd_apply'
    _per_element(what + ' g_z', (name, dcode), outs[0].get(), ref, bound)
    assert bool(outs[0].zero_bits()[y <= 0].all()), what + ': g_z is not +0 where y <= 0'
    if integer:
        assert torch.equal(outs[0].get().double(), ref), what + ': integer-valued g_z differs from the reference'
    if sums and integer:
        bad = (outs[1].view.double().sum(0) != ref.sum(0)).nonzero()
        assert bad.numel() == 0, f'{what}: row totals differ from the exact reference in channels {bad[:4].flatten().tolist()}'
    elif sums:
        # the rows add the fp32 g_z before its storage rounding: n additions of values within EPS-relative bounds of ref
        fref, fbound = _ref_gz(k012, gu, y, 0)
        tot = outs[1].view.double().sum(0)
        _per_element(what + ' rows', (name + ' rows', dcode), tot, fref.sum(0), fbound.sum(0) + npix * EPS * fref.abs().sum(0))
    return SimpleNamespace(y=ya, ga=gaa, gp=gpa, sc=sc, sh=sh, k012=k012, gz=outs[0])


def _bn_bwd_eval_case(C, what, dcode, cp, Cl, B, H, W, pool, pin, pout, seed, with_ga=True, integer=False, zeros=0.25):
    """clamd_bn_bwd_eval: g_z per element, the three rows exactly (integer) or within n EPS sum |terms|."""
    L, s = C._lib, C._lib.stream_ptr()
    g, npix = _gen(seed), B * H * W
    if integer:
        y, ga, gp = _ints(g, (npix, cp)), _ints(g, (npix, cp)), _ints(g, (npix // 4, cp))
        sc, sh = _choice(g, cp, [-2.0, -1.0, -0.5, 0.5, 1.0, 2.0]), _ints(g, (cp,))
    else:
        y = _quarters(g, (npix, cp)) if pool else _normal(g, (npix, cp), dcode)
        ga, gp = _normal(g, (npix, cp), dcode, zeros), _normal(g, (npix // 4, cp), dcode, zeros)
        sc, sh = _signed(g, cp, 0.5, 2.0), torch.randn(cp, generator=g, device=DEV)
    ya, gaa = Act(C, npix, cp, cp, dcode, y), Act(C, npix, cp, pin * cp, dcode, ga) if with_ga else None
    gpa = Act(C, npix // 4, cp, pin * cp, dcode, gp) if pool else None
    nrows = L.load().clamd_bn_bwd_eval_rows(B, H, W, cp, 1 if pool else 0)
    assert nrows > 0

    def launch():
        gz, rows = Act(C, npix, cp, pout * cp, dcode), Rows(nrows, 3, cp)
        L.call('clamd_bn_bwd_eval', gaa.ptr if with_ga else None, gaa.ldc if with_ga else 0, gpa.ptr if pool else None, gpa.ldc if pool else 0,
               ya.ptr, ya.ldc, L.ptr(sc), L.ptr(sh) if pool else None, gz.ptr, gz.ldc, rows.ptr, nrows, B, H, W, cp, Cl, dcode, s)
        _sync()
        return [gz, rows]

    gz, rows = _twice(what, launch)
    gu = ga if with_ga else torch.zeros_like(y)
    if pool:
        gu = gu + _route(gp, _fma32(y, sc.expand_as(y), sh.expand_as(y)), B, H, W)
    live = (y > 0) & (torch.arange(cp, device=DEV) < Cl)
    r = torch.where(live, sc.double() * gu.double(), torch.zeros((), dtype=torch.float64, device=DEV))
    e = EPS * r.abs()
    _per_element(what + ' g_z', ('bn_bwd_eval', dcode), gz.get(), r, e + STORE_REL[dcode] * (r.abs() + e))
    assert bool(gz.zero_bits()[~live].all()), what + ': g_z is not +0 where y <= 0 or in channels >= C'
    tot = rows.view.double().sum(0)
    gd, yd = gu.double(), y.double()
    ref = torch.stack([gd.sum(0), (gd * yd).sum(0), r.sum(0)])
    if integer:
        bad = (tot != ref).nonzero()
        assert bad.numel() == 0, f'{what}: row totals differ from the integer reference at (kind, channel) {bad[:4].tolist()}'
    else:
        mag = torch.stack([gd.abs().sum(0), (gd * yd).abs().sum(0), r.abs().sum(0)])
        _per_element(what + ' rows', ('bn_bwd_eval rows', dcode), tot, ref, npix * EPS * mag)
    return SimpleNamespace(y=ya, ga=gaa, gp=gpa, sc=sc, sh=sh, gz=gz, nrows=nrows)


def _maxpool_case(C, what, dcode, cp, B, H, W, pin, pout, seed):
    """clamd_maxpool2x2 and _bwd without sign: the maximum of the stored values and the routing to its first occurrence, exactly."""
    L, s = C._lib, C._lib.stream_ptr()
    g, npix = _gen(seed), B * H * W
    x, gp = _quarters(g, (npix, cp)), _normal(g, (npix // 4, cp), dcode)
    xa, gpa = Act(C, npix, cp, pin * cp, dcode, x), Act(C, npix // 4, cp, cp, dcode, gp)

    def launch():
        out, gx = Act(C, npix // 4, cp, pout * cp, dcode), Act(C, npix, cp, pout * cp, dcode)
        L.call('clamd_maxpool2x2', xa.ptr, xa.ldc, None, out.ptr, out.ldc, B, H, W, cp, dcode, s)
        L.call('clamd_maxpool2x2_bwd', xa.ptr, xa.ldc, None, gpa.ptr, gpa.ldc, gx.ptr, gx.ldc, B, H, W, cp, dcode, s)
        _sync()
        return [out, gx]

    out, gx = _twice(what, launch)
    wx = _windows(x, B, H, W)
    assert torch.equal(out.get(), wx.max(1).values), what + ': pooled'
    first = _first_max(wx)
    assert int(first.sum()) == wx.shape[0] * cp and int((wx == wx.max(1, keepdim=True).values).sum()) > int(first.sum()), 'ties expected'
    ref = _unwindows(torch.where(first, gp[:, None, :].expand(-1, 4, -1), torch.zeros((), device=DEV)).contiguous(), B, H, W)
    assert torch.equal(gx.get(), ref), what + ': gradient routing'
    assert bool(gx.zero_bits()[_unwindows((~first).contiguous(), B, H, W)].all()), what + ': +0 off the maximum'


@pytest.mark.parametrize('cp', CPS)
@pytest.mark.parametrize('name,dcode', DT)
def test_bn_apply(C, name, dcode, cp):
    for pin, pout in ((1, 1), (2, 1), (1, 2)):
        _bn_apply_case(C, f'bn_apply {name} Cp{cp} pitch {pin}/{pout}', dcode, cp, 2, 5, 7, False, pin, pout, cp + pin)
        _bn_apply_case(C, f'bn_apply+pool {name} Cp{cp} pitch {pin}/{pout}', dcode, cp, 2, 6, 10, True, pin, pout, cp + pout)


@pytest.mark.parametrize('cp', CPS)
@pytest.mark.parametrize('name,dcode', DT)
def test_bn_bwd_apply(C, name, dcode, cp):
    for pin, pout in ((1, 1), (2, 1), (1, 2)):
        _bn_bwd_apply_case(C, f'bn_bwd_apply {name} Cp{cp} pitch {pin}/{pout}', dcode, cp, 2, 5, 7, False, pin, pout, cp + pin)
        _bn_bwd_apply_case(C, f'bn_bwd_apply+pool {name} Cp{cp} pitch {pin}/{pout}', dcode, cp, 2, 6, 10, True, pin, pout, cp + pout)
    _bn_bwd_apply_case(C, f'bn_bwd_apply+pool, no ga {name} Cp{cp}', dcode, cp, 2, 6, 10, True, 2, 2, cp, with_ga=False)


@pytest.mark.parametrize('cp', CPS)
@pytest.mark.parametrize('name,dcode', DT)
def test_bn_bwd_apply_sums(C, name, dcode, cp):
    for pin, pout in ((1, 1), (2, 2)):
        _bn_bwd_apply_case(C, f'bn_bwd_apply_sums {name} Cp{cp} pitch {pin}/{pout}', dcode, cp, 2, 5, 7, False, pin, pout, cp + pin, sums=True)
        _bn_bwd_apply_case(C, f'bn_bwd_apply_sums {name} Cp{cp} pitch {pin}/{pout} integer', dcode, cp, 2, 5, 7, False, pin, pout, cp + pout,
                           sums=True, integer=True)


@pytest.mark.parametrize('cp', CPS)
@pytest.mark.parametrize('name,dcode', DT)
def test_bn_bwd_eval(C, name, dcode, cp):
    Cl = cp - 11
    for pin, pout in ((1, 1), (2, 2)):
        _bn_bwd_eval_case(C, f'bn_bwd_eval {name} Cp{cp} pitch {pin}/{pout}', dcode, cp, Cl, 2, 5, 7, False, pin, pout, cp + pin)
        _bn_bwd_eval_case(C, f'bn_bwd_eval+pool {name} Cp{cp} pitch {pin}/{pout}', dcode, cp, Cl, 2, 6, 10, True, pin, pout, cp + pout)
    _bn_bwd_eval_case(C, f'bn_bwd_eval+pool, no ga {name} Cp{cp}', dcode, cp, cp, 2, 6, 10, True, 1, 2, cp, with_ga=False)


@pytest.mark.parametrize('name,dcode', DT)
def test_bn_bwd_eval_trips(C, name, dcode):
    """Cp 1024: 256 workgroups of 2 pixel rows.  576 pixels: one trip, the second pixel for pixel rows 0 .. 63 only; 1156: a pair trip
    and a single one; pooled 576 windows: two trips of the single loop.  Integer inputs: the rows exactly."""
    for B, H, W, pool in ((1, 24, 24, False), (1, 34, 34, False), (1, 48, 48, True)):
        assert C._lib.load().clamd_bn_bwd_eval_rows(B, H, W, 1024, int(pool)) == 256
        _bn_bwd_eval_case(C, f'bn_bwd_eval {name} Cp1024 {B}x{H}x{W} pool {pool}', dcode, 1024, 1000, B, H, W, pool, 1, 1, H, integer=True)
    _bn_bwd_eval_case(C, f'bn_bwd_eval {name} Cp1024 1x34x34 random', dcode, 1024, 1000, 1, 34, 34, False, 1, 2, 5)


@pytest.mark.parametrize('cp', CPS)
@pytest.mark.parametrize('name,dcode', DT)
def test_maxpool2x2(C, name, dcode, cp):
    for pin, pout in ((1, 1), (2, 1), (1, 2)):
        _maxpool_case(C, f'maxpool2x2 {name} Cp{cp} pitch {pin}/{pout}', dcode, cp, 2, 6, 10, pin, pout, cp + pin)


SECOND_TRIP = [
    ('bn_apply', 'bf16x3', 2, 2048, 1, 91, 93, False), ('bn_apply', 'fp32', 0, 256, 1, 257, 257, False), ('bn_apply', 'bf16', 1, 2048, 1, 182, 186, True),
    ('bn_bwd_apply', 'fp32', 0, 2048, 1, 91, 93, False), ('bn_bwd_apply', 'bf16x3', 2, 256, 1, 257, 257, False),
    ('bn_bwd_apply', 'bf16', 1, 2048, 1, 182, 186, True), ('bn_bwd_apply without ga', 'bf16', 1, 2048, 1, 182, 186, True),
    ('bn_bwd_apply_sums', 'fp32', 0, 2048, 1, 45, 47, False), ('bn_bwd_apply_sums', 'bf16', 1, 32, 1, 363, 363, False),
    ('maxpool2x2', 'bf16', 1, 2048, 1, 182, 186, True),
]


@pytest.mark.parametrize('kernel,name,dcode,cp,B,H,W,pool', SECOND_TRIP)
def test_second_trip(C, kernel, name, dcode, cp, B, H, W, pool):
    """The smallest shapes past the grid caps (8192 workgroups; 2048 for bn_bwd_apply_sums): a second, partial trip of the grid-stride loop.
    bn_bwd_apply_sums runs each shape with random values and with integer values: 2115 and 131769 pixels are both below the 466033 up to
    which the integer sums are exact, so a pixel of the second trip missing from the rows fails the equality."""
    items = B * (H // 2) * (W // 2) * (cp // 8) if pool else B * H * W * (cp // 8)
    cap = (2048 if kernel == 'bn_bwd_apply_sums' else 8192) * 256
    assert cap < items < 2 * cap and items % cap
    what = f'{kernel} {name} Cp{cp} {B}x{H}x{W} second trip'
    if kernel == 'bn_apply':
        _bn_apply_case(C, what, dcode, cp, B, H, W, pool, 1, 1, 3)
    elif kernel == 'maxpool2x2':
        _maxpool_case(C, what, dcode, cp, B, H, W, 1, 1, 3)
    else:
        _bn_bwd_apply_case(C, what, dcode, cp, B, H, W, pool, 1, 1, 3, sums=kernel == 'bn_bwd_apply_sums', with_ga=not kernel.endswith('without ga'))
        if kernel == 'bn_bwd_apply_sums':
            _bn_bwd_apply_case(C, what + ' integer', dcode, cp, B, H, W, pool, 1, 1, 4, sums=True, integer=True)


@pytest.mark.parametrize('name,dcode', DT)
def test_cross_form_identities(C, name, dcode):
    L, s = C._lib, C._lib.stream_ptr()
    for cp in (32, 256):
        B, H, W = 2, 6, 10
        npix = B * H * W
        a = _bn_bwd_apply_case(C, f'identity {name} Cp{cp}: bn_bwd_apply', dcode, cp, B, H, W, False, 2, 1, 9)
        b = _bn_bwd_apply_case(C, f'identity {name} Cp{cp}: bn_bwd_apply_sums', dcode, cp, B, H, W, False, 2, 1, 9, sums=True)
        assert _same_bits(a.gz, b.gz), 'bn_bwd_apply and bn_bwd_apply_sums write different g_z'
        for pool in (False, True):
            Cl = cp - 5
            e = _bn_bwd_eval_case(C, f'identity {name} Cp{cp}: bn_bwd_eval pool {pool}', dcode, cp, Cl, B, H, W, pool, 1, 1, 9, zeros=0.0)
            k012 = torch.zeros(3, cp, device=DEV)
            k012[0, :Cl] = e.sc[:Cl]
            gz = Act(C, npix, cp, cp, dcode)
            L.call('clamd_bn_bwd_apply', e.ga.ptr, e.ga.ldc, e.gp.ptr if pool else None, e.gp.ldc if pool else 0, e.y.ptr, e.y.ldc,
                   L.ptr(e.sc) if pool else None, L.ptr(e.sh) if pool else None, L.ptr(k012), gz.ptr, gz.ldc, B, H, W, cp, dcode, s)
            _sync()
            assert gz.guards_intact() and _same_bits(gz, e.gz), f'eval g_z != bn_bwd_apply with k012 = (scale, 0, 0) (pool {pool})'
        f = _bn_apply_case(C, f'identity {name} Cp{cp}: bn_apply+pool', dcode, cp, B, H, W, True, 1, 2, 9)
        pos = _bn_apply_case(C, f'identity {name} Cp{cp}: bn_apply+pool, positive scale', dcode, cp, B, H, W, True, 1, 2, 10, positive=True)
        assert bool((f.sc < 0).any()) and bool((pos.sc > 0).all())
        for r in (f, pos):
            p2 = Act(C, npix // 4, cp, cp, dcode)
            L.call('clamd_maxpool2x2', r.out.ptr, r.out.ldc, None, p2.ptr, p2.ldc, B, H, W, cp, dcode, s)
            _sync()
            # bf16x3: the same VALUES -- maxpool2x2 splits hi + lo again, and at a rounding tie of hi another pair holds the same number
            same = torch.equal(_raw(p2.get()), _raw(r.pooled.get())) if dcode == 2 else _same_bits(p2, r.pooled)
            assert p2.guards_intact() and same, 'maxpool2x2 on u != the pooled output of bn_apply'


# ---------------------------------------------------------------------------------------------------------------------------- reductions
def _ref_sums(gu, y):
    g, yy, pos = gu.double(), y.double(), (y > 0).double()
    return torch.stack([g.sum(0), (g * yy).sum(0), (g * pos).sum(0), pos.sum(0), yy.sum(0)]), \
        torch.stack([g.abs().sum(0), (g * yy).abs().sum(0), (g * pos).abs().sum(0), pos.sum(0), yy.abs().sum(0)])


def _reduce_case(C, what, dcode, cp, B, H, W, pool, blocks, seed, integer=True, with_ga=True, expect_rows=None):
    L, s = C._lib, C._lib.stream_ptr()
    g, npix = _gen(seed), B * H * W
    if integer:
        y, ga, gp = _ints(g, (npix, cp)), _ints(g, (npix, cp)), _ints(g, (npix // 4, cp))
        sc, sh = _choice(g, cp, [-2.0, -1.0, -0.5, 0.5, 1.0, 2.0]), _ints(g, (cp,))
    else:
        y = _quarters(g, (npix, cp)) if pool else _normal(g, (npix, cp), dcode)
        ga, gp = _normal(g, (npix, cp), dcode), _normal(g, (npix // 4, cp), dcode)
        sc, sh = _signed(g, cp, 0.5, 2.0), torch.randn(cp, generator=g, device=DEV)
    tune = L.Tuning(bn_reduce_blocks=blocks) if blocks else None
    nrows = L.stat_rows(L.OP_BN_BWD_REDUCE, B, H, W, 1 if pool else 0, cp, dcode, False, tune)
    assert expect_rows is None or nrows == expect_rows, (what, nrows, expect_rows)
    ya, gaa = Act(C, npix, cp, 2 * cp, dcode, y), Act(C, npix, cp, cp, dcode, ga) if with_ga else None
    gpa = Act(C, npix // 4, cp, 2 * cp, dcode, gp) if pool else None

    def launch():
        rows = Rows(nrows, 5, cp)
        L.call('clamd_bn_bwd_reduce', gaa.ptr if with_ga else None, gaa.ldc if with_ga else 0, gpa.ptr if pool else None, gpa.ldc if pool else 0,
               ya.ptr, ya.ldc, L.ptr(sc) if pool else None, L.ptr(sh) if pool else None, rows.ptr, nrows, B, H, W, cp, dcode, L.tune_ptr(tune), s)
        _sync()
        return [rows]

    rows, = _twice(what, launch)
    gu = ga if with_ga else torch.zeros_like(y)
    if pool:
        gu = gu + _route(gp, _fma32(y, sc.expand_as(y), sh.expand_as(y)), B, H, W)
    ref, mag = _ref_sums(gu, y)
    tot = rows.view.double().sum(0)
    if integer:
        bad = (tot != ref).nonzero()
        assert bad.numel() == 0, f'{what}: totals differ from the integer reference at (sum, channel) {bad[:4].tolist()}: ' \
                                 f'{[(float(tot[i, j]), float(ref[i, j])) for i, j in bad[:4].tolist()]}'
    else:
        _per_element(what, ('bn_bwd_reduce', dcode), tot, ref, npix * EPS * mag)


@pytest.mark.parametrize('cp', CPS)
@pytest.mark.parametrize('name,dcode', DT)
def test_bn_bwd_reduce_exact(C, name, dcode, cp):
    """Forced grids of 1 .. 3 workgroups, R = 256 / (Cp / 8) pixel rows each, stride S = grid * R pixels; integer inputs, exact totals."""
    R = 2048 // cp
    k = max(1, (3 * R) // 5)                                 # a part of a workgroup's pixel rows (1 at Cp 2048, where R == 1)
    plain = [(3, 3 * R - (1 if R > 1 else 0), 'one trip, no second pixel'),
             (2, 4 * R, 'every pixel row with its second pixel'),
             (2, 2 * R + R + k if R > 1 else 3, 'the second pixel for some pixel rows of a workgroup only'),
             (1, 2 * R + k, 'a pair trip, then an odd last trip'),
             (3, 3 * (3 * R) + R + k, 'a pair trip, then a trip with the second pixel for some rows only')]
    for grid, npix, path in plain:
        _reduce_case(C, f'bn_bwd_reduce {name} Cp{cp} grid {grid} npix {npix}: {path}', dcode, cp, 1, 1, npix, False, grid, npix, expect_rows=grid)
    for grid, nwin, path in [(3, 3 * R, 'one trip'), (2, 2 * R + R + k, 'two trips, the second partial'), (1, 2 * R + k, 'three trips')]:
        for with_ga in (True, False):
            _reduce_case(C, f'bn_bwd_reduce+pool {name} Cp{cp} grid {grid} windows {nwin} ga {with_ga}: {path}', dcode, cp, 1, 2, 2 * nwin, True,
                         grid, nwin, with_ga=with_ga, expect_rows=grid)
    # the library's own grid, past its cap (256 .. 1024 workgroups): 257 workgroups' worth of pixels and a few more
    cap = min(max(131072 // cp, 256), 1024)
    _reduce_case(C, f'bn_bwd_reduce {name} Cp{cp} natural grid', dcode, cp, 1, 1, cap * R + R + k, False, 0, 7, expect_rows=cap)


@pytest.mark.parametrize('name,dcode', DT)
def test_bn_bwd_reduce_random(C, name, dcode):
    _reduce_case(C, f'bn_bwd_reduce {name} Cp64 random', dcode, 64, 1, 1, 2 * 64 + 37, False, 2, 1, integer=False)
    _reduce_case(C, f'bn_bwd_reduce+pool {name} Cp64 random', dcode, 64, 1, 2, 2 * (2 * 64 + 37), True, 2, 2, integer=False)


@pytest.mark.parametrize('cp', CPS)
@pytest.mark.parametrize('name,dcode', DT)
def test_channel_sum_exact(C, name, dcode, cp):
    L, s = C._lib, C._lib.stream_ptr()
    R, Cl = 2048 // cp, cp - 3
    wsb = L.load().clamd_channel_sum_workspace_bytes(cp)
    for grid, npix in [(3, 3 * R - (1 if R > 1 else 0)), (2, 2 * R + max(1, R // 3)), (1, 2 * R + max(1, R // 3)), (0, 1024 * R + R + 1)]:
        what = f'channel_sum {name} Cp{cp} grid {grid} npix {npix}'
        x = _ints(_gen(npix), (npix, cp))
        xa = Act(C, npix, cp, 2 * cp, dcode, x)
        tune = L.Tuning(chsum_blocks=grid) if grid else None

        def launch():
            out, ws = Rows(Cl, fill=float('nan')), Rows(wsb // (4 * cp), cp)
            L.call('clamd_channel_sum', xa.ptr, xa.ldc, out.ptr, npix, cp, Cl, dcode, ws.ptr, wsb, L.tune_ptr(tune), s)
            _sync()
            return [out, ws]

        out, ws = _twice(what, launch)
        assert torch.equal(out.view.double(), x.double().sum(0)[:Cl]), what
        used = grid if grid else min(max(131072 // cp, 256), 1024)
        assert bool(torch.isnan(ws.view[used:]).all()) and not bool(torch.isnan(ws.view[:used]).any()), what + ': rows of the workspace written'


@pytest.mark.parametrize('name,dcode', DT)
def test_channel_sum_random(C, name, dcode):
    """Normal values in the storage's own precision (bf16x3: a live lo plane), grids of 2 workgroups over three trips, the last partial:
    |out - ref| <= n EPS sum |x| for the fp32 sums + EPS |ref| for the fp32 result."""
    L, s = C._lib, C._lib.stream_ptr()
    for cp in (32, 256):
        R, Cl = 2048 // cp, cp - 3
        npix = 2 * (2 * R) + R + max(1, R // 3)
        what = f'channel_sum {name} Cp{cp} grid 2 npix {npix} random'
        x = _normal(_gen(cp), (npix, cp), dcode, zeros=0.0)
        assert dcode != 2 or bool((x != x.to(torch.bfloat16).float()).any())
        xa = Act(C, npix, cp, 2 * cp, dcode, x)
        wsb = L.load().clamd_channel_sum_workspace_bytes(cp)
        tune = L.Tuning(chsum_blocks=2)

        def launch():
            out, ws = Rows(Cl, fill=float('nan')), Rows(wsb // (4 * cp), cp)
            L.call('clamd_channel_sum', xa.ptr, xa.ldc, out.ptr, npix, cp, Cl, dcode, ws.ptr, wsb, L.tune_ptr(tune), s)
            _sync()
            return [out, ws]

        out, ws = _twice(what, launch)
        ref = x.double().sum(0)[:Cl]
        _per_element(what, ('channel_sum', dcode), out.view, ref, npix * EPS * x.double().abs().sum(0)[:Cl] + EPS * ref.abs())


# ------------------------------------------------------------------------------------------------------------ row sums and finalizes
RL = {1: 128, 2: 64, 3: 42, 5: 25}
CAP = {1: 2048, 2: 4096, 3: 2048, 5: 1024}


def _nrows_list(nk):
    rl = RL[nk]
    return [1, rl - 1, rl, rl + 1, 3 * rl + 1, 4 * rl, 4 * rl + 1, 8 * rl + 3, CAP[nk]]


def _int_rows(nrows, nk, cp, mul=(1, 1, 1, 1, 1)):
    """Rows [nrows][nk][cp] of positive integers that depend on (row, kind, channel): a dropped, doubled or mis-indexed row changes every
    total.  -> Rows (NaN rows behind), the exact int64 totals [nk][cp] as numpy."""
    r = torch.arange(nrows, device=DEV).view(-1, 1, 1)
    k = torch.arange(nk, device=DEV).view(1, -1, 1)
    c = torch.arange(cp, device=DEV).view(1, 1, -1)
    v = (1 + (r * 131 + k * 17 + c * 29) % 13) * torch.tensor(mul[:nk], device=DEV).view(1, -1, 1)
    rows = Rows(nrows, nk, cp)
    rows.view.copy_(v.float())
    rows.buf[GUARD + rows.n * rows.per:GUARD + (rows.n + EXTRA_ROWS) * rows.per] = float('nan')       # a read past nrows shows in every total
    rows.before = rows.buf.clone()
    return rows, v.sum(0).cpu().numpy().astype(np.int64)


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def _np(t):
    return t.detach().cpu().numpy()


def _check_vec(what, key, got, ref, bound):
    _per_element(what, key, torch.from_numpy(np.asarray(got, np.float64)), torch.from_numpy(np.asarray(ref, np.float64)),
                 torch.from_numpy(np.asarray(bound, np.float64)))


def _ref_bn_finalize(s0, s1, count, gamma, beta, rm0, rv0, mom, eps, Cl):
    """include/clamd.h's clamd_bn_finalize (train mode) in float64 on exact integer totals; (name -> value, bound) over Cp channels."""
    cp = len(s0)
    cnt = int(count)
    var = np.array([float(max(Fraction(int(b) * cnt - int(a) * int(a), cnt * cnt), 0)) for a, b in zip(s0, s1)])
    mean = s0.astype(np.float64) / count
    dv = 2.0 ** -50 * (s1 / count + mean * mean)               # the kernel forms var = s1 / count - mean^2 in float64: it cancels
    istd = 1.0 / np.sqrt(var + eps)
    di = 0.5 * istd ** 3 * dv
    g = np.where(np.arange(cp) < Cl, np.pad(gamma.astype(np.float64), (0, cp - len(gamma))), 0.0)
    b = np.where(np.arange(cp) < Cl, np.pad(beta.astype(np.float64), (0, cp - len(beta))), 0.0)
    out = {'scale': (g * istd, np.abs(g) * di), 'save_mean': (mean, 0.0), 'save_istd': (istd, di),
           'shift': (b - mean * (g * istd), 2.0 ** -50 * (np.abs(b) + np.abs(mean * g * istd)) + np.abs(mean * g) * di)}
    unb = var * (count / (count - 1.0)) if count > 1 else var
    f = count / (count - 1.0) if count > 1 else 1.0
    m, v = mean[:Cl], unb[:Cl]
    out['running_mean'] = ((1 - mom) * rm0 + mom * m, 2.0 ** -50 * (np.abs(rm0) + np.abs(m)))
    out['running_var'] = ((1 - mom) * rv0 + mom * v, 2.0 ** -50 * (np.abs(rv0) + np.abs(v)) + mom * f * dv[:Cl])
    return {k: (val, _ulp32(val) + bd) for k, (val, bd) in out.items()}


def _ref_bn_bwd_finalize(s, gs0, gs1, count, gamma, mu, istd, Cl, with_bias=True):
    """clamd_bn_bwd_finalize in float64 on exact totals s [5][Cp] (gs: the totals behind k0, k1, k2)."""
    cp = s.shape[1]
    s = s.astype(np.float64)
    mu, istd = mu.astype(np.float64), istd.astype(np.float64)
    g = np.where(np.arange(cp) < Cl, np.pad(gamma.astype(np.float64), (0, cp - len(gamma))), 0.0)
    k0 = g * istd
    A, Bt = istd * istd * gs1 / count, istd * istd * mu * gs0 / count
    c2 = A - Bt
    k1, k2 = -k0 * c2, k0 * (mu * c2 - gs0 / count)
    e1 = 2.0 ** -50 * np.abs(k0) * (np.abs(A) + np.abs(Bt))
    e2 = 2.0 ** -50 * np.abs(k0) * (np.abs(mu) * (np.abs(A) + np.abs(Bt)) + np.abs(gs0 / count))
    out = {'k0': (k0, 0.0), 'k1': (k1, e1), 'k2': (k2, e2),
           'dgamma': ((istd * (s[1] - mu * s[0]))[:Cl], (2.0 ** -50 * istd * (np.abs(s[1]) + np.abs(mu * s[0])))[:Cl]), 'dbeta': (s[0][:Cl], 0.0)}
    if with_bias:
        out['dbias'] = ((k0 * s[2] + k1 * s[4] + k2 * s[3])[:Cl],
                        (2.0 ** -50 * (np.abs(k0 * s[2]) + np.abs(k1 * s[4]) + np.abs(k2 * s[3])) + e1 * np.abs(s[4]) + e2 * np.abs(s[3]))[:Cl])
    return {k: (val, _ulp32(val) + bd) for k, (val, bd) in out.items()}


@pytest.mark.parametrize('nk', [2, 5])
def test_rows_total_exact(C, nk):
    """clamd_bn_rows_total: the doubles are the integer sums; reduce = the first two kinds and the count; nothing else written."""
    L, s = C._lib, C._lib.stream_ptr()
    for cp, nrows in [(32, n) for n in _nrows_list(nk)] + [(2048, 8 * RL[nk] + 3)]:
        rows, tot = _int_rows(nrows, nk, cp)

        def launch():
            totals, red = Rows(nk, cp, dtype=torch.float64), Rows(1, 2 * cp + 1, dtype=torch.float64)
            L.call('clamd_bn_rows_total', rows.ptr, nrows, nk, cp, float(3 * nrows), totals.ptr, red.ptr, s)
            _sync()
            return [totals, red]

        totals, red = _twice(f'bn_rows_total<{nk}> Cp{cp} nrows {nrows}', launch)
        assert np.array_equal(_np(totals.view), tot.astype(np.float64)), (nk, cp, nrows)
        assert np.array_equal(_np(red.view)[0, :2 * cp].reshape(2, cp), tot[:2].astype(np.float64)) and float(red.view[0, 2 * cp]) == 3 * nrows
        assert rows.guards_intact()


def test_rows_sum_exact(C):
    """clamd_rows_sum (sum_partial_rows<1>): out[c] for c < C, nothing behind it."""
    L, s = C._lib, C._lib.stream_ptr()
    for cp, Cl, nrows in [(32, 27, n) for n in _nrows_list(1)] + [(2048, 2048, 515), (2048, 2041, 1)]:
        rows, tot = _int_rows(nrows, 1, cp)

        def launch():
            out = Rows(Cl)
            L.call('clamd_rows_sum', rows.ptr, nrows, out.ptr, cp, Cl, s)
            _sync()
            return [out]

        out, = _twice(f'rows_sum Cp{cp} nrows {nrows}', launch)
        assert np.array_equal(_np(out.view).astype(np.float64), tot[0, :Cl].astype(np.float64)), (cp, nrows)


def _vecs(names, n):
    return {k: Rows(n) for k in names}


def _finalize_fwd(C, what, rows, nrows, cp, Cl, count, gamma, beta, rm0, rv0, total):
    """clamd_bn_finalize on the rows, or clamd_bn_rows_total + clamd_bn_finalize_total.  -> outputs, num_batches_tracked."""
    L, s = C._lib, C._lib.stream_ptr()

    def launch():
        o = _vecs(('scale', 'shift', 'save_mean', 'save_istd'), cp)
        o['running_mean'], o['running_var'] = Rows(Cl), Rows(Cl)
        o['running_mean'].view.copy_(rm0)
        o['running_var'].view.copy_(rv0)
        o['nbt'] = Rows(1, fill=41, dtype=torch.int64)
        for k in ('running_mean', 'running_var', 'nbt'):
            o[k].before = o[k].buf.clone()
        tail = (L.ptr(gamma), L.ptr(beta), o['running_mean'].ptr, o['running_var'].ptr, o['scale'].ptr, o['shift'].ptr, o['save_mean'].ptr,
                o['save_istd'].ptr, cp, Cl)
        if total:
            red = Rows(1, 2 * cp + 1, dtype=torch.float64)
            L.call('clamd_bn_rows_total', rows.ptr, nrows, 2, cp, float(count), None, red.ptr, s)
            L.call('clamd_bn_finalize_total', red.ptr, *tail, 0.1, 1e-5, o['nbt'].ptr, s)
        else:
            L.call('clamd_bn_finalize', rows.ptr, nrows, *tail, float(count), 0.1, 1e-5, o['nbt'].ptr, s)
        _sync()
        return list(o.values())

    names = ('scale', 'shift', 'save_mean', 'save_istd', 'running_mean', 'running_var', 'nbt')
    o = dict(zip(names, _twice(what, launch)))
    assert int(o['nbt'].view[0]) == 42, what + ': num_batches_tracked incremented exactly once'
    return o


def _check_fwd(what, o, ref, cp, Cl):
    for k, (val, bound) in ref.items():
        _check_vec(f'{what} {k}', ('bn_finalize', k), _np(o[k].view), val, bound)
    assert bool((o['scale'].view[Cl:] == 0).all()) and bool((o['shift'].view[Cl:] == 0).all()), what + ': padding channels'


def test_rows_bn_finalize(C):
    """sum_partial_rows<2> through clamd_bn_finalize over the row counts; clamd_bn_finalize_total gives the same bits."""
    g = _gen(2)
    for cp, Cl, nrows in [(32, 27, n) for n in _nrows_list(2)] + [(2048, 2043, 4 * 64 + 1)]:
        rows, tot = _int_rows(nrows, 2, cp, mul=(1, 8))
        count = 2 * nrows
        gamma, beta = torch.randn(Cl, generator=g, device=DEV), torch.randn(Cl, generator=g, device=DEV)
        rm0, rv0 = torch.randn(Cl, generator=g, device=DEV), torch.rand(Cl, generator=g, device=DEV) + 0.5
        what = f'bn_finalize Cp{cp} C{Cl} nrows {nrows}'
        o = _finalize_fwd(C, what, rows, nrows, cp, Cl, count, gamma, beta, rm0, rv0, False)
        _check_fwd(what, o, _ref_bn_finalize(tot[0], tot[1], count, _np(gamma), _np(beta), _np(rm0).astype(np.float64), _np(rv0).astype(np.float64),
                                            0.1, 1e-5, Cl), cp, Cl)
        t = _finalize_fwd(C, what + ' (_total)', rows, nrows, cp, Cl, count, gamma, beta, rm0, rv0, True)
        for k in o:
            assert torch.equal(_raw(o[k].buf), _raw(t[k].buf)), f'{what}: _total differs in {k}'


def test_finalize_special_channels(C):
    """A low-variance channel (mean 1000, variance 1e-4: sum x^2 = count (1e6 + 1e-4) held exactly by two fp32 rows), count == 1, C < Cp."""
    cp, Cl, count = 32, 20, 20000
    rows, tot = _int_rows(3, 2, cp, mul=(1, 8))
    big = float(np.float32(2e10))                                               # a multiple of 2048: exact in fp32
    assert big == int(big) and 0 <= 20000 * 1000000 + 2 - int(big) < 2 ** 24
    rows.view[:, :, 0] = torch.tensor([[1.6e7, big], [4e6, float(20000 * 1000000 + 2 - int(big))], [0.0, 0.0]], device=DEV)
    tot = _np(rows.view.double().sum(0)).astype(np.int64)
    assert tot[0, 0] == 1000 * count and tot[1, 0] == count * 1000000 + 2
    g = _gen(3)
    gamma, beta = torch.randn(Cl, generator=g, device=DEV), torch.randn(Cl, generator=g, device=DEV)
    rm0, rv0 = torch.randn(Cl, generator=g, device=DEV), torch.rand(Cl, generator=g, device=DEV) + 0.5
    args = (_np(gamma), _np(beta), _np(rm0).astype(np.float64), _np(rv0).astype(np.float64), 0.1, 1e-5, Cl)
    o = _finalize_fwd(C, 'bn_finalize low variance', rows, 3, cp, Cl, count, gamma, beta, rm0, rv0, False)
    ref = _ref_bn_finalize(tot[0], tot[1], count, *args)
    assert abs(ref['save_istd'][0][0] - 1 / math.sqrt(1e-4 + 1e-5)) < 1e-6 * ref['save_istd'][0][0]
    _check_fwd('bn_finalize low variance', o, ref, cp, Cl)
    # count == 1: one pixel x per channel, sum x^2 = x^2: variance 0, running_var takes the biased value
    x = 1 + torch.arange(cp, device=DEV) % 7
    rows1, _ = _int_rows(1, 2, cp)
    rows1.view[0, 0], rows1.view[0, 1] = x.float(), (x * x).float()
    o = _finalize_fwd(C, 'bn_finalize count 1', rows1, 1, cp, Cl, 1, gamma, beta, rm0, rv0, False)
    _check_fwd('bn_finalize count 1', o, _ref_bn_finalize(_np(x).astype(np.int64), _np(x * x).astype(np.int64), 1, *args), cp, Cl)


@pytest.mark.parametrize('with_bias', [True, False])
def test_rows_bn_bwd_finalize(C, with_bias):
    """sum_partial_rows<5> through clamd_bn_bwd_finalize; clamd_bn_rows_total + clamd_bn_bwd_finalize_total give the same bits."""
    L, s = C._lib, C._lib.stream_ptr()
    g = _gen(4)
    for cp, Cl, nrows in [(32, 27, n) for n in _nrows_list(5)] + [(2048, 2043, 4 * 25 + 1)]:
        rows, tot = _int_rows(nrows, 5, cp)
        count = float(4 * nrows)
        gamma, mu = torch.randn(Cl, generator=g, device=DEV), torch.randn(cp, generator=g, device=DEV)
        istd = torch.rand(cp, generator=g, device=DEV) + 0.5
        what = f'bn_bwd_finalize Cp{cp} C{Cl} nrows {nrows} dbias {with_bias}'

        def launch(total):
            k012, dg, db, dbias = Rows(3, cp), Rows(Cl), Rows(Cl), Rows(Cl)
            bp = dbias.ptr if with_bias else None
            if total:
                totals, red = Rows(5, cp, dtype=torch.float64), Rows(1, 2 * cp + 1, dtype=torch.float64)
                L.call('clamd_bn_rows_total', rows.ptr, nrows, 5, cp, count, totals.ptr, red.ptr, s)
                L.call('clamd_bn_bwd_finalize_total', totals.ptr, red.ptr, L.ptr(gamma), L.ptr(mu), L.ptr(istd), k012.ptr, dg.ptr, db.ptr, bp, cp, Cl, s)
            else:
                L.call('clamd_bn_bwd_finalize', rows.ptr, nrows, L.ptr(gamma), L.ptr(mu), L.ptr(istd), k012.ptr, dg.ptr, db.ptr, bp, cp, Cl, count, s)
            _sync()
            return [k012, dg, db, dbias]

        k012, dg, db, dbias = _twice(what, lambda: launch(False))
        ref = _ref_bn_bwd_finalize(tot, tot[0].astype(np.float64), tot[1].astype(np.float64), count, _np(gamma), _np(mu), _np(istd), Cl, with_bias)
        got = {'k0': k012.view[0], 'k1': k012.view[1], 'k2': k012.view[2], 'dgamma': dg.view, 'dbeta': db.view, 'dbias': dbias.view}
        for k, (val, bound) in ref.items():
            _check_vec(f'{what} {k}', ('bn_bwd_finalize', k), _np(got[k]), val, bound)
        assert bool((k012.view[:, Cl:] == 0).all()), what + ': k012 of the padding channels'
        assert with_bias or bool(torch.isnan(dbias.view).all()), what + ': dbias written without being asked for'
        for a, b in zip((k012, dg, db, dbias), _twice(what + ' (_total)', lambda: launch(True))):
            assert torch.equal(_raw(a.buf), _raw(b.buf)), what + ': _total differs'


@pytest.mark.parametrize('nk', [3, 5])
def test_rows_bn_bwd_eval_finalize(C, nk):
    """sum_partial_rows<3|5> through clamd_bn_bwd_eval_finalize: dgamma = istd (s1 - mu s0), dbeta = s0, dbias = s2 (3) | scale s2 (5)."""
    L, s = C._lib, C._lib.stream_ptr()
    g = _gen(5)
    for cp, Cl, nrows in [(32, 27, n) for n in _nrows_list(nk)] + [(2048, 2043, 4 * RL[nk] + 1)]:
        rows, tot = _int_rows(nrows, nk, cp)
        sc, mu = torch.randn(cp, generator=g, device=DEV), torch.randn(cp, generator=g, device=DEV)
        istd = torch.rand(cp, generator=g, device=DEV) + 0.5
        what = f'bn_bwd_eval_finalize<{nk}> Cp{cp} C{Cl} nrows {nrows}'
        for with_k, with_bias in ((True, True), (False, False)):

            def launch():
                k012, dg, db, dbias = Rows(3, cp), Rows(Cl), Rows(Cl), Rows(Cl)
                L.call('clamd_bn_bwd_eval_finalize', rows.ptr, nrows, nk, L.ptr(sc), L.ptr(mu), L.ptr(istd), k012.ptr if with_k else None, dg.ptr,
                       db.ptr, dbias.ptr if with_bias else None, cp, Cl, s)
                _sync()
                return [k012, dg, db, dbias]

            k012, dg, db, dbias = _twice(what, launch)
            t = tot.astype(np.float64)
            m, i, scd = _np(mu).astype(np.float64), _np(istd).astype(np.float64), _np(sc).astype(np.float64)
            val = (i * (t[1] - m * t[0]))[:Cl]
            _check_vec(what + ' dgamma', ('bn_bwd_eval_finalize', 'dgamma'), _np(dg.view), val,
                       _ulp32(val) + (2.0 ** -50 * i * (np.abs(t[1]) + np.abs(m * t[0])))[:Cl])
            assert np.array_equal(_np(db.view).astype(np.float64), t[0][:Cl]), what + ': dbeta'
            if with_bias:
                val = (t[2] if nk == 3 else scd * t[2])[:Cl]
                _check_vec(what + ' dbias', ('bn_bwd_eval_finalize', 'dbias'), _np(dbias.view), val, _ulp32(val) if nk == 5 else 0 * val)
            else:
                assert bool(torch.isnan(dbias.view).all())
            if with_k:
                want = torch.zeros(3, cp, device=DEV)
                want[0, :Cl] = sc[:Cl]
                assert torch.equal(k012.view, want), what + ': k012 = (scale [c < C], 0, 0)'
            else:
                assert bool(torch.isnan(k012.view).all())
