"""GPU: the pointwise / ConvTranspose2d instantiations of igemm_kernel (csrc/igemm.hip) and the boundary layout kernels
(csrc/elementwise.hip), per element, over the grid their launchers can start.

Every case calls the C ABI directly.  Every output sits in a poisoned buffer (Act / ActAt / Rows: guard bands in front and behind, the pitch
gap or the other half of a concat neighbour, extra rows behind the statistics rows and behind the last class plane) that must come back
bit-identical outside the written region; every launch runs twice and must give the same bits.  References are float64 torch evaluations of
include/clamd.h's formulas on the same inputs (one contraction over channels, and copies), never another call into libclamd.so.  Packed
operands are written here from the layouts the header documents -- [Cout_p][Cin_p] (1x1), [4][Cout_p][Cin_p] (ConvTranspose2d forward, tap
q = 2 dy + dx), [Cin_p][4][Cout_p] (its data gradient), bf16x3 through ops.split_encode on the innermost dimension -- and one case per
entry point (test_*_exact) also packs through ops.PackTable and asserts the same bits; that case has power-of-two Kp and Np, because
PackTable pads logical channel counts with ops.cpad, to a power of two, and so cannot produce Kp = 96.  Inputs come from numpy generators
on the host, so the references alone can be evaluated without a GPU (test_argmax_random's decidability was checked that way).

Exact-integer cases (activations in [-4, 4], weights in {-2 .. 2}, integer bias, about a quarter zeros): every product and partial sum is an
integer far below 2^24, exact in fp32 in any order, so the output EQUALS storage(exact result) bit for bit (float64 holds every such
integer: the float64 contraction is the integer result, taken to int64 for the sums); padded channels are +0 in all bits; statistics and
five-sum rows, per tile and in total, equal the int64 reference taken on the fp32 value before storage (every per-channel sum of absolute
terms is asserted below 2^24 from the reference); the row count equals clamd_stat_rows().  Five sums in clamd_bn_bwd_reduce's order:
sum g, sum g y, sum g [y > 0], sum [y > 0], sum y, with g this launch's result and y = bn_y.

Random-valued cases (normal values rounded to what the storage holds; bf16x3 with a live lo plane), bound per element, derived:
  accumulation   n u (sum_k |a_k w_k| + |bias|), n the number of additions: Kp + 1 (fp32, bf16), 3 Kp + 1 (bf16x3: hi hi + hi lo + lo hi
                 per channel), u = UNIT[(entry point, dtype)], EPS = 2^-24 unless a kernel whose exact cases pass exceeds it (then one
                 ulp, 2^-23, which also covers a truncating adder); + 2^-50 of the same sum for the float64 reference's own roundings
  bf16x3         the kernel drops lo_a lo_w.  The inputs keep |lo| <= 2^-9 |x| (asserted; where rne leaves a larger lo -- it can reach
                 2^-8 |x| at the bottom of a binade -- the generator clears it), so |lo_a lo_w| <= 2^-18 |a w|: + 2^-18 sum_k |a_k w_k|
  storage        + STORE_REL[dtype] (|ref| + the above); the fp32 NCHW logits have none
  statistics     as test_bn_grid_gpu.py bounds its random sums: the per-element bounds of the fp32 values added up, + n EPS sum |terms|,
                 n the pixels per channel; for v^2 and g y the propagated 2 |v| e + e^2 and |y| e
Worst error / bound seen on the MI355X (exact cases: equality).  No pair exceeds 1 with u = 2^-24, so UNIT is empty; bf16 outputs sit just
under 1 because the half-ulp storage term is sharp.
                                                          fp32                    bf16                    bf16x3
  conv1x1 output / statistics rows / five-sum rows        0.104 / 0.002 / 0.002   0.987 / 0.003 / 0.001   0.275 / 0.004 / 0.006
  conv1x1_logits, conv1x1_argmax (fp32 logits)            0.127, 0.091            0.056, 0.045            0.227, 0.156
  convT2x2_fwd output                                     0.117                   0.993                   0.293
  convT2x2_dgrad output / five-sum rows                   0.033 / 0.001           0.989 / 0.000           0.119 / 0.001

Kernels, instantiations (T = float | bf16_t | split_t looped by every test) and the case that reaches each path.  Shapes: S16 = 2 x 17 x 18
(TW 16, TH 16: ragged in both directions, W % 4 != 0, two images), S32a = 1 x 9 x 36 (TW 32, TH 8: W % 4 == 0, a partial tile in x and y),
S32b = 2 x 8 x 33 (TW 32: scalar logits stores).  x2 / y2: the operand is the second half of a buffer of twice the pitch.
  igemm_kernel<T, MODE_PW, EPI_NHWC, 16|32, 0>   test_conv1x1_exact / _random, CONV1X1 rows: S16 Kp 32 Np 32 bias relu stats (bf16: the second
                                                 slab of the only K-step past the end; Np 32: the n < Np guards; vmask: bias on a ragged tile)
                                                 | S32a Kp 64 x2 Np 64 y2 bn_y + bn_sums | S32b Kp 96 (bf16: the last K-step's second slab past the
                                                 end) Np 128 (two slabs) bias stats | S16 Kp 128 x2 Np 128 y2 bias relu | S32a Kp 32 x2 Np 32 y2
                                                 bias bn_y + bn_sums | S32b Kp 64 Np 64 relu stats
  igemm_kernel<T, MODE_PW, EPI_UP2, 16|32, 0>    test_convT_fwd_exact / _random, CONVT rows: S16 Kp 32 Cout_p 32 bias | S32a Kp 64 x2 Cout_p 64 y2 |
                                                 S32b Kp 96 Cout_p 32 y2 bias | S32a Kp 128 x2 Cout_p 64 bias (Np = 4 Cout_p = 128, 256: a tap's
                                                 channels span slabs at Cout_p 32)
  igemm_kernel<T, MODE_UP2, EPI_NHWC, 16|32, 0>  test_convT_dgrad_exact / _random, DGRAD rows: S16 Cout_p 32 Cin_p 32 | S32a Cout_p 64 x2 Cin_p 128 y2
                                                 bn_y + bn_sums | S32b Cout_p 32 x2 Cin_p 128 bn_y + bn_sums | S16 Cout_p 64 Cin_p 32 y2 bn_y +
                                                 bn_sums (half a slab: the n0 + c < Np guard of the five-sum rows)
  igemm_kernel<T, MODE_PW, EPI_NCHW, 16|32, 0>   test_logits_exact / _random, HEAD rows: num_classes 1 (S16 Kp 32), 2 (S32a Kp 64 x2, no bias), 21
                                                 (S32b Kp 96), 32 (S16 Kp 128 x2), 33 (S32a Kp 32: float4 stores with a partial tile in x), 64
                                                 (S32b Kp 64 x2, no bias: scalar stores), 21 and 100 of Cout_p 128 (two slabs, S32a).
                                                 test_argmax_exact: the same rows up to 64 classes, pred against the first maximum of the
                                                 float64 logits, with logits_nchw NULL and non-NULL (the same pred bits).  test_argmax_ties:
                                                 all classes equal | a class < 32 and a class >= 32 (the v1 > v0 step) | two lanes that meet at
                                                 butterfly distance 16, 8, 4, 2, 1 | the maximum in the last logical class under larger padded
                                                 rows.  test_argmax_random: pred where the reference's top two differ by more than their bounds
                                                 (undecidable share asserted 0).  test_argmax_two_slabs: Cout_p 128 is refused, status -1, pred
                                                 untouched
  nchw_to_nhwc4_kernel<T, 32> / nchw_to_nhwc_kernel<T>   test_nchw_to_nhwc: C 1, 5, 21, 32 of Cp 32 and C 40 of Cp 64; ldc Cp and 2 Cp; mul 1 and
                                                 0.37; 2 x 6 x 10 (H W % 4 == 0) and 2 x 5 x 7; the source at a 16-byte boundary (Cp 32, H W % 4 == 0:
                                                 the four-pixel kernel) and 4 bytes past one (the generic kernel), the two results bit-identical
  nhwc_to_nchw_kernel<T>                         test_nhwc_to_nchw: C 21 of Cp 32 at pitch 64, C 40 of Cp 64 at pitch 128, bf16x3 with a live lo;
                                                 test_nhwc_to_nchw_second_trip: 1 x 230 x 230, C 40: 2116000 > 2097152 elements, a partial second trip
  nchw_im2col3p_kernel<T>                        test_im2col3: fp32 / bf16x3 at C 1 and 3; bf16 at 2 x 6 x 7 (W % 4 != 0) and from a misaligned source
  nchw_im2col3x4_kernel<T>                       test_im2col3: bf16, aligned, 1 x 5 x 12 (15 quads: a partial wave) and 3 x 10 x 36 (270 quads: a partial
                                                 second workgroup, image boundaries inside a wave), ldc 32 (LDS exchange) and 64 (plain stores)
  nchw_im2col3_kernel<T>                         test_im2col3: C 5 and C 2 of Cp 64, ldc 64 and 128
Grid-stride loops left with their first trip only, because a second one needs more than 64 MB of tensors (grids of 256 threads, capped at
8192 workgroups, 16384 for the piece kernel): nchw_to_nhwc_kernel and nchw_im2col3_kernel, one pixel per thread, from 2097152 pixels on
(Cp >= 32 channels each: 268 MB of fp32, 134 MB of bf16); nchw_to_nhwc4_kernel and nchw_im2col3x4_kernel, four pixels per thread, from
8388608 pixels on; nchw_im2col3p_kernel, four threads per pixel, from 1048576 pixels on (67 MB of bf16 output, 134 MB otherwise, plus the
source).  nhwc_to_nchw_kernel's grid runs over B C H W elements, so its second trip starts at 2097152 elements and is run.
"""
import numpy as np
import pytest
import torch

from grid_util import (DEV, EPS, POISON, STORE_REL, Act, ActAt, Rows, _dev, _expect_bits, _expect_rows, _half, _ints, _normal, _operand, _pad2,
                       _per_element, _raw, _twice)

pytestmark = pytest.mark.gpu

DT = [('fp32', 0), ('bf16', 1), ('bf16x3', 2)]
UNIT = {}                                      # (entry point, dtype code) -> u of the accumulation bound where EPS is exceeded (see above)
S16, S32A, S32B = (2, 17, 18), (1, 9, 36), (2, 8, 33)


@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    C._lib.load()
    return C


def _sync():
    torch.cuda.synchronize()


def _weights(rng, shape, dcode, exact):
    return _ints(rng, shape, 2, 0.07) if exact else _normal(rng, shape, dcode, zeros=0.1)


def _acts(rng, shape, dcode, exact):
    return _ints(rng, shape, 4, 0.15) if exact else _normal(rng, shape, dcode)


# --------------------------------------------------------------------------------------------------------------------------- references
def _tiles(B, H, W):
    """Pixel -> tile index of igemm_kernel (TW x TH = 32 x 8 for W >= 32, else 16 x 16), and the tile count = statistics rows."""
    TW = 32 if W >= 32 else 16
    TH = 256 // TW
    tx, ty = -(-W // TW), -(-H // TH)
    b, y, x = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), indexing='ij')
    return ((b * ty + y // TH) * tx + x // TW).reshape(-1).to(DEV), B * tx * ty


def _contract(A, Wm, bias):
    """A [M, K], Wm [N, K], bias [N] | None (fp32 values) -> float64 A Wm^T + bias and the sum of the absolute terms."""
    Ad, Wd = A.double(), Wm.double()
    ref, mag = Ad @ Wd.T, Ad.abs() @ Wd.abs().T
    prod = mag.clone()
    if bias is not None:
        ref, mag = ref + bias.double(), mag + bias.double().abs()
    return ref, mag, prod


def _acc_bound(entry, dcode, K, mag, prod):
    """The bound of the fp32 accumulator value against the float64 contraction (module docstring)."""
    n = (3 if dcode == 2 else 1) * K + 1
    return n * UNIT.get((entry, dcode), EPS) * mag + 2.0 ** -50 * mag + (2.0 ** -18 * prod if dcode == 2 else 0.0)


def _per_tile(ids, nt, v):
    return torch.zeros(nt, v.shape[1], dtype=v.dtype, device=DEV).index_add_(0, ids, v)


def _check_out(what, entry, dcode, exact, out, ref, mag, prod, K, logical_n):
    """The NHWC output of a launch against the float64 result `ref` [npix, Np] -> the per-element bound of the fp32 value before storage."""
    if exact:
        assert float(mag.max()) < 2 ** 24
        _expect_bits(what + ' output', out, ref.float())
        assert bool(out.zero_bits()[:, logical_n:].all()), what + ': padded channels are not +0'
        return torch.zeros_like(ref)
    e = _acc_bound(entry, dcode, K, mag, prod)
    _per_element(what + ' output', (entry, dcode), out.get(), ref, e + STORE_REL[dcode] * (ref.abs() + e))
    assert bool(out.zero_bits()[:, logical_n:].all()), what + ': padded channels are not +0'
    return e


def _check_sums(what, entry, dcode, exact, rows, ids, nt, terms, errs):
    """rows [nt][nk][Np] against the float64 per-pixel `terms` [nk][npix, Np]: exact -> per tile and in total EQUAL the int64 sums; else the
    totals within sum(errs) + npix EPS sum |terms| (errs: the propagated per-element bounds of the terms)."""
    npix = terms[0].shape[0]
    if exact:
        for t in terms:
            assert float(t.abs().sum(0).max()) < 2 ** 24, what + ': a per-channel sum of absolute terms reaches 2^24'
        exp = torch.stack([_per_tile(ids, nt, t.to(torch.int64)) for t in terms], 1)
        _expect_rows(what + ' rows per tile', rows, exp.float())
        bad = (rows.view.double().sum(0).to(torch.int64) != exp.sum(0)).nonzero()
        assert bad.numel() == 0, f'{what}: totals differ from the int64 reference at (sum, channel) {bad[:4].tolist()}'
        return
    tot = rows.view.double().sum(0)
    ref = torch.stack([t.sum(0) for t in terms])
    bound = torch.stack([e.sum(0) + (npix + 1) * EPS * (t.abs() + e).sum(0) for t, e in zip(terms, errs)])
    _per_element(what + ' rows', (entry + ' rows', dcode), tot, ref, bound)


def _stat_terms(v, e):
    return [v, v * v], [e, 2 * v.abs() * e + e * e]


def _five_terms(g, e, y):
    yd, pos, z = y.double(), (y > 0).double(), torch.zeros_like(g)
    return [g, g * yd, g * pos, pos.expand_as(g).clone(), yd.expand_as(g).clone()], [e, e * yd.abs(), e * pos, z, z]


# ------------------------------------------------------------------------------------------------------------------ clamd_conv1x1
#         shape  Kp   x  Np   y  bias   relu mode
CONV1X1 = [(S16, 32, 1, 32, 1, True, 1, 'stats'),
           (S32A, 64, 2, 64, 2, False, 0, 'bn'),
           (S32B, 96, 1, 128, 1, True, 0, 'stats'),
           (S16, 128, 2, 128, 2, True, 1, ''),
           (S32A, 32, 2, 32, 2, True, 0, 'bn'),
           (S32B, 64, 1, 64, 1, False, 1, 'stats')]


def _pack_check(C, what, dcode, kind, w_logical, wf, wd):
    """ops.PackTable's output for the same logical weights has the bits of the hand-written operands."""
    T = C.ops.TORCH_DT[dcode]
    pf, pd = (torch.full((t.numel(),), POISON, dtype=T, device=DEV) if t is not None else None for t in (wf, wd))
    tab = C.ops.PackTable(dcode)
    if kind == 'head':
        tab.head(w_logical, pf, None, w_logical.shape[1], w_logical.shape[0])
    else:
        tab.convT(w_logical, pf, pd, w_logical.shape[0], w_logical.shape[1])
    tab.finalize(DEV).run(dcode)
    _sync()
    for name, p, h in (('forward', pf, wf), ('data-gradient', pd, wd)):
        if h is not None:
            assert torch.equal(_raw(p), _raw(h.reshape(-1))), f'{what}: clamd_pack and the documented {name} layout differ'


def _conv1x1_case(C, what, dcode, exact, shape, Kp, xm, Np, ym, with_bias, relu, mode, seed, via_pack=False):
    L, s = C._lib, C._lib.stream_ptr()
    (B, H, W), rng = shape, np.random.default_rng(seed)
    npix, Kl, Nl = B * H * W, Kp - 3, Np - 5
    x = torch.zeros(npix, Kp, device=DEV)
    x[:, :Kl] = _acts(rng, (npix, Kl), dcode, exact)
    wl = _weights(rng, (Nl, Kl), dcode, exact)                                    # the parameter [Cout][Cin] (1 x 1)
    wp = _pad2(wl, Np, Kp)                                                        # [Cout_p][Cin_p]
    bias = torch.zeros(Np, device=DEV)
    bias[:Nl] = _ints(rng, (Nl,), 3, 0.0) if exact else _normal(rng, (Nl,), 0, zeros=0.0)
    y = _ints(rng, (npix, Np), 4, 0.15) if exact else _normal(rng, (npix, Np), dcode)     # bn_y
    xa, wdev = _half(C, npix, Kp, xm, dcode, x), _operand(C, wp, dcode)
    if via_pack:
        _pack_check(C, what, dcode, 'head', wl.view(Nl, Kl, 1, 1).contiguous(), wdev, None)
    ya = Act(C, npix, Np, Np, dcode, y) if mode == 'bn' else None
    ids, nt = _tiles(B, H, W)
    nrows = L.stat_rows(L.OP_CONV1X1, B, H, W, Kp, Np, dcode, mode == 'bn')
    assert nrows == nt, (what, nrows, nt)

    def launch():
        out = _half(C, npix, Np, ym, dcode)
        st, bn = Rows(nt, 2, Np) if mode == 'stats' else None, Rows(nt, 5, Np) if mode == 'bn' else None
        L.call('clamd_conv1x1', xa.ptr, xa.ldc, L.ptr(wdev), L.ptr(bias) if with_bias else None, out.ptr, out.ldc, st.ptr if st else None,
               ya.ptr if ya else None, bn.ptr if bn else None, nt if mode else 0, B, H, W, Kp, Np, relu, dcode, s)
        _sync()
        return [out] + [r for r in (st, bn) if r]

    outs = _twice(what, launch)
    ref, mag, prod = _contract(x, wp, bias if with_bias else None)
    if relu:
        ref = ref.clamp_min(0.0)
    e = _check_out(what, 'conv1x1', dcode, exact, outs[0], ref, mag, prod, Kp, Nl)
    if mode == 'stats':
        _check_sums(what, 'conv1x1', dcode, exact, outs[1], ids, nt, *_stat_terms(ref, e))
    elif mode == 'bn':
        _check_sums(what, 'conv1x1 five sums', dcode, exact, outs[1], ids, nt, *_five_terms(ref, e, y))


@pytest.mark.parametrize('name,dcode', DT)
def test_conv1x1_exact(C, name, dcode):
    for i, row in enumerate(CONV1X1):
        _conv1x1_case(C, f'conv1x1 {name} exact {row}', dcode, True, *row, seed=100 + i, via_pack=i == 1)


@pytest.mark.parametrize('name,dcode', DT)
def test_conv1x1_random(C, name, dcode):
    for i, row in enumerate(CONV1X1):
        _conv1x1_case(C, f'conv1x1 {name} random {row}', dcode, False, *row, seed=200 + i)


# ------------------------------------------------------------------------------------- clamd_convT2x2_fwd / clamd_convT2x2_dgrad
#        shape  Kp  x  Cout_p y bias
CONVT = [(S16, 32, 1, 32, 1, True),
         (S32A, 64, 2, 64, 2, False),
         (S32B, 96, 1, 32, 2, True),
         (S32A, 128, 2, 64, 1, True)]
#        shape Cout_p x Cin_p y  bn
DGRAD = [(S16, 32, 1, 32, 1, False),
         (S32A, 64, 2, 128, 2, True),
         (S32B, 32, 2, 128, 1, True),
         (S16, 64, 1, 32, 2, True)]


def _convT_weights(rng, cin_p, cout_p, dcode, exact):
    """The parameter [Cin][Cout][2][2] (logical sizes 3 and 5 short of the padded ones) and its two documented packings as fp32:
    [4][Cout_p][Cin_p] with tap q = 2 dy + dx, and [Cin_p][4][Cout_p]."""
    cin, cout = cin_p - 3, cout_p - 5
    wl = _weights(rng, (cin, cout, 2, 2), dcode, exact)
    wf = torch.zeros(4, cout_p, cin_p, device=DEV)
    wf[:, :cout, :cin] = wl.permute(2, 3, 1, 0).reshape(4, cout, cin)
    wd = torch.zeros(cin_p, 4, cout_p, device=DEV)
    wd[:cin, :, :cout] = wl.permute(0, 2, 3, 1).reshape(cin, 4, cout)
    return wl, wf, wd


def _to_windows(t, B, h, w):
    """[B 2h 2w, c] -> [B h w, 4 c], column q c + i = the pixel (2 y + dy, 2 x + dx), q = 2 dy + dx."""
    c = t.shape[-1]
    return t.view(B, h, 2, w, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(B * h * w, 4 * c)


def _from_windows(t, B, h, w):
    c = t.shape[-1] // 4
    return t.view(B, h, w, 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(B * 4 * h * w, c)


def _convT_fwd_case(C, what, dcode, exact, shape, Kp, xm, Cp, ym, with_bias, seed, via_pack=False):
    L, s = C._lib, C._lib.stream_ptr()
    (B, h, w), rng = shape, np.random.default_rng(seed)
    npix, cin, cout = B * h * w, Kp - 3, Cp - 5
    x = torch.zeros(npix, Kp, device=DEV)
    x[:, :cin] = _acts(rng, (npix, cin), dcode, exact)
    wl, wf, wd = _convT_weights(rng, Kp, Cp, dcode, exact)
    bias = torch.zeros(Cp, device=DEV)
    bias[:cout] = _ints(rng, (cout,), 3, 0.0) if exact else _normal(rng, (cout,), 0, zeros=0.0)
    xa, wdev = _half(C, npix, Kp, xm, dcode, x), _operand(C, wf, dcode)
    if via_pack:
        _pack_check(C, what, dcode, 'convT', wl, wdev, _operand(C, wd, dcode))

    def launch():
        out = _half(C, 4 * npix, Cp, ym, dcode)
        L.call('clamd_convT2x2_fwd', xa.ptr, xa.ldc, L.ptr(wdev), L.ptr(bias) if with_bias else None, out.ptr, out.ldc, B, h, w, Kp, Cp, dcode, s)
        _sync()
        return [out]

    out, = _twice(what, launch)
    ref, mag, prod = _contract(x, wf.reshape(4 * Cp, Kp), bias.repeat(4) if with_bias else None)
    ref, mag, prod = (_from_windows(t, B, h, w) for t in (ref, mag, prod))
    _check_out(what, 'convT2x2_fwd', dcode, exact, out, ref, mag, prod, Kp, cout)


def _convT_dgrad_case(C, what, dcode, exact, shape, Cp, xm, Np, ym, bn, seed, via_pack=False):
    """gy [B, 2h, 2w, Cout_p = Cp] -> gx [B, h, w, Cin_p = Np]."""
    L, s = C._lib, C._lib.stream_ptr()
    (B, h, w), rng = shape, np.random.default_rng(seed)
    npix, cin, cout = B * h * w, Np - 3, Cp - 5
    gy = torch.zeros(4 * npix, Cp, device=DEV)
    gy[:, :cout] = _acts(rng, (4 * npix, cout), dcode, exact)
    wl, wf, wd = _convT_weights(rng, Np, Cp, dcode, exact)
    y = _ints(rng, (npix, Np), 4, 0.15) if exact else _normal(rng, (npix, Np), dcode)
    ga, wdev = _half(C, 4 * npix, Cp, xm, dcode, gy), _operand(C, wd, dcode)
    if via_pack:
        _pack_check(C, what, dcode, 'convT', wl, _operand(C, wf, dcode), wdev)
    ya = Act(C, npix, Np, Np, dcode, y) if bn else None
    ids, nt = _tiles(B, h, w)
    assert L.stat_rows(L.OP_CONVT2X2_DGRAD, B, h, w, Np, Cp, dcode, bn) == nt

    def launch():
        out, rows = _half(C, npix, Np, ym, dcode), Rows(nt, 5, Np) if bn else None
        L.call('clamd_convT2x2_dgrad', ga.ptr, ga.ldc, L.ptr(wdev), out.ptr, out.ldc, ya.ptr if bn else None, rows.ptr if bn else None,
               nt if bn else 0, B, h, w, Np, Cp, dcode, s)
        _sync()
        return [out, rows] if bn else [out]

    outs = _twice(what, launch)
    ref, mag, prod = _contract(_to_windows(gy, B, h, w), wd.reshape(Np, 4 * Cp), None)
    e = _check_out(what, 'convT2x2_dgrad', dcode, exact, outs[0], ref, mag, prod, 4 * Cp, cin)
    if bn:
        _check_sums(what, 'convT2x2_dgrad five sums', dcode, exact, outs[1], ids, nt, *_five_terms(ref, e, y))


@pytest.mark.parametrize('name,dcode', DT)
def test_convT_fwd_exact(C, name, dcode):
    for i, row in enumerate(CONVT):
        _convT_fwd_case(C, f'convT2x2_fwd {name} exact {row}', dcode, True, *row, seed=300 + i, via_pack=i == 1)


@pytest.mark.parametrize('name,dcode', DT)
def test_convT_fwd_random(C, name, dcode):
    for i, row in enumerate(CONVT):
        _convT_fwd_case(C, f'convT2x2_fwd {name} random {row}', dcode, False, *row, seed=400 + i)


@pytest.mark.parametrize('name,dcode', DT)
def test_convT_dgrad_exact(C, name, dcode):
    for i, row in enumerate(DGRAD):
        _convT_dgrad_case(C, f'convT2x2_dgrad {name} exact {row}', dcode, True, *row, seed=500 + i, via_pack=i == 1)


@pytest.mark.parametrize('name,dcode', DT)
def test_convT_dgrad_random(C, name, dcode):
    for i, row in enumerate(DGRAD):
        _convT_dgrad_case(C, f'convT2x2_dgrad {name} random {row}', dcode, False, *row, seed=600 + i)


# ------------------------------------------------------------------------------------- clamd_conv1x1_logits / clamd_conv1x1_argmax
#       shape  Kp   x  Cout_p classes bias
HEAD = [(S16, 32, 1, 32, 1, True),
        (S32A, 64, 2, 32, 2, False),
        (S32B, 96, 1, 32, 21, True),
        (S16, 128, 2, 32, 32, True),
        (S32A, 32, 1, 64, 33, True),
        (S32B, 64, 2, 64, 64, False)]
HEAD_WIDE = [(S32A, 64, 1, 128, 21, True), (S32A, 32, 2, 128, 100, True)]          # two 64-channel slabs: clamd_conv1x1_logits only


def _head_inputs(rng, dcode, exact, npix, Kp, Np, K, padded_rows=False):
    """x [npix, Kp], the operand [Cout_p][Cin_p] with `K` class rows (padded_rows: the rows behind them hold weights too, which the header
    does not promise to be zero for this entry point's arg-max: they must not win), bias [Cout_p]."""
    Kl = Kp - 3
    x = torch.zeros(npix, Kp, device=DEV)
    x[:, :Kl] = _acts(rng, (npix, Kl), dcode, exact)
    nrow = Np if padded_rows else K
    wp = _pad2(_weights(rng, (nrow, Kl), dcode, exact), Np, Kp)
    bias = torch.zeros(Np, device=DEV)
    bias[:nrow] = _ints(rng, (nrow,), 3, 0.0) if exact else _normal(rng, (nrow,), 0, zeros=0.0)
    return x, wp, bias


def _nchw(t, B, K):
    """[B H W, Np] -> [B K, H W]."""
    return t.view(B, -1, t.shape[-1])[:, :, :K].permute(0, 2, 1).reshape(B * K, -1).contiguous()


def _first_max(logits, K):
    """[npix, Np] float64 -> int64 [npix]: the first maximum over classes 0 .. K - 1."""
    lg = logits[:, :K]
    idx = torch.arange(K, device=lg.device).expand_as(lg)
    return torch.where(lg == lg.max(1, keepdim=True).values, idx, torch.full_like(idx, K)).min(1).values


def _head_launch(C, what, dcode, shape, Kp, xm, Np, K, x, wp, bias, with_pred, with_logits):
    """clamd_conv1x1_logits (with_pred False) or clamd_conv1x1_argmax, twice -> (logits Rows [B K, H W] | None, pred Rows [B, H W] | None)."""
    L, s = C._lib, C._lib.stream_ptr()
    B, H, W = shape
    npix = B * H * W
    xa, wdev = _half(C, npix, Kp, xm, dcode, x), _operand(C, wp, dcode)
    bp = L.ptr(bias) if bias is not None else None

    def launch():
        lg = Rows(B * K, H * W) if with_logits else None
        pr = Rows(B, H * W, fill=-1, dtype=torch.int64) if with_pred else None
        if with_pred:
            L.call('clamd_conv1x1_argmax', xa.ptr, xa.ldc, L.ptr(wdev), bp, pr.ptr, lg.ptr if lg else None, B, H, W, Kp, Np, K, dcode, s)
        else:
            L.call('clamd_conv1x1_logits', xa.ptr, xa.ldc, L.ptr(wdev), bp, lg.ptr, B, H, W, Kp, Np, K, dcode, s)
        _sync()
        return [r for r in (lg, pr) if r]

    w_before = wdev.clone()
    outs = _twice(what, launch)
    assert xa.guards_intact() and torch.equal(_raw(xa.buf), _raw(xa.before)), what + ': the input was written'
    assert torch.equal(_raw(wdev), _raw(w_before)), what + ': the operand was written'
    return outs[0] if with_logits else None, outs[-1] if with_pred else None


def _check_logits(what, entry, dcode, exact, lg, ref, mag, prod, B, K, Kp):
    if exact:
        assert float(mag.max()) < 2 ** 24
        _expect_rows(what + ' logits', lg, _nchw(ref, B, K).float())
    else:
        _per_element(what + ' logits', (entry, dcode), lg.view, _nchw(ref, B, K), _nchw(_acc_bound(entry, dcode, Kp, mag, prod), B, K))


def _logits_case(C, what, dcode, exact, shape, Kp, xm, Np, K, with_bias, seed, via_pack=False):
    (B, H, W), rng = shape, np.random.default_rng(seed)
    x, wp, bias = _head_inputs(rng, dcode, exact, B * H * W, Kp, Np, K)
    if via_pack:
        _pack_check(C, what, dcode, 'head', wp[:K, :Kp - 3].reshape(K, Kp - 3, 1, 1).contiguous(), _operand(C, wp, dcode), None)
    lg, _ = _head_launch(C, what, dcode, shape, Kp, xm, Np, K, x, wp, bias if with_bias else None, False, True)
    ref, mag, prod = _contract(x, wp, bias if with_bias else None)
    _check_logits(what, 'conv1x1_logits', dcode, exact, lg, ref, mag, prod, B, K, Kp)


@pytest.mark.parametrize('name,dcode', DT)
def test_logits_exact(C, name, dcode):
    for i, row in enumerate(HEAD + HEAD_WIDE):
        _logits_case(C, f'conv1x1_logits {name} exact {row}', dcode, True, *row, seed=700 + i, via_pack=i == 3)


@pytest.mark.parametrize('name,dcode', DT)
def test_logits_random(C, name, dcode):
    for i, row in enumerate(HEAD + HEAD_WIDE):
        _logits_case(C, f'conv1x1_logits {name} random {row}', dcode, False, *row, seed=800 + i)


def _argmax_case(C, what, dcode, exact, shape, Kp, xm, Np, K, x, wp, bias, via_pack=False):
    """pred with logits_nchw non-NULL and NULL: the same bits; exact: pred == the first maximum of the float64 logits; random values: where
    the reference's top two logits differ by more than their two bounds, and that is every pixel (asserted)."""
    B = shape[0]
    if via_pack:
        _pack_check(C, what, dcode, 'head', wp[:K, :Kp - 3].reshape(K, Kp - 3, 1, 1).contiguous(), _operand(C, wp, dcode), None)
    lg, pred = _head_launch(C, what, dcode, shape, Kp, xm, Np, K, x, wp, bias, True, True)
    _, pred0 = _head_launch(C, what + ', no logits', dcode, shape, Kp, xm, Np, K, x, wp, bias, True, False)
    assert torch.equal(_raw(pred.buf), _raw(pred0.buf)), what + ': pred differs between logits_nchw given and NULL'
    ref, mag, prod = _contract(x, wp, bias)
    _check_logits(what, 'conv1x1_argmax', dcode, exact, lg, ref, mag, prod, B, K, Kp)
    want = _first_max(ref, K)
    if not exact:
        assert _undecidable(ref, _acc_bound('conv1x1_argmax', dcode, Kp, mag, prod), K) == 0, what + ': pixels the reference cannot decide'
    _expect_rows(what + ' pred', pred, want.view(B, -1))


def _undecidable(ref, bound, K):
    """Pixels whose two largest reference logits lie within the sum of their bounds of each other."""
    if K == 1:
        return 0
    top = ref[:, :K].topk(2, dim=1)
    b = bound[:, :K].gather(1, top.indices)
    return int(((top.values[:, 0] - top.values[:, 1]) <= b[:, 0] + b[:, 1]).sum())


@pytest.mark.parametrize('name,dcode', DT)
def test_argmax_exact(C, name, dcode):
    for i, (shape, Kp, xm, Np, K, with_bias) in enumerate(HEAD):
        rng = np.random.default_rng(900 + i)
        x, wp, bias = _head_inputs(rng, dcode, True, shape[0] * shape[1] * shape[2], Kp, Np, K)
        _argmax_case(C, f'conv1x1_argmax {name} exact {HEAD[i]}', dcode, True, shape, Kp, xm, Np, K, x, wp, bias if with_bias else None,
                     via_pack=i == 3)


@pytest.mark.parametrize('name,dcode', DT)
def test_argmax_random(C, name, dcode):
    for i, (shape, Kp, xm, Np, K, with_bias) in enumerate(HEAD):
        rng = np.random.default_rng(1000 + i)
        x, wp, bias = _head_inputs(rng, dcode, False, shape[0] * shape[1] * shape[2], Kp, Np, K)
        _argmax_case(C, f'conv1x1_argmax {name} random {HEAD[i]}', dcode, False, shape, Kp, xm, Np, K, x, wp, bias if with_bias else None)


def _tie_levels():
    """(name, num_classes, Cout_p, per-class integer level, levels of the padded rows | None, expected class).  Every class row of the
    operand is the SAME integer row r, so logit[p, n] = r . x[p] + level[n]: the arg-max is that of `level` at every pixel while the values
    differ from pixel to pixel, and each pixel's result is written by another lane of the butterfly."""
    out = [('all classes equal', 64, 64, [2] * 64, None, 0), ('all classes equal', 21, 32, [-1] * 21, None, 0),
           ('class 7 and class 39: the step between the halves', 64, 64, [3 if n in (7, 39) else 0 for n in range(64)], None, 7),
           ('class 31 and class 32', 33, 64, [3 if n in (31, 32) else 1 for n in range(33)], None, 31),
           ('classes 39 and 45 of the upper half only', 64, 64, [3 if n in (39, 45) else 0 for n in range(64)], None, 39)]
    for d in (16, 8, 4, 2, 1):
        for a in (5, 21 | d):                          # a lower partner with the distance bit clear, and one with it set
            lo, hi = min(a, a ^ d), max(a, a ^ d)
            out.append((f'lanes {lo} and {hi} meet at distance {d}', 32, 32, [4 if n in (lo, hi) else n % 3 for n in range(32)], None, lo))
            out.append((f'lanes {lo} and {hi} of the upper half meet at distance {d}', 64, 64,
                        [4 if n in (32 + lo, 32 + hi) else n % 3 for n in range(64)], None, 32 + lo))
    out += [('the last of 21 classes under larger padded rows', 21, 32, [n % 5 for n in range(20)] + [6], [9] * 11, 20),
            ('the last of 33 classes under larger padded rows', 33, 64, [n % 5 for n in range(32)] + [6], [9] * 31, 32),
            ('class 0 of 1 under larger padded rows', 1, 32, [0], [9] * 31, 0)]
    return out


@pytest.mark.parametrize('name,dcode', DT)
def test_argmax_ties(C, name, dcode):
    shape, Kp = S16, 32
    npix = shape[0] * shape[1] * shape[2]
    for i, (tie, K, Np, level, padded, expect) in enumerate(_tie_levels()):
        rng = np.random.default_rng(1100 + i)
        x = torch.zeros(npix, Kp, device=DEV)
        x[:, :Kp - 3] = _ints(rng, (npix, Kp - 3), 4, 0.15)
        r = _ints(rng, (1, Kp - 3), 2, 0.07)
        wp = _pad2(r.expand(Np if padded else K, -1), Np, Kp)
        bias = torch.zeros(Np, device=DEV)
        bias[:K] = torch.tensor(level, dtype=torch.float32)
        if padded:
            bias[K:] = torch.tensor(padded, dtype=torch.float32)
        ref = _contract(x, wp, bias)[0]
        assert bool((_first_max(ref, K) == expect).all()) and int((ref[:, :K] == ref[:, :K].max(1, keepdim=True).values).sum()) >= npix
        assert not padded or bool((ref[:, K:].min(1).values > ref[:, :K].max(1).values).all())
        _argmax_case(C, f'conv1x1_argmax {name} tie: {tie}', dcode, True, shape, Kp, 1, Np, K, x, wp, bias)


@pytest.mark.parametrize('name,dcode', DT)
def test_argmax_two_slabs(C, name, dcode):
    """Cout_p = 128 would start two channel slabs per pixel tile, and a workgroup of the second slab (every lane -inf) would write pred = 64 over
    the first slab's result: the launcher refuses it (status -1, nothing launched, pred and the logits untouched).  Cout_p = 64 with the same
    21 classes runs and gives the first maximum."""
    L, s = C._lib, C._lib.stream_ptr()
    shape, Kp, K = S32A, 64, 21
    B, H, W = shape
    rng = np.random.default_rng(1200)
    x, wp, bias = _head_inputs(rng, dcode, True, B * H * W, Kp, 128, K)
    xa, wdev = _half(C, B * H * W, Kp, 1, dcode, x), _operand(C, wp, dcode)
    lg, pr = Rows(B * K, H * W), Rows(B, H * W, fill=-1, dtype=torch.int64)
    rc = L.load().clamd_conv1x1_argmax(xa.ptr, xa.ldc, L.ptr(wdev), L.ptr(bias), pr.ptr, lg.ptr, B, H, W, Kp, 128, K, dcode, s)
    _sync()
    assert rc == -1 and b'Cout' in L.load().clamd_last_error(), (rc, L.load().clamd_last_error())
    assert torch.equal(_raw(pr.buf), _raw(pr.before)) and torch.equal(_raw(lg.buf), _raw(lg.before)), 'a refused launch wrote'
    _argmax_case(C, f'conv1x1_argmax {name} 21 classes of Cout_p 64', dcode, True, shape, Kp, 1, 64, K, x, wp[:64].contiguous(), bias[:64].contiguous())


# ------------------------------------------------------------------------------------------------------------------------ layout kernels
def _source(vals, misalign):
    """fp32 values in a fresh buffer: at a 16-byte boundary, or 4 bytes past one."""
    buf = torch.full((vals.numel() + 8,), POISON, device=DEV)
    off = 4 + (1 if misalign else 0)
    view = buf[off:off + vals.numel()]
    view.copy_(vals.reshape(-1))
    assert view.data_ptr() % 16 == (4 if misalign else 0)
    return view


def _bf16_distinct(n):
    """n distinct, increasing values that bf16 holds exactly (consecutive bf16 bit patterns from 1.0 on): a swapped tap or neighbour shows in
    every storage."""
    return (torch.arange(n, dtype=torch.int32) + 0x3F80).to(torch.int16).view(torch.bfloat16).float().to(DEV)


@pytest.mark.parametrize('name,dcode', DT)
def test_nchw_to_nhwc(C, name, dcode):
    L, s = C._lib, C._lib.stream_ptr()
    for Cl, Cp in ((1, 32), (5, 32), (21, 32), (32, 32), (40, 64)):
        for B, H, W in ((2, 6, 10), (2, 5, 7)):
            npix = B * H * W
            x = _dev(np.random.default_rng(Cl * 100 + H).standard_normal((B, Cl, H * W)).astype(np.float32))
            for ldm in (1, 2):
                for mul in (1.0, 0.37):
                    res = []
                    for misalign in (False, True):
                        what = f'nchw_to_nhwc {name} C {Cl} of {Cp} pitch x{ldm} mul {mul} {B}x{H}x{W} misaligned {misalign}'
                        src = _source(x, misalign)

                        def launch():
                            out = _half(C, npix, Cp, ldm, dcode)
                            L.call('clamd_nchw_to_nhwc', src.data_ptr(), out.ptr, out.ldc, B, Cl, H, W, Cp, mul, dcode, s)
                            _sync()
                            return [out]

                        out, = _twice(what, launch)
                        exp = torch.zeros(npix, Cp, device=DEV)
                        exp[:, :Cl] = (x * torch.tensor(mul, dtype=torch.float32, device=DEV)).permute(0, 2, 1).reshape(npix, Cl)
                        _expect_bits(what, out, exp)
                        assert bool(out.zero_bits()[:, Cl:].all()), what + ': channels C .. Cp - 1 are not +0'
                        res.append(out)
                    assert torch.equal(_raw(res[0].buf), _raw(res[1].buf)), \
                        f'nchw_to_nhwc {name} C {Cl} of {Cp} {B}x{H}x{W}: the aligned and the misaligned source give different bits'


@pytest.mark.parametrize('name,dcode', DT)
def test_nhwc_to_nchw(C, name, dcode):
    L, s = C._lib, C._lib.stream_ptr()
    for Cl, Cp in ((21, 32), (40, 64), (1, 32)):
        for B, H, W in ((2, 5, 7), (1, 6, 10)):
            npix = B * H * W
            what = f'nhwc_to_nchw {name} C {Cl} of {Cp} {B}x{H}x{W}'
            v = _normal(np.random.default_rng(Cl + H), (npix, Cp), dcode, zeros=0.1)
            src = _half(C, npix, Cp, 2, dcode, v)

            def launch():
                dst = Rows(B * Cl, H * W)
                L.call('clamd_nhwc_to_nchw', src.ptr, src.ldc, dst.ptr, B, Cl, H, W, dcode, s)
                _sync()
                return [dst]

            dst, = _twice(what, launch)
            _expect_rows(what, dst, _nchw(v, B, Cl))
            assert src.guards_intact() and torch.equal(_raw(src.buf), _raw(src.before))


@pytest.mark.parametrize('name,dcode', DT)
def test_nhwc_to_nchw_second_trip(C, name, dcode):
    """The grid runs over B C H W elements, capped at 8192 workgroups of 256: C 40 of Cp 64 at pitch 128 on 1 x 230 x 230 is 2116000 elements,
    so workgroups 0 .. 73 make a second, partial trip of the grid-stride loop (27 MB of source in fp32, 8.5 MB written)."""
    L, s = C._lib, C._lib.stream_ptr()
    (B, H, W), Cl, Cp = (1, 230, 230), 40, 64
    npix, cap = B * H * W, 8192 * 256
    assert cap < npix * Cl < 2 * cap and (npix * Cl) % cap
    what = f'nhwc_to_nchw {name} C {Cl} of {Cp} {B}x{H}x{W} second trip'
    v = _normal(np.random.default_rng(7), (npix, Cp), dcode, zeros=0.1)
    src = _half(C, npix, Cp, 2, dcode, v)

    def launch():
        dst = Rows(B * Cl, H * W)
        L.call('clamd_nhwc_to_nchw', src.ptr, src.ldc, dst.ptr, B, Cl, H, W, dcode, s)
        _sync()
        return [dst]

    dst, = _twice(what, launch)
    _expect_rows(what, dst, _nchw(v, B, Cl))
    assert src.guards_intact() and torch.equal(_raw(src.buf), _raw(src.before))


def _im2col_ref(x, Cp):
    """x [B, C, H, W] -> [B H W, Cp]: column c 9 + ky 3 + kx = x[b, c, y + ky - 1, x + kx - 1], zero outside the image and from 9 C on."""
    B, Cl, H, W = x.shape
    xp = torch.zeros(B, Cl, H + 2, W + 2, device=x.device)
    xp[:, :, 1:H + 1, 1:W + 1] = x
    out = torch.zeros(B, H, W, Cp, device=x.device)
    for c in range(Cl):
        for ky in range(3):
            for kx in range(3):
                out[..., c * 9 + ky * 3 + kx] = xp[:, c, ky:ky + H, kx:kx + W]
    return out.reshape(B * H * W, Cp)


@pytest.mark.parametrize('name,dcode', DT)
def test_im2col3(C, name, dcode):
    """The launcher's dispatch: C <= 3 and Cp 32 -> the piece kernel, but bf16 from an aligned source with W % 4 == 0 -> the four-pixel kernel
    (pitch 32: LDS exchange; pitch 64: plain stores); everything else -> the generic kernel."""
    L, s = C._lib, C._lib.stream_ptr()
    for B, H, W in ((1, 5, 12), (3, 10, 36), (2, 6, 7)):
        npix = B * H * W
        for Cl, Cp, ldcs in ((1, 32, (32, 64)), (3, 32, (32, 64)), (5, 64, (64, 128)), (2, 64, (64, 128))):
            x = _bf16_distinct(B * Cl * H * W).view(B, Cl, H, W)
            exp = _im2col_ref(x, Cp)
            assert int((exp != 0).sum()) > 0 and bool((exp[:, 9 * Cl:] == 0).all())
            for ldc in ldcs:
                for misalign in (False, True):
                    what = f'nchw_im2col3 {name} C {Cl} of {Cp} pitch {ldc} {B}x{H}x{W} misaligned {misalign}'
                    src = _source(x, misalign)

                    def launch():
                        out = ActAt(C, npix, Cp, ldc, dcode)
                        L.call('clamd_nchw_im2col3', src.data_ptr(), out.ptr, ldc, B, Cl, H, W, Cp, dcode, s)
                        _sync()
                        return [out]

                    out, = _twice(what, launch)
                    _expect_bits(what, out, exp)
                    assert bool(out.zero_bits()[exp == 0].all()), what + ': not +0 outside the image or from 9 C on'
