"""GPU: the pre-transformed Winograd forward / data-gradient kernels and their filter packs, per element -- clamd_conv3x3_winograd44_pre
(wino44g_kernel, F(4x4,3x3), csrc/wino44g.hip), clamd_conv3x3_winograd24_pre (wino24g_kernel, F(2x4,3x3), wino24g.hip), clamd_wino44_pack
(wino44_pack_kernel) and clamd_wino24_pack (wino24_pack_kernel, wino24.hip).  The in-kernel-transform kernels and the border-class bias are
not covered here.

Every case calls the C ABI directly on host-generated inputs.  Every buffer a launch writes -- y (at its own pitch, or as the second half
of a buffer of twice the pitch whose first half is poisoned), the statistics rows (exactly clamd_stat_rows rows, EXTRA_ROWS poisoned rows
behind them), the packed filters, V -- sits between guard bands that must come back bit-identical, is pre-filled with NaN, and every launch
runs twice and must give the same bits (_twice).  References are float64 torch evaluations; the matrices and layouts are grid_util's
(the kernel comments' B^T, G, A^T; V [tile block][Cin_p / 8][P][2][32][4], U [Cin_p / 8][P][Cout_p][8], plane = 6 i + j).

1. The kernels on operands placed by hand (test_fwd_exact, test_fwd_low_magnitude, test_fwd_persistent).  The kernel computes
   Y = A^T (sum_c U[c, n, plane] V[tile, c, plane]) A for ANY U and V, so both are filled directly with integers in {-2 .. 2} (about a quarter
   zeros) in the documented layouts: no transform, no pack.  F(2x4) stores row i = 2 negated in BOTH operands, so the product is the true one
   and the reference applies the true A4^T, A6^T to the stored values.  Every term bound |A|^T (sum_c |U| |V|) |A| + |bias| is asserted
   below 2^24 from the reference (at most 361 * 4 * Cin_p: 19 = the largest absolute row sum of A6^T), so M and Y are integers in fp32 in any
   order of summation and
     Y                EQUALS the float64 reference as numbers for every element, with integer bias and ReLU (full), without either and
                      without statistics (plain: the data-gradient path), with ReLU alone and with bias + statistics alone
     tiles outside    a ragged image hold NaN in V instead of the transform's zeros: none of it reaches Y, the guard bands or the rows
     statistics rows  EVERY row: one workgroup per item -> row tm = that tile block's per-channel sums over in-image pixels; persistent grid
                      -> row blockIdx = the sums over exactly the items that workgroup ran, from this file's copy of decode (xcd_remap,
                      band from the copy of wino_band, per_band, stride gridDim) and of the grid rule of wino_forward_plan.  First moments
                      are exact (asserted: the sum of |y| per row < 2^24).  Second moments are exact wherever the sum of y^2 per row stays
                      below 2^24 -- asserted to hold in the low-magnitude case of each form ({-1, 0, 1}, three quarters zeros, Cin_p 16 /
                      64) -- and within gamma(n) sum(y^2) elsewhere, gamma(n) = n u / (1 - n u), u = 2^-24, n = additions on the longest chain:
                        F(4x4): per item 8 fmas of a reader thread (2 columns x 4 rows) + 1 into its running sum = 9; per fold 3 shuffle
                                steps + 8 wave partials + 1 onto the row (persistent grid only) = 12; n = 21 x (items of the busiest workgroup)
                        F(2x4): per item 8 fmas (4 columns x 2 rows) into the running register = 8; per fold 3 shuffle steps + 3 wave
                                partials + 1 onto the row = 7; n = 15 x (items of the busiest workgroup)
                      (every item charged a fold of its own: an upper bound).  Output channels whose filters and bias are zero: zero.
2. The filter packs (test_pack) through ops.WinoPackTable(24 / 36): random fp32 filters, forward and data-gradient (tap-flipped, transposed)
   jobs, identity / padded N / padded K / two-segment K / two-segment N channel maps, kscale with a zero and a negative entry on the forward
   jobs, two and three jobs per table.  |U - G g G^T| <= gamma(n) |G| |g| |G|^T against the float64 product placed by the layout (F(2x4):
   row 2 negated), n = roundings of the kernel's formulas, rounded constants included: the row stage G4 0.5 (a + b + c) is 2 (the halving is
   exact); a G6 stage is 4: -1/6 (a + b + c) = two additions, the constant, the product; (1/24) a + (1/12) b + (1/6) c = per term the
   constant and the product, then two additions, of which a term passes at most two.  F(2x4): 2 + 4 = 6, F(4x4): 4 + 4 = 8, + 1 with kscale
   (g * kscale).  The bound is 0 on padded rows and columns and under a zero scale: zero as a number (the kernel's -1/6 * 0 is -0).
3. End to end (test_end_to_end): x -> clamd_winograd{24,44}_transform_input -> packed filters -> clamd_conv3x3_winograd{24,44}_pre, forward
   with bias, ReLU and statistics, and the data gradient with the wd filters, on random fp32 data, a concat input (two cin_segs) and padded
   output channels included.  Reference: the float64 direct sum over the nine taps of shifted slices of the host inputs.  Per element
   |y - ref| <= gamma(n_V + n_U + K + n_A + 1) (M + |bias|), data gradient gamma(n_V + n_U + K + n_A) M, M = |A|^T (sum_c |U| |V|) |A| of the
   float64 intermediates; n_V = 3 / 4 (grid_util.FORM), n_U = 6 / 8 (above), K = Cin_p accumulations, n_A = the output transform: A6^T in-lane
   m0 + (m1 + m2) + (m3 + m4) and fma(8, m3 - m4, m1 - m2) + m5 are 3, the same across the rows 3 (F(4x4): 6), A4^T r0 + r1 + r2 is 2
   (F(2x4): 5); + 1 for the bias addition (ReLU is 1-Lipschitz).  The float64 A^T (sum U V) A is asserted to BE the direct sum, so matrices
   and layouts are checked without any kernel.  Padded channels of y and of the input gradient are exactly zero.  The rows are compared with
   the sums of the y the launch stored, within gamma(n) sum |y| and gamma(n) sum y^2.  UNIT is empty: nothing exceeds u = 2^-24.

Paths (check_wino_fwd_plans asserts them from this file's copies of the launcher's rules; no device):
  wino44g_kernel<4|8, RAGGED>      1 x 16 x 32 (one whole wide block), 1 x 20 x 36 (ragged, four blocks), 2 x 36 x 20 (narrow, ragged),
                                   1 x 32 x 16 (narrow, whole), each with Cin_p 16, 24, 64 (nk = 2, 3, 8: one, two and seven trips of the K loop)
  wino24g_kernel<4|8, RAGGED, 2>   1 x 8 x 32, 1 x 10 x 36, 2 x 18 x 20, 2 x 16 x 16, each with Cin_p 64 and 96 (one and two refills of each set)
  both                             Cout_p 64, 128, 192; y at its own pitch and as the second half of 2 Cout_p; five zeroed output channels
  persistent loop                  3 x 48 x 96 / 3 x 24 x 96, Cin_p 16 / 64, Cout_p 640: 27 blocks x 10 slabs = 270 items; default: 256 workgroups,
                                   14 of them run two items; cu_reserve 128: 128 workgroups, 14 run three, a slab change inside a workgroup
                                   (fold_stats, then flush_row onto the row it wrote before); wino_persist 0: 270 workgroups, one row per tile
                                   block; wino_band 1 and 2 forced.  Y is bit-identical under all of them
Worst error / bound on the MI355X in one run of this file (RATIOS; 38 cases in 6.3 s; hand-placed operands: Y and the first moments EQUAL the
reference in every case, the second moments wherever a row's sum of y^2 stays below 2^24, elsewhere the ratio of the first column):
                                 second moments    |  random: forward  data gradient  rows (1st, 2nd moments)  |  pack
  conv3x3_winograd24_pre         0.066             |          0.010    0.011          0.178, 0.179             |  wino24_pack   0.477
  conv3x3_winograd44_pre         0.124             |          0.010    0.009          0.129, 0.140             |  wino44_pack   0.418
(The random output bound is loose because K u M charges every accumulation a worst-case rounding of the whole magnitude; the hand-placed
cases and the packs are the sharp ones.)
Left unreached: Cout_p that is no multiple of 64 and Cin_p off the launcher's rule (refused on entry; test_wino44_gpu.py asserts the refusal);
the 2^31 / 2^32-byte operand and image limits; a forced wino_band of 4 and more (the 10 slabs of the persistent case divide by 2 only).
Mutation check (one scratch build with both, not committed): 8 -> 8 (1 + 2^-18) in the row stage of wino44g_kernel's output transform fails
every hand-placed F(4x4) case (14: "Y: 3893 of 32768 elements differ; worst ... got 3957.0139, expected 3957.0") and passes the random bound;
0.25 -> 0.25 (1 + 2^-16) in the column stage of wino24_pack_kernel fails all four F(2x4) pack cases at error / bound 43; the 2e-5 tests
test_wino44_gpu.py::test_conv3x3_winograd44_pretransformed and test_kernels_gpu.py::test_conv3x3_winograd24_pretransformed pass both (12
passed).  With 2^-16 on the 8 the F(4x4) oracle test does notice (2.3 - 2.8e-5 against its 2e-5): it sees a quarter of that step no more.
"""
import numpy as np
import pytest
import torch

from grid_util import (DEV, EPS, FORM, Rows, _expect_vals, _geom, _half, _ints, _m, _normal, _per_element, _planes_n, _raw, _sign, _tile_origin,
                       _twice, _u_index, _u_layout, _u_unindex, _untile, _v_layout, _wg_map, _xform)

pytestmark = pytest.mark.gpu

UNIT = {}                                      # entry point -> u of the random bound where EPS is exceeded (none is: see above)
NCU = 256                                      # compute units of the MI355X (asserted against the device by the fixture)
# planes; transformed input per input element (wino_band's traffic model); the launcher's Cin_p rule; roundings of the pack and of the output
# transform; additions per item / per fold on a statistics chain (all counted in the docstring)
PRE = {24: dict(P=24, band_x=3.0, cin_mult=32, cin_min=64, nU=6, nA=5, stat=(8, 7), op='OP_CONV3X3_WINOGRAD24'),
       44: dict(P=36, band_x=2.25, cin_mult=8, cin_min=16, nU=8, nA=6, stat=(9, 12), op='OP_CONV3X3_WINOGRAD44')}
SH = {24: [(1, 8, 32), (1, 10, 36), (2, 18, 20), (2, 16, 16)], 44: [(1, 16, 32), (1, 20, 36), (2, 36, 20), (1, 32, 16)]}
KP = {24: (64, 96), 44: (16, 24, 64)}
NP = (64, 128, 192)
#            bias   relu  statistics
VARIANTS = {'full': (True, 1, True), 'plain': (False, 0, False), 'relu': (False, 1, False), 'bias+stats': (True, 0, True)}


@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    C._lib.load()
    assert torch.cuda.get_device_properties(0).multi_processor_count == NCU
    return C


def _sync():
    torch.cuda.synchronize()


def _gamma(n):
    return n * EPS / (1.0 - n * EPS)


# ----------------------------------------------------------------------------------------------------- the launcher's rules, in Python
TUNE0 = dict(wino_band=0, wino_persist=1, cu_reserve=0)


def _td(tune):
    return dict(TUNE0, **tune)


def _tuning(C, tune):
    tn = C._lib.Tuning(**tune)
    assert {k: v for k, v in tn.as_dict().items() if k in TUNE0} == _td(tune)
    return tn


def _cus(td):
    """clamd_usable_cus."""
    return max(8, NCU - max(td['cu_reserve'], 0))


def xcd_remap(bid, nwg):
    q, r, x, i = nwg >> 3, nwg & 7, bid & 7, bid >> 3
    return (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + i


def wino_band(tiles, slabs, x_elems, f_elems, forced):
    """Output-channel slabs per band of the block order: the cheapest power of two that divides the slabs, or `forced` rounded down to one."""
    best, best_cost, b = 1, 0.0, 1
    while b <= 32 and b <= slabs:
        if slabs % b:
            break
        a = min(32.0 / b, float(tiles))
        cost = x_elems * (slabs / b) + f_elems * (tiles / a)
        if b == 1 or cost < best_cost:
            best, best_cost = b, cost
        b *= 2
    if forced > 0:
        best = 1
        while best * 2 <= forced and slabs % (best * 2) == 0:
            best *= 2
    return best


def _fwd_plan(form, shape, Kp, Np, td):
    """wino_pre_conv3x3 + wino_forward_plan + wino_stat_rows + the kernels' decode: the instantiation, the grid, the rows and, per
    workgroup, the (slab tn, tile block tm) items it runs, in order."""
    f, g = PRE[form], _geom(form, shape)
    B, H, W = shape
    assert Kp % f['cin_mult'] == 0 and Kp >= f['cin_min'] and Np % 64 == 0
    tiles, slabs, cus = g['ntm'], Np // 64, _cus(td)
    nblk = tiles * slabs
    band = wino_band(tiles, slabs, f['band_x'] * B * H * W * Kp, float(f['P']) * Kp * Np, td['wino_band'])
    grid = min(nblk, cus) if td['wino_persist'] else nblk
    rows = cus if (td['wino_persist'] and nblk > cus) else tiles
    per_wg = grid < nblk
    assert rows == (grid if per_wg else tiles)
    per_band = tiles * band

    def decode(v):
        bnd, rem = divmod(xcd_remap(v, nblk), per_band)
        return bnd * band + rem % band, rem // band

    items = [[decode(v) for v in range(wg, nblk, grid)] for wg in range(grid)]
    assert sorted(it for its in items for it in its) == [(tn, tm) for tn in range(slabs) for tm in range(tiles)], 'decode is no bijection'
    return dict(TXN=g['TXN'], ragged=bool(H % g['PH'] or W % g['PW']), nk=Kp // 8, tiles=tiles, slabs=slabs, nblk=nblk, band=band, grid=grid,
                rows=rows, per_wg=per_wg, items=items, busiest=max(len(its) for its in items))


def _stat_n(form, pl):
    a, b = PRE[form]['stat']
    return (a + b) * (pl['busiest'] if pl['per_wg'] else 1)


# ------------------------------------------------------------------------------------------------------------------- section 1: references
def _in_image(g, shape):
    """[Tp] bool: the tile has pixels inside the image (H and W are whole numbers of tiles: all of them or none)."""
    return torch.tensor([(lambda o: o[1] < shape[1] and o[2] < shape[2])(_tile_origin(g, t)) for t in range(g['Tp'])], device=DEV)


def _out_transform(form, M, g, shape, absolute=False):
    """[P, Tp, N] plane products -> the image [B, H, W, N] of A_rows^T M A_cols with the TRUE matrices."""
    ni, nj = _planes_n(form)
    Ar, Ac = (_m(m, absolute) for m in FORM[form]['A'])
    return _untile(torch.einsum('ia,ijtn,jb->tabn', Ar, M.view(ni, nj, *M.shape[1:]), Ac), g, shape)


def _plane_products(V, U, absolute=False):
    """V [Tp, P, Kp], U [Kp, P, Np] -> [P, Tp, Np] = sum_c V U per plane."""
    V, U = (V.abs(), U.abs()) if absolute else (V, U)
    return torch.bmm(V.permute(1, 0, 2), U.permute(1, 0, 2))


def _block_sums(v, g, shape):
    """[B, H, W, N] -> [tile blocks, N]: per-channel sums over the in-image pixels of every tile block, in the order tm."""
    B, H, W = shape
    pad = torch.zeros(B, g['by'] * g['PH'], g['bx'] * g['PW'], v.shape[-1], dtype=torch.float64, device=v.device)
    pad[:, :H, :W] = v
    return pad.view(B, g['by'], g['PH'], g['bx'], g['PW'], -1).sum((2, 4)).reshape(g['ntm'], -1)


def _row_sums(pl, S):
    """[tile blocks, Np] block sums -> [rows, Np]: what every statistics row of the plan holds."""
    if not pl['per_wg']:
        return S.clone()
    trip = [(wg, tn, tm) for wg, its in enumerate(pl['items']) for tn, tm in its]
    wg, tn, tm = (torch.tensor(c, dtype=torch.long, device=S.device) for c in zip(*trip))
    E = torch.zeros(pl['rows'], pl['slabs'], 64, dtype=torch.float64, device=S.device)
    E.index_put_((wg, tn), S.view(-1, pl['slabs'], 64)[tm, tn], accumulate=True)
    return E.view(pl['rows'], -1)


def _fwd_expect(form, shape, Kp, Np, npad, seed, low=False):
    """Hand-placed operands and everything a launch on them is compared with: the stored V (NaN in the tiles outside the image) and U as
    the kernels read them, an integer bias, the float64 image A^T (sum_c U V) A.  Asserts the 2^24 condition of every element."""
    g, P = _geom(form, shape), PRE[form]['P']
    rng = np.random.default_rng(seed)
    amax, zeros = (1, 0.625) if low else (2, 0.07)
    V, U = _ints(rng, (g['Tp'], P, Kp), amax, zeros).double(), _ints(rng, (Kp, P, Np), amax, zeros).double()
    bias = _ints(rng, (Np,), 3, 0.0).double()
    if npad:
        U[:, :, Np - npad:] = 0
        bias[Np - npad:] = 0
    img = _out_transform(form, _plane_products(V, U), g, shape)
    mag = _out_transform(form, _plane_products(V, U, True), g, shape, True)
    assert float(mag.max()) + float(bias.abs().max()) < 2 ** 24, 'a sum of absolute terms reaches 2^24'
    assert float(mag.max()) <= 361 * 4 * Kp
    inimg = _in_image(g, shape)
    assert bool(inimg.all()) == (shape[1] % g['PH'] == 0 and shape[2] % g['PW'] == 0)
    Vs = V.clone()
    Vs[~inimg] = float('nan')
    return dict(g=g, V=_v_layout(Vs).float(), U=_u_layout(U).float(), bias=bias, img=img, Kp=Kp, Np=Np, npad=npad, low=low, shape=shape)


def _fwd_stats_expect(form, ex, pl, yv):
    """The rows of a launch whose stored image is yv: (first moments, second moments, second moments exact?), with the conditions asserted."""
    E1, EA, E2 = (_row_sums(pl, _block_sums(t, ex['g'], ex['shape'])) for t in (yv, yv.abs(), yv * yv))
    assert float(EA.max()) < 2 ** 24, 'the sum of |y| of a row reaches 2^24: first moments would not be exact'
    exact2 = float(E2.max()) < 2 ** 24
    assert exact2 or not ex['low'], f'the low-magnitude case does not keep sum y^2 below 2^24 ({float(E2.max()):.3g})'
    return E1, E2, exact2


def _fwd_image(ex, variant):
    bias, relu, _ = VARIANTS[variant]
    yv = ex['img'] + ex['bias'] if bias else ex['img'].clone()
    return yv.clamp_min(0) if relu else yv


def _filled(values):
    r = Rows(values.numel())
    r.view.copy_(values)
    r.before = r.buf.clone()
    return r


def _fwd_run(C, what, form, ex, bufs, mult, variant, tune):
    """One variant of one case: two launches, Y and every statistics row against the reference.  Returns the y buffer."""
    L, s = C._lib, C._lib.stream_ptr()
    B, H, W = shape = ex['shape']
    Kp, Np, npix = ex['Kp'], ex['Np'], B * H * W
    pl = _fwd_plan(form, shape, Kp, Np, _td(tune))
    tn = _tuning(C, tune)
    has_bias, relu, has_stats = VARIANTS[variant]
    what = f'{what} {variant} [TXN {pl["TXN"]} RAGGED {pl["ragged"]} nk {pl["nk"]} grid {pl["grid"]} of {pl["nblk"]} band {pl["band"]} rows {pl["rows"]}]'
    assert L.stat_rows(getattr(L, PRE[form]['op']), B, H, W, Kp, Np, 0, False, tn) == pl['rows'], what
    v, u, bias = bufs

    def launch():
        y = _half(C, npix, Np, mult, 0)
        st = Rows(pl['rows'], 2, Np) if has_stats else None
        L.call(f'clamd_conv3x3_winograd{form}_pre', v.ptr, u.ptr, L.ptr(bias) if has_bias else None, y.ptr, y.ldc, st.ptr if st else None,
               pl['rows'] if st else 0, B, H, W, Kp, Np, relu, tn.ref(), s)
        _sync()
        return [y, st] if st else [y]

    out = _twice(what, launch)
    assert torch.equal(_raw(v.buf), _raw(v.before)) and torch.equal(_raw(u.buf), _raw(u.before)), what + ': an operand was written'
    y = out[0]
    yv = _fwd_image(ex, variant)
    _expect_vals(what + ' Y', y.get(), yv.reshape(npix, Np))
    if ex['npad']:
        assert not bool(y.get()[:, Np - ex['npad']:].any()), what + ': an output channel without filters or bias is not zero'
    if has_stats:
        st = out[1]
        E1, E2, exact2 = _fwd_stats_expect(form, ex, pl, yv)
        assert not bool(torch.isnan(st.view).any()), what + ': a statistics word was not written'
        _expect_vals(what + ' first moments', st.view[:, 0], E1)
        if exact2:
            _expect_vals(what + ' second moments', st.view[:, 1], E2)
        else:
            _per_element(what + ' second moments', f'conv3x3_winograd{form}_pre rows (hand-placed)', st.view[:, 1], E2, _gamma(_stat_n(form, pl)) * E2)
        if ex['npad']:
            assert not bool(st.view[:, :, Np - ex['npad']:].any()), what + ': a zero channel of a row is not zero'
    return y


def _fwd_bufs(ex):
    return _filled(ex['V']), _filled(ex['U']), ex['bias'].float().contiguous()


def _small_rows(form):
    """(shape index, Cin_p, Cout_p, y as the n-th half, zeroed output channels, third variant): every shape with every Cin_p."""
    rows = []
    for si in range(4):
        for ki, Kp in enumerate(KP[form]):
            i = len(rows)
            rows.append((si, Kp, NP[(si + ki) % 3], 1 + (si + ki) % 2, (0, 5)[(i // 2) % 2], ('relu', 'bias+stats')[i % 2]))
    return rows


@pytest.mark.parametrize('form,i', [(form, i) for form in (24, 44) for i in range(len(_small_rows(form)))], ids=lambda v: str(v))
def test_fwd_exact(C, form, i):
    si, Kp, Np, mult, npad, third = _small_rows(form)[i]
    ex = _fwd_expect(form, SH[form][si], Kp, Np, npad, 6000 + 100 * form + i)
    bufs = _fwd_bufs(ex)
    for variant in ('full', 'plain', third):
        _fwd_run(C, f'conv3x3_winograd{form}_pre exact {SH[form][si]} Cin_p {Kp} Cout_p {Np} pitch x{mult}', form, ex, bufs, mult, variant, {})


LOW = {24: (1, 64, 128), 44: (1, 16, 128)}            # shape index, Cin_p, Cout_p of the case whose second moments are exact


@pytest.mark.parametrize('form', [24, 44])
def test_fwd_low_magnitude(C, form):
    si, Kp, Np = LOW[form]
    ex = _fwd_expect(form, SH[form][si], Kp, Np, 0, 6900 + form, low=True)
    _fwd_run(C, f'conv3x3_winograd{form}_pre low magnitude {SH[form][si]} Cin_p {Kp} Cout_p {Np}', form, ex, _fwd_bufs(ex), 1, 'full', {})


PERSIST = {24: ((3, 24, 96), 64, 640), 44: ((3, 48, 96), 16, 640)}
PTUNE = [dict(), dict(cu_reserve=128), dict(wino_persist=0), dict(wino_band=1), dict(wino_band=2)]


@pytest.mark.parametrize('form', [24, 44])
def test_fwd_persistent(C, form):
    """270 items: the persistent loop, its prefetch across tiles and its per-workgroup rows, under five plans.  Y is bit-identical under all."""
    shape, Kp, Np = PERSIST[form]
    ex = _fwd_expect(form, shape, Kp, Np, 5, 7000 + form)
    bufs = _fwd_bufs(ex)
    what = f'conv3x3_winograd{form}_pre persistent {shape} Cin_p {Kp} Cout_p {Np}'
    first = None
    for tune in PTUNE:
        y = _fwd_run(C, f'{what} {tune}', form, ex, bufs, 1, 'full', tune)
        first = first if first is not None else y
        assert torch.equal(_raw(y.buf), _raw(first.buf)), f'{what} {tune}: Y depends on the grid or the block order'
    _fwd_run(C, what, form, ex, bufs, 2, 'plain', dict(cu_reserve=128))


# ------------------------------------------------------------------------------------------------------------- section 2: the filter packs
#        per convolution of the table: (Cout, cin_segs, kscale, forward job, data-gradient job)
PACK = [[(32, [(32, 32)], False, True, True)],                                                  # identity maps
        [(20, [(24, 32)], True, True, True)],                                                   # padded N, padded K (and the reverse for wd)
        [(40, [(10, 16), (12, 16)], True, True, True), (32, [(32, 32)], True, True, False)],    # two-segment K / N; three jobs
        [(64, [(30, 32), (32, 32)], False, False, True), (33, [(16, 16)], True, True, False)]]  # a data-gradient job in front of a forward one


def _cpad(c):
    """ops.cpad."""
    return max(32, 1 << (int(c) - 1).bit_length())


def _pack_ref(form, w, Np, nmap, Kp, kmap, dgrad, ks):
    """w [Cout][Cin][3][3] -> (G g G^T, |G| |g| |G|^T) as float64 [Kp, P, Np] in the kernels' sign convention: g = w[n][k] (forward) or the
    tap-flipped w[k][n] (data gradient) of the logical channels behind physical (n, k), zero elsewhere, times kscale[physical k]."""
    g = w.double().permute(1, 0, 2, 3).flip(2, 3) if dgrad else w.double()
    gp = torch.zeros(Np, Kp, 3, 3, dtype=torch.float64, device=w.device)
    gp[_wg_map(nmap, Np)[:, None], _wg_map(kmap, Kp)[None, :]] = g
    if ks is not None:
        gp = gp * ks.double()[None, :, None, None]
    out = []
    for absolute in (False, True):
        Gr, Gc = (_m(m, absolute) for m in FORM[form]['G'])
        out.append(torch.einsum('ia,nkab,jb->kijn', Gr, gp.abs() if absolute else gp, Gc).reshape(Kp, -1, Np))
    return out[0] * _sign('pre%d' % form, form)[None, :, None], out[1]


def _pack_inputs(form, convs, seed):
    """Per convolution: w, kscale (entry 1 zero, entry 2 negative) and, per job, (Np, Kp, dgrad, float64 U, |U| bound magnitude, roundings)."""
    rng = np.random.default_rng(seed)
    res = []
    for cout, segs, kscale, fwd, dg in convs:
        cin, cin_p, cout_p = sum(s[0] for s in segs), sum(s[1] for s in segs), _cpad(cout)
        w = _normal(rng, (cout, cin, 3, 3), 0, zeros=0.1)
        ks = None
        if kscale:
            ks = _normal(rng, (cin_p,), 0, zeros=0.0)
            ks[1], ks[2] = 0.0, -ks[2].abs() - 0.5
        seg = tuple(segs[0]) if len(segs) == 2 else (cin, cin_p)
        jobs = []
        if fwd:
            jobs.append((cout_p, cin_p, *_pack_ref(form, w, cout_p, (cout, cout, cout_p), cin_p, (cin,) + seg, False, ks), PRE[form]['nU'] + (1 if kscale else 0)))
        if dg:
            jobs.append((cin_p, cout_p, *_pack_ref(form, w, cin_p, (cin,) + seg, cout_p, (cout, cout, cout_p), True, None), PRE[form]['nU']))
        res.append(dict(w=w, ks=ks, segs=segs, cout=cout, fwd=fwd, dg=dg, jobs=jobs))
    return res


def _pack_launch(C, form, convs):
    """One table, one launch: the destinations in job order."""
    tab, dsts = C.ops.WinoPackTable(PRE[form]['P']), []
    for cv in convs:
        d = [Rows(PRE[form]['P'] * j[0] * j[1]) for j in cv['jobs']]
        tab.conv3x3(cv['w'], d[0].view if cv['fwd'] else None, d[-1].view if cv['dg'] else None, cv['segs'], cv['cout'], cv['ks'])
        dsts += d
    tab.finalize(DEV).run()
    _sync()
    assert len(tab.jobs) == len(dsts)
    return dsts


@pytest.mark.parametrize('form,i', [(form, i) for form in (24, 44) for i in range(len(PACK))], ids=lambda v: str(v))
def test_pack(C, form, i):
    convs = _pack_inputs(form, PACK[i], 8000 + 10 * form + i)
    what = f'wino{form}_pack {PACK[i]}'
    dsts = _twice(what, lambda: _pack_launch(C, form, convs))
    jobs = [j for cv in convs for j in cv['jobs']]
    for k, (d, (Np, Kp, U, aU, n)) in enumerate(zip(dsts, jobs)):
        assert not bool(torch.isnan(d.view).any()), f'{what} job {k}: an element of the destination was not written'
        _per_element(f'{what} job {k} [Np {Np} Kp {Kp} n {n}]', f'wino{form}_pack', d.view, _u_layout(U), (_gamma(n) + 2.0 ** -50) * _u_layout(aU))


# ------------------------------------------------------------------------------------------------------------------ section 3: end to end
#      shape index, cin_segs, Cout, y as the n-th half
E2E = [(1, [(20, 32), (25, 32)], 100, 2),            # ragged wide blocks, a concat input, padded output channels
       (2, [(64, 64)], 64, 1),                       # narrow ragged blocks, two images
       (0, [(50, 64), (64, 64)], 64, 1)]             # one whole block, a concat input with a padded first segment, Cin_p 128
E2E_TUNE = [dict(), dict(), dict(wino_band=1)]


def _conv_ref(a, w, shape, dgrad):
    """a [npix, Ca] float64, w [Cout][Cin][3][3] -> the float64 direct sum over the nine taps (and the sum of the absolute terms): forward
    y[p, n] = sum a[p + (ky - 1, kx - 1), c] w[n, c, ky, kx]; data gradient gx[p, c] = sum a[p - (ky - 1, kx - 1), n] w[n, c, ky, kx]."""
    B, H, W = shape
    pad = torch.zeros(B, H + 2, W + 2, a.shape[1], dtype=torch.float64, device=a.device)
    pad[:, 1:H + 1, 1:W + 1] = a.view(B, H, W, -1)
    wd = w.double()
    out, mag = 0.0, 0.0
    for ky in range(3):
        for kx in range(3):
            oy, ox = (2 - ky, 2 - kx) if dgrad else (ky, kx)
            sl = pad[:, oy:oy + H, ox:ox + W].reshape(B * H * W, -1)
            m = wd[:, :, ky, kx] if dgrad else wd[:, :, ky, kx].T
            out, mag = out + sl @ m, mag + sl.abs() @ m.abs()
    return out, mag


def _e2e_expect(form, i, seed):
    si, segs, cout, _ = E2E[i]
    shape = SH[form][si]
    B, H, W = shape
    g, npix = _geom(form, shape), B * H * W
    cin, cin_p, cout_p = sum(s[0] for s in segs), sum(s[1] for s in segs), _cpad(cout)
    rng = np.random.default_rng(seed)
    x, gz = _normal(rng, (npix, cin_p), 0), _normal(rng, (npix, cout_p), 0)          # padded channels hold values too
    w = _normal(rng, (cout, cin, 3, 3), 0, zeros=0.1)
    bias = torch.zeros(cout_p, dtype=torch.float32, device=DEV)
    bias[:cout] = _normal(rng, (cout,), 0, zeros=0.0)
    seg = tuple(segs[0]) if len(segs) == 2 else (cin, cin_p)
    kmap, nmap = (cin,) + seg, (cout, cout, cout_p)
    kl = _wg_map(kmap, cin_p)
    yref, ymag = _conv_ref(x.double()[:, kl], w, shape, False)
    gref, gmag = _conv_ref(gz.double()[:, :cout], w, shape, True)
    res = dict(shape=shape, g=g, x=x, gz=gz, w=w, bias=bias, segs=segs, cout=cout, cin_p=cin_p, cout_p=cout_p, kl=kl,
               yref=(yref + bias.double()[:cout]).clamp_min(0), gref=gref)
    # the same results through the reference's own Winograd algebra, in float64: the matrices and layouts reproduce the direct sums
    for a, Np, nm, Kp, km, dg, ref, mag, live, key in ((x, cout_p, nmap, cin_p, kmap, False, yref, ymag, slice(0, cout), 'My'),
                                                       (gz, cin_p, kmap, cout_p, nmap, True, gref, gmag, kl, 'Mg')):
        V = _xform(form, 'BT', a, shape, g)
        U, _ = _pack_ref(form, w, Np, nm, Kp, km, dg, None)
        U = U * _sign('pre%d' % form, form)[None, :, None]                      # the true planes
        Y = _out_transform(form, _plane_products(V, U), g, shape).reshape(npix, Np)
        M = _out_transform(form, _plane_products(V, U, True), g, shape, True).reshape(npix, Np)
        assert bool(((Y[:, live] - ref).abs() <= 2.0 ** -40 * (M[:, live] + mag + 1)).all()), 'the Winograd matrices do not reproduce the direct sum'
        dead = torch.ones(Np, dtype=torch.bool, device=DEV)
        dead[live] = False
        assert not bool(Y[:, dead].any()) and not bool(M[:, dead].any())
        res[key] = M[:, live]
    return res


@pytest.mark.parametrize('form,i', [(form, i) for form in (24, 44) for i in range(len(E2E))], ids=lambda v: str(v))
def test_end_to_end(C, form, i):
    L, lib, s = C._lib, C._lib.load(), C._lib.stream_ptr()
    ex = _e2e_expect(form, i, 9000 + 10 * form + i)
    B, H, W = shape = ex['shape']
    f, g, npix, cin_p, cout_p, cout, mult = PRE[form], ex['g'], B * H * W, ex['cin_p'], ex['cout_p'], ex['cout'], E2E[i][3]
    tune = E2E_TUNE[i]
    tn, P = _tuning(C, tune), f['P']
    plf, plg = _fwd_plan(form, shape, cin_p, cout_p, _td(tune)), _fwd_plan(form, shape, cout_p, cin_p, _td(tune))
    what = f'winograd{form} end to end {shape} {ex["segs"]} -> {cout} [forward RAGGED {plf["ragged"]} nk {plf["nk"]} grid {plf["grid"]}; gradient nk {plg["nk"]}]'
    pre, conv = f'clamd_winograd{form}_', f'clamd_conv3x3_winograd{form}_pre'
    nvx, nvg = g['ntm'] * (cin_p // 8) * P * 256, g['ntm'] * (cout_p // 8) * P * 256
    assert getattr(lib, pre + 'input_elems')(B, H, W, cin_p) == nvx and getattr(lib, pre + 'input_elems')(B, H, W, cout_p) == nvg
    assert L.stat_rows(getattr(L, f['op']), B, H, W, cin_p, cout_p, 0, False, tn) == plf['rows'] and not plf['per_wg']
    xa, ga = _half(C, npix, cin_p, 1, 0, ex['x']), _half(C, npix, cout_p, 1, 0, ex['gz'])

    def launch():
        wf, wd, vx, vg = Rows(P * cout_p * cin_p), Rows(P * cin_p * cout_p), Rows(nvx), Rows(nvg)
        y, gx, st = _half(C, npix, cout_p, mult, 0), _half(C, npix, cin_p, mult, 0), Rows(plf['rows'], 2, cout_p)
        tab = C.ops.WinoPackTable(P)
        tab.conv3x3(ex['w'], wf.view, wd.view, ex['segs'], cout)
        tab.finalize(DEV).run()
        L.call(pre + 'transform_input', xa.ptr, xa.ldc, None, None, vx.ptr, B, H, W, cin_p, s)
        L.call(conv, vx.ptr, wf.ptr, L.ptr(ex['bias']), y.ptr, y.ldc, st.ptr, plf['rows'], B, H, W, cin_p, cout_p, 1, tn.ref(), s)
        L.call(pre + 'transform_input', ga.ptr, ga.ldc, None, None, vg.ptr, B, H, W, cout_p, s)
        L.call(conv, vg.ptr, wd.ptr, None, gx.ptr, gx.ldc, None, 0, B, H, W, cout_p, cin_p, 0, tn.ref(), s)
        _sync()
        return [wf, wd, vx, vg, y, gx, st]

    wf, wd, vx, vg, y, gx, st = _twice(what, launch)
    for name, t in (('wf', wf), ('wd', wd), ('V of x', vx), ('V of gz', vg), ('the rows', st)):
        assert not bool(torch.isnan(t.view).any()), f'{what}: {name} holds NaN (an element was not written)'
    assert torch.equal(_raw(xa.buf), _raw(xa.before)) and torch.equal(_raw(ga.buf), _raw(ga.before)), what + ': an input was written'
    n = FORM[form]['nV'] + f['nU'] + f['nA']
    key = f'conv3x3_winograd{form}_pre'
    yv, gv = y.get(), gx.get()
    assert not bool(torch.isnan(yv).any()) and not bool(torch.isnan(gv).any()), what + ': an output element was not written'
    _per_element(what + ' forward', key + ' forward', yv[:, :cout], ex['yref'],
                 _gamma(n + cin_p + 1) * UNIT.get(key, EPS) / EPS * (ex['My'] + ex['bias'].double()[:cout].abs()) + 2.0 ** -40 * ex['My'])
    _per_element(what + ' data gradient', key + ' data gradient', gv[:, ex['kl']], ex['gref'],
                 (_gamma(n + cout_p) * UNIT.get(key, EPS) / EPS + 2.0 ** -40) * ex['Mg'])
    assert not bool(yv[:, cout:].any()), what + ': a padded channel of y is not zero'
    dead = torch.ones(cin_p, dtype=torch.bool, device=DEV)
    dead[ex['kl']] = False
    assert not bool(gv[:, dead].any()), what + ': a padded channel of the input gradient is not zero'
    # the rows against the sums of what the launch stored (one workgroup per item: row tm = tile block tm)
    yd = yv.double().view(B, H, W, cout_p)
    S1, SA, S2 = (_block_sums(t, g, shape) for t in (yd, yd.abs(), yd * yd))
    ns = _gamma(_stat_n(form, plf))
    _per_element(what + ' first moments', key + ' rows', st.view[:, 0], S1, ns * SA)
    _per_element(what + ' second moments', key + ' rows', st.view[:, 1], S2, ns * S2)


# -------------------------------------------------------------------------------------------------- what needs no device (test_host_cpu.py)
def check_wino_fwd_plans():
    """The rows reach every instantiation and every grid class the docstring lists, from this file's copies of the launcher's rules."""
    for form in (24, 44):
        rows = _small_rows(form)
        plans = [(r, _fwd_plan(form, SH[form][r[0]], r[1], r[2], TUNE0)) for r in rows]
        for txn in (4, 8):
            for ragged in (False, True):
                ps = [r for r, p in plans if p['TXN'] == txn and p['ragged'] == ragged]
                assert {r[1] for r in ps} == set(KP[form]), (form, txn, ragged)
                assert {r[3] for r in ps} == {1, 2} and len({r[2] for r in ps}) >= 2, (form, txn, ragged)
        assert {p['nk'] for _, p in plans} == ({2, 3, 8} if form == 44 else {8, 12})
        assert {r[2] for r in rows} == set(NP) and {r[4] for r in rows} == {0, 5} and {r[5] for r in rows} == {'relu', 'bias+stats'}
        assert all(not p['per_wg'] and p['rows'] == p['tiles'] for _, p in plans)
        assert max(p['tiles'] for _, p in plans) >= 4 and min(p['tiles'] for _, p in plans) == 1
        assert KP[form][0] == PRE[form]['cin_min'] and KP[form][1] == PRE[form]['cin_min'] + PRE[form]['cin_mult']
        si, Kp, Np = LOW[form]
        assert Kp == KP[form][0] and _fwd_plan(form, SH[form][si], Kp, Np, TUNE0)['ragged']
        # the persistent case
        shape, Kp, Np = PERSIST[form]
        assert Kp == KP[form][0]
        dflt, res, one, b1, b2 = (_fwd_plan(form, shape, Kp, Np, _td(t)) for t in PTUNE)
        assert dflt['tiles'] == 27 and dflt['slabs'] == 10 and dflt['nblk'] == 270 and not dflt['ragged'] and dflt['TXN'] == 8
        assert dflt['per_wg'] and dflt['grid'] == 256 and dflt['rows'] == 256 and dflt['busiest'] == 2
        assert res['per_wg'] and res['grid'] == 128 and res['rows'] == 128 and res['busiest'] == 3
        assert any(len({tn for tn, _ in its}) > 1 for its in res['items']), 'a slab change inside a workgroup'
        assert any(len(its) == 3 and its[0][0] != its[1][0] for its in res['items']), 'a fold and a flush, then a flush onto the same row'
        assert not one['per_wg'] and one['grid'] == 270 and one['rows'] == 27 and one['busiest'] == 1
        assert b1['band'] == 1 and b2['band'] == 2 and dflt['band'] in (1, 2) and b1['items'] != b2['items']
        assert wino_band(27, 10, 1.0, 1.0, 4) == 2 and wino_band(27, 8, 1.0, 1.0, 32) == 8 and wino_band(1, 3, 1.0, 1.0, 0) == 1
        # end to end: forward and data gradient of every row are launches the entry point accepts, ragged and whole, wide and narrow
        eps = [(_fwd_plan(form, SH[form][r[0]], sum(s[1] for s in r[1]), _cpad(r[2]), _td(t)),
                _fwd_plan(form, SH[form][r[0]], _cpad(r[2]), sum(s[1] for s in r[1]), _td(t))) for r, t in zip(E2E, E2E_TUNE)]
        assert {(a['TXN'], a['ragged']) for a, _ in eps} >= {(8, True), (4, True), (8, False)}
        assert any(len(r[1]) == 2 for r in E2E) and any(r[2] < _cpad(r[2]) for r in E2E) and {r[3] for r in E2E} == {1, 2}
    kinds = {(len(c[1]) == 2, c[0] < _cpad(c[0]), sum(s[0] for s in c[1]) < sum(s[1] for s in c[1]), c[2], c[3], c[4]) for t in PACK for c in t}
    assert any(k[0] and k[4] for k in kinds) and any(k[0] and k[5] for k in kinds), 'two-segment K (forward) and two-segment N (data gradient)'
    assert any(k[1] for k in kinds) and any(k[2] for k in kinds) and any(not (k[0] or k[1] or k[2]) for k in kinds)
    assert any(k[3] for k in kinds) and {sum(c[3] + c[4] for c in t) for t in PACK} >= {2, 3}


def check_wino_fwd_exact_conditions():
    """The 2^24 conditions of every exact case -- every element of Y, the first moments of every row of every plan, the second moments of the
    low-magnitude cases -- from the references alone (no library call, no device): _fwd_expect and _fwd_stats_expect assert them."""
    for form in (24, 44):
        for i, (si, Kp, Np, _, npad, third) in enumerate(_small_rows(form)):
            ex = _fwd_expect(form, SH[form][si], Kp, Np, npad, 6000 + 100 * form + i)
            pl = _fwd_plan(form, SH[form][si], Kp, Np, TUNE0)
            for variant in ('full', 'bias+stats'):
                _fwd_stats_expect(form, ex, pl, _fwd_image(ex, variant))
        si, Kp, Np = LOW[form]
        ex = _fwd_expect(form, SH[form][si], Kp, Np, 0, 6900 + form, low=True)
        assert _fwd_stats_expect(form, ex, _fwd_plan(form, SH[form][si], Kp, Np, TUNE0), _fwd_image(ex, 'full'))[2]
        shape, Kp, Np = PERSIST[form]
        ex = _fwd_expect(form, shape, Kp, Np, 5, 7000 + form)
        for tune in PTUNE:
            _fwd_stats_expect(form, ex, _fwd_plan(form, shape, Kp, Np, _td(tune)), _fwd_image(ex, 'full'))
        for i in range(len(E2E)):
            _e2e_expect(form, i, 9000 + 10 * form + i)           # float64: the Winograd algebra of the reference IS the direct sum


def check_wino_fwd_layout_helpers():
    """The U index helpers round-trip and agree with the vectorised placement; _untile puts every tile where _tile_origin says."""
    for P, Kp, Np in ((24, 64, 64), (36, 16, 192), (36, 24, 128)):
        n = Kp * P * Np
        lay = _u_layout(torch.arange(n, dtype=torch.float64).view(Kp, P, Np))
        for off in list(range(0, n, max(1, n // 997))) + [n - 1]:
            c, pl, nn = _u_unindex(off, Np, P)
            assert _u_index(c, pl, nn, Np, P) == off and int(lay[off]) == (c * P + pl) * Np + nn
    for form in (24, 44):
        for shape in SH[form] + [PERSIST[form][0]]:
            g = _geom(form, shape)
            B, H, W = shape
            th = g['th']
            tiles = torch.arange(g['Tp'] * th * 4, dtype=torch.float64).view(g['Tp'], th, 4, 1)
            img = _untile(tiles, g, shape)
            assert img.shape == (B, H, W, 1)
            seen = torch.zeros(B, H, W, dtype=torch.bool)
            for t in range(g['Tp']):
                b, y0, x0 = _tile_origin(g, t)
                if y0 < H and x0 < W:
                    assert torch.equal(img[b, y0:y0 + th, x0:x0 + 4, 0], tiles[t, :, :, 0]), (form, shape, t)
                    seen[b, y0:y0 + th, x0:x0 + 4] = True
            assert bool(seen.all())
