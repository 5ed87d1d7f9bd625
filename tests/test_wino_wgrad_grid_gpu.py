"""GPU: the Winograd weight-gradient kernels, per element, over the grid their launchers can start -- clamd_wgrad_winograd (F(2x2), csrc/wino.hip),
clamd_wgrad_winograd24 (F(2x4), wino24_wgrad.hip), clamd_wgrad_winograd24_pre (wino24g.hip), clamd_wgrad_winograd44_pre (wino44g.hip), the two
input transforms clamd_winograd{24,44}_transform_input and the two gradient transforms clamd_wgrad_winograd{24,44}_pre_transform.

Every case calls the C ABI directly.  Every buffer a launch writes -- V (exactly clamd_winograd{24,44}_input_elems floats), Yt (exactly
..._pre_operand_elems), the workspace (exactly the bytes this file's copy of the plan needs) and out [R][C][3][3] -- sits between guard bands
that must come back bit-identical, is pre-filled with NaN, and every launch runs twice and must give the same bits (_twice).  V and Yt hold
no NaN afterwards; a workspace slot the plan does not use is still NaN; NaN in out means the reduce read something nobody wrote.  One byte
less of workspace is refused (status < 0, "workspace too small", out untouched), so the plan a row is listed for is the plan that ran.

References are float64 torch evaluations on the same host-generated inputs.  The gradient is grid_util._wgrad_ref: the direct sum over
pixels of gz[p, r] x[p + (ky - 1, kx - 1), c], zero outside the image -- never F.conv2d, the oracle, another libclamd call or Winograd
algebra.  The intermediates are float64 contractions with the matrices of the kernel comments (B4^T, B6^T, A4, A6 of grid_util; G4, G6 for the
bounds) placed by the documented layouts: V [tile block][Cp / 8][plane = 6 i + j][2][32][4], Yt [plane][Tp][Rp], tile t = 32 block + tile
in block, blocks 8 x 32 / 16 x 16 pixels (F(2x4)) and 16 x 32 / 32 x 16 (F(4x4)), blocks x fastest.  _expect asserts in float64 that
G^T (sum_t Yt x V) G of those matrices IS the direct sum, so the matrices are checked without any kernel.  What the kernels store negated
(SIGN): V row i = 2 of the pre-transformed F(2x4) form; planes i = 2, 3 of both in-kernel kernels' slabs, and column j = 3 of F(2x2)'s.

Exact-integer cases (activations in [-4, 4], gradients in {-2 .. 2}, about a quarter zeros; scale in {-2 .. 2}, shift in {-3 .. 3}): both
transforms have integer coefficients, so V, Yt and every plane partial sum are integers, exact in fp32 in any order while the sum of the
absolute terms stays below 2^24 -- asserted from the reference for every element of V and Yt (|M| |d| |M|^T) and every plane element
(sum_t |Yt| |V|), here and without a device by test_host_cpu.py (check_wino_exact_conditions).  Then
  V, Yt            EQUAL the integer reference as numbers (a zero's sign is free), the all-zero tiles of a ragged block included; with
                   scale / shift: the transform of the explicitly computed x * scale + shift, zero padding applied after the affine
  split-K          every slab [split][plane][Rp][Cp] equals the sum over ITS tile range [split per, min(Tp, (split + 1) per))
  stream-K plans   the slots written are exactly slot < (slots of the item) for every (plane, block) item; an item's slots add up to the
                   integer total; wave-level plan: the reduced planes behind the slots equal it too
  in-kernel forms  the slabs [split][i][r][c][j] add up to the integer total (F(2x4): the two floats of padding behind j = 5 stay NaN)
  F(2x2) out       EQUALS the exact result bit for bit (G4 has only halves; asserted: |G|^T |U| |G| < 2^22)
  F(2x4), F(4x4)   |out - reference| <= n_G u |G|^T |U| |G|, u = 2^-24, U the exact plane sums (the reference is the float64 direct sum): a bound
                   that does not grow with the pixels.  n_G = roundings on the longest path of the reduce kernels, every operation and every
                   rounded constant counted once: t = U0 + 0.5 (U1 + U2) is 2 (the halving is exact); G6's o0 = 0.25 t0 - c s12 + c' s34 is
                   s12 (1), the constant 1/6 (1), its product (1), the subtraction (1), the last addition (1) = 5.  F(2x4): 2 + 5 = 7,
                   F(4x4): 5 + 5 = 10 (F(2x2): 2 + 2 = 4, not needed).  The compiler may contract some into fmas: fewer roundings, same bound
Random cases (_normal, fp32): |out - reference| <= (n_V + n_Y + 1 + T + n_S + n_G) u M + 2^-50 sum |a b|, M = |G|^T (sum_t |A||dY||A|^T x
|B|^T|d||B|) |G|; n_V / n_Y = roundings of the two transforms (an fma is one): F(2x2) 2 / 2 (one fma down the rows, one add along the
columns), F(2x4) 3 / 3 (rows 1, columns 2: fma(4, t0, fma(-5, t2, t4)); (g0 + g2) + (g1 + g3)), F(4x4) 4 / 4; T = Winograd tiles summed (Tp,
padding tiles included); n_S = nsplit + 2 (pre split-K: the zero start and two shuffle steps) or + 3 (in-kernel reduce) or the largest slot
count.  V and Yt: n_V (+ 1 with scale / shift) and n_Y times u times |M| |d| |M|^T.  UNIT is empty: nothing exceeds u = 2^-24.
Worst error / bound on the MI355X in one run of this file (188 cases, one test per row, in 14.9 s; exact cases: equality except where a ratio is given):
                                       exact out   random out   |  transforms (random)
  wgrad_winograd (F(2x2))              equal       0.011        |  winograd24_transform_input        0.890
  wgrad_winograd24                     0.250       0.008        |  winograd44_transform_input        0.744
  wgrad_winograd24_pre split-K         0.263       0.007        |  wgrad_winograd24_pre_transform    0.797
  wgrad_winograd24_pre stream-K        0.253       0.008        |  wgrad_winograd44_pre_transform    0.670
  wgrad_winograd24_pre wave-level      0.237       0.004
  wgrad_winograd44_pre split-K         0.157       0.003
  wgrad_winograd44_pre stream-K        0.141       0.004
  wgrad_winograd44_pre wave-level      0.133       0.002
(The random gradient bound is loose because T u M charges every tile a worst-case rounding of the whole magnitude; the exact cases are the sharp ones.)

Paths (check_wino_wgrad_plans asserts them from this file's copies of wino_wgrad_nsplit, w24g_wg_plan_planes, w24g_sk_plan, w24g_skw_plan,
the phs choice and wave_level / streamk; no device).  Shapes: F(2x4) 1 x 8 x 32 (one whole wide block), 1 x 10 x 36 (ragged, four blocks),
2 x 18 x 20 (narrow, ragged, Tp = 256), 2 x 16 x 16 (narrow, whole); F(4x4) 1 x 16 x 32, 1 x 20 x 36, 2 x 36 x 20 (Tp = 256), 1 x 32 x 16;
in-kernel forms 1 x 8 x 16 (one pixel tile), 1 x 16 x 32 (four whole tiles), 2 x 10 x 20 (8 ragged tiles), 1 x 18 x 36 (9 ragged tiles).
  wino_wgrad_kernel<RAGGED>, wino24_wgrad_kernel<RAGGED>   INK rows: both RAGGED values with Rp and Cp in 32 / 64 / 96 each (the n < Rp guards of
                   a 64 x 64 and a 64 x 32 block), nsplit 1, 2, 3, 4, 5, 8 through wgrad_blocks (the reduce's four split phases), 5 + 4 and
                   3 + 3 + 2 tiles (a short last split), cu_reserve halving the target
  wino24_xform_kernel<4|8>, wino44_xform_kernel<4|8>       XFORM rows: Cp 8, 40 (a lone chunk in the second 32-channel group), 64, x the second half of
                   a concat buffer, with and without scale / shift, W < 32 and >= 32, whole and ragged blocks; and Cp 128 .. 512 in the PRE rows
  wino24g_wgrad_xform_kernel<4|8>, wino44g_wgrad_xform_kernel<4|8>   PRE rows; gz as the second half of a buffer of twice the pitch; the two-call
                   form (..._pre_transform, then gz == NULL) gives the same bits of Yt, workspace and out
  wino24g_wgrad_kernel + wino24g_wgrad_reduce_kernel<1|2|4> / wino44g_wgrad_reduce_kernel<1|2|4>   wgrad_streamk 0: nsplit 1 .. 8; a last split shorter than
                   per (F(2x4): 6 x 48 of 256 at cu_reserve 77; F(4x4): 3 x 48 of 128 and 3 x 96 of 256 at cu_reserve 128)
  wino24g_wgrad_sk_kernel + wino_sk_reduce_kernel<24|36>   wgrad_streamk 2: items of 1, 2, 4, 6, 8 slots, a workgroup stopping inside an item
                   (S % Q != 0), cu_reserve 128 changing Q (16 -> 24, 24 -> 40); the default wgrad_streamk 1 on both sides of its switch
  wino24g_wgrad_skw_kernel + wino_skw_sum_kernel + wino_sk_reduce_kernel   128 x 128, 128 x 256, 256 x 128, 384 x 256 (with wgrad_streamk 0: ignored there)
  channel maps     identity, R padded, C padded, two-segment C (a concat input), two-segment R, in the INK and the PRE rows
Seven PRE rows (five for F(4x4)) use 512 channels, past the 384 of the other rows, because no smaller size reaches their path: cu_reserve is
at most 128, so the default plan's switch (planes x blocks x 8 >= 3 x usable CUs) needs at least two 256 x 256 blocks (512 x 256); an item
with ONE slot under wgrad_streamk 2 needs Q >= S, i.e. >= 72 items of 16 k-steps on 128 CUs: 512 x 256 with 36 planes, 512 x 512 with 24;
reduce<1> (nsplit 1) is chosen at 72 items on 193 CUs (F(4x4), 512 x 256) and only from 96 items on with 24 planes.  The two 512 x 512 rows
therefore run for F(2x4) alone (_pre_rows).
Left unreached: the 2^32-byte operand and 2^31 / 2^30-byte image limits; a second trip of the grid-stride loops of the transform and reduce
kernels (grids are capped at 2^20 / 8192 / 16384 workgroups: over 2 M gradient elements); nquad > 65536 in the phs choice (more than
512 x 512 channels); a refusal's effect on Yt (the stream-K launchers check the workspace AFTER the gradient transform is queued: a short
workspace leaves out untouched but Yt written -- harmless, and not asserted either way).
Mutation check (scratch builds, not committed): dropping the last k-step of one stream-K workgroup fails "slot sums" (and both random
stream-K cases); t_end = t_begin + tiles_per_split - 2 for the last split fails "slab 1"; (1/12)(1 + 2^-16) on the centre tap of
wino24g_wgrad_reduce_kernel fails the exact out bound at error / bound 4.4 and passes every random bound and the old oracle bound (2e-5)
"""
import numpy as np
import pytest
import torch

from grid_util import (DEV, EPS, FORM, Rows, _expect_rows, _expect_vals, _geom, _half, _ints, _m, _normal, _per_element, _planes_n, _raw, _sign,
                       _tile_of, _tile_origin, _twice, _v_index, _v_layout, _v_unindex, _wg_map, _wgrad_ref, _xform, _yt_index)

pytestmark = pytest.mark.gpu

UNIT = {}                                      # (entry point and plan) -> u of the random bound where EPS is exceeded (none is: see above)
NCU = 256                                      # compute units of the MI355X (asserted against the device by the fixture)
RING = 8                                       # W24G_D: k-steps (of two tiles) the plane GEMMs' load stream runs ahead

@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    C._lib.load()
    assert torch.cuda.get_device_properties(0).multi_processor_count == NCU
    return C


def _sync():
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------ plane sums
def _usum(Y, V, t0=0, t1=None):
    """Y [T, P, Rp], V [T, P, Cp] -> float64 [P, Rp, Cp]: the plane sums over tiles [t0, t1)."""
    return torch.bmm(Y[t0:t1].permute(1, 2, 0), V[t0:t1].permute(1, 0, 2))


def _gug(form, U, absolute=False):
    """[P, Rp, Cp] -> G_rows^T U G_cols as [Rp, Cp, 3, 3]."""
    ni, nj = _planes_n(form)
    Gr, Gc = (_m(m, absolute) for m in FORM[form]['G'])
    return torch.einsum('ik,ijrc,jl->rckl', Gr, (U.abs() if absolute else U).view(ni, nj, *U.shape[1:]), Gc)


# ----------------------------------------------------------------------------------------------------- the launchers' rules, in Python
TUNE0 = dict(wgrad_blocks=512, cu_reserve=0, wgrad_streamk=1)


def _td(tune):
    return dict(TUNE0, **tune)


def _tuning(C, tune):
    tn = C._lib.Tuning(**tune)
    assert {k: v for k, v in tn.as_dict().items() if k in TUNE0} == _td(tune)
    return tn


def _cus(td):
    """clamd_usable_cus."""
    return max(8, NCU - max(td['cu_reserve'], 0))


def wino_wgrad_nsplit(ntiles, blocks, td):
    nsplit = min(max(1, (td['wgrad_blocks'] // 2) * _cus(td) // NCU // blocks), ntiles)
    per = -(-ntiles // nsplit)
    return -(-ntiles // per), per


def _ink_plan(form, shape, Rp, Cp, td):
    """clamd_wgrad_winograd / clamd_wgrad_winograd24: 8 x 16 pixel tiles, 64 x 64 / 64 x 32 channel blocks."""
    B, H, W = shape
    ntiles = -(-W // 16) * -(-H // 8) * B
    blocks = -(-Rp // 64) * -(-Cp // (64 if form == 22 else 32))
    nsplit, per = wino_wgrad_nsplit(ntiles, blocks, td)
    return dict(ntiles=ntiles, blocks=blocks, nsplit=nsplit, per=per, ragged=bool(H % 8 or W % 16), J=4 if form == 22 else 8)


def w24g_wg_plan_planes(Tp, Rp, Cp, P, cus):
    """The split-K plan of the plane GEMM: the split count with the smallest modelled time (the same double arithmetic) -> (nsplit, per)."""
    quant, nb = 2 * RING, P * (Rp // 256) * (Cp // 256)
    max_split = max(1, min(3 * NCU // nb, Tp // quant))
    best, best_ns, best_per = 0.0, 1, Tp
    for ns in range(1, max_split + 1):
        per = -(-(-(-Tp // ns)) // quant) * quant
        n = -(-Tp // per)
        if n != ns:
            continue
        rounds = float((nb * n + cus - 1) // cus)
        cycles = rounds * (per // 2 * 1024.0 + 28000.0)
        t = cycles / 2.3e9 + float(nb) * n * 262144.0 / 4.5e12
        if best == 0 or t < best:
            best, best_ns, best_per = t, n, per
    return best_ns, best_per


def _sk_plan(Tp, items, units):
    """w24g_sk_plan (units = workgroups, items of 256 x 256) and w24g_skw_plan (units = 4 waves per CU, items of 128 x 128)."""
    S = Tp // 2
    total = items * S
    Q = -(-(-(-total // units)) // RING) * RING
    return dict(S=S, Q=Q, items=items, nunits=-(-total // Q), max_slots=-(-S // Q) + 1)


def w24g_sk_plan(Tp, Rp, Cp, P, cus):
    return _sk_plan(Tp, P * (Rp // 256) * (Cp // 256), cus)


def w24g_skw_plan(Tp, Rp, Cp, P, cus):
    return _sk_plan(Tp, P * (Rp // 128) * (Cp // 128), 4 * cus)


def _item_slots(pl):
    """Slots per item: item b is touched by units floor(b S / Q) .. floor(((b + 1) S - 1) / Q)."""
    S, Q = pl['S'], pl['Q']
    return [((b + 1) * S - 1) // Q - (b * S) // Q + 1 for b in range(pl['items'])]


def _pre_plan(form, Tp, Rp, Cp, td):
    """wino_pre_wgrad: wave_level / streamk / the split plan and the phs choice -> dict(kind, slots (workspace slabs), ...)."""
    P, cus = 24 if form == 24 else 36, _cus(td)
    if Rp % 256 or Cp % 256:
        pl = w24g_skw_plan(Tp, Rp, Cp, P, cus)
        return dict(pl, kind='skw', blk=128, slots=pl['max_slots'] + 1, P=P)
    if td['wgrad_streamk'] == 2 or (td['wgrad_streamk'] == 1 and P * (Rp // 256) * (Cp // 256) * 8 >= 3 * cus):
        pl = w24g_sk_plan(Tp, Rp, Cp, P, cus)
        return dict(pl, kind='sk', blk=256, slots=pl['max_slots'], P=P)
    nsplit, per = w24g_wg_plan_planes(Tp, Rp, Cp, P, cus)
    nquad = Rp * Cp // 4
    phs = 4 if (nsplit >= 4 and nquad <= 65536) else 2 if (nsplit >= 2 and nquad <= 131072) else 1
    return dict(kind='split', nsplit=nsplit, per=per, phs=phs, slots=nsplit, P=P)


# ----------------------------------------------------------------------------------------------------------------------------- inputs
def _acts(rng, shape, exact):
    return _ints(rng, shape, 4, 0.15) if exact else _normal(rng, shape, 0)


def _grads(rng, shape, exact):
    return _ints(rng, shape, 2, 0.07) if exact else _normal(rng, shape, 0, zeros=0.1)


def _id(p):
    return (p, p, p)


def _expect(form, exact, shape, Rp, rmap, Cp, cmap, seed, g):
    """Everything a weight-gradient launch is compared with, from the inputs alone (no library call): gz, x (padded channels hold values too),
    the float64 planes V [T, P, Cp] and Y [T, P, Rp] with the TRUE matrices in tile order (g: the pre forms' block order), the plane sums U,
    the direct-sum reference, M = |G|^T (sum_t |A||dY||A|^T x |B|^T|d||B|) |G|.  Exact cases assert the 2^24 conditions per plane element."""
    B, H, W = shape
    rng = np.random.default_rng(seed)
    gz, x = _grads(rng, (B * H * W, Rp), exact), _acts(rng, (B * H * W, Cp), exact)
    V, Y = _xform(form, 'BT', x, shape, g), _xform(form, 'A', gz, shape, g)
    aV, aY = _xform(form, 'BT', x, shape, g, True), _xform(form, 'A', gz, shape, g, True)
    U, aU = _usum(Y, V), _usum(aY, aV)
    ref, mag = _wgrad_ref(0, gz, x, shape)
    ref, mag = ref.view(Rp, Cp, 3, 3), mag.view(Rp, Cp, 3, 3)
    M = _gug(form, aU, True)
    # the reference's own algebra: G^T U G of the matrices above IS the direct sum (float64: far below one fp32 ulp of anything here)
    assert bool(((_gug(form, U) - ref).abs() <= 2.0 ** -40 * (M + 1)).all()), 'the transform matrices do not reproduce the direct sum'
    if exact:
        assert float(aV.max()) < 2 ** 24 and float(aY.max()) < 2 ** 24, 'a transform partial sum reaches 2^24'
        assert float(_usum(Y.abs(), V.abs()).max()) < 2 ** 24, 'a plane element\'s sum of absolute terms reaches 2^24'
        if form == 22:          # G4 has only halves: every value of the reduce is a multiple of 1/4 below 2^22
            assert float(_gug(form, U, True).max()) < 2 ** 22
    rl, cl = _wg_map(rmap, Rp), _wg_map(cmap, Cp)
    live = lambda t: t[rl][:, cl].reshape(len(rl), len(cl), 9)
    return dict(gz=gz, x=x, V=V, Y=Y, aV=aV, aY=aY, U=U, ref=live(ref), mag=live(mag), M=live(M), MU=live(_gug(form, U, True)), live=live)


def _check_out(what, key, form, exact, out, ex, T, nS):
    """The gradient itself.  Exact cases: F(2x2) bit for bit; F(2x4) / F(4x4) within n_G roundings of G^T U G's absolute evaluation (a bound
    that does not grow with the pixels).  Random cases: the derived bound of the module docstring."""
    f = FORM[form]
    assert not bool(torch.isnan(out.view).any()), what + ': NaN in out: a logical element was not written, or the reduce read a slot nobody wrote'
    if exact and form == 22:
        _expect_rows(what, out, ex['ref'].float())
    elif exact:
        _per_element(what, key + ' exact', out.view, ex['ref'], f['nG'] * EPS * ex['MU'])
    else:
        n = f['nV'] + f['nY'] + 1 + T + nS + f['nG']
        _per_element(what, key, out.view, ex['ref'], n * UNIT.get(key, EPS) * ex['M'] + 2.0 ** -50 * ex['mag'])


# ------------------------------------------------------------------------------------------- clamd_winograd{24,44}_transform_input
SH = {24: [(1, 8, 32), (1, 10, 36), (2, 18, 20), (2, 16, 16)], 44: [(1, 16, 32), (1, 20, 36), (2, 36, 20), (1, 32, 16)]}
#        shape  Cp  x as the n-th half  scale / shift
XFORM = [(0, 8, 1, True), (0, 40, 2, True), (0, 64, 1, False),
         (1, 40, 1, True), (1, 64, 2, True), (1, 8, 2, False),
         (2, 64, 1, True), (2, 8, 2, True), (2, 40, 1, False),
         (3, 40, 2, True), (3, 8, 1, True), (3, 64, 2, False)]


def _xform_expect(form, exact, si, Cp, affine, seed):
    """x, scale, shift and the float64 V [Tp, P, Cp] (true matrices) of x * scale + shift with the zero padding applied AFTER the affine."""
    shape = SH[form][si]
    B, H, W = shape
    rng, g = np.random.default_rng(seed), _geom(form, shape)
    x = _acts(rng, (B * H * W, Cp), exact)
    sc = (_ints(rng, (Cp,), 2, 0.0) if exact else _normal(rng, (Cp,), 0, zeros=0.0)) if affine else None
    sh = (_ints(rng, (Cp,), 3, 0.0) if exact else _normal(rng, (Cp,), 0, zeros=0.0)) if affine else None
    xa = x.double() * sc.double() + sh.double() if affine else x.double()
    xm = x.double().abs() * sc.double().abs() + sh.double().abs() if affine else x.double().abs()
    V, aV = _xform(form, 'BT', xa, shape, g), _xform(form, 'BT', xm, shape, g, True)
    if exact:
        assert float(aV.max()) < 2 ** 24
    return shape, g, x, sc, sh, V, aV


def _check_v(what, key, form, exact, v, V, aV, n):
    """The stored image against the true planes [Tp, P, Cp] (F(2x4): row 2 of B4^T negated), placed by the documented layout."""
    sg = _sign('pre%d' % form, form)[None, :, None]
    got = v.view.double()
    assert not bool(torch.isnan(got).any()), what + ': V holds NaN (an element was not written)'
    if exact:
        _expect_vals(what + ' V', got, _v_layout(V * sg))
    else:
        _per_element(what + ' V', key, got, _v_layout(V * sg), _v_layout((n * EPS + 2.0 ** -50) * aV))


def _xform_case(C, what, form, exact, si, Cp, mult, affine, seed):
    L, lib, s = C._lib, C._lib.load(), C._lib.stream_ptr()
    shape, g, x, sc, sh, V, aV = _xform_expect(form, exact, si, Cp, affine, seed)
    B, H, W = shape
    P = V.shape[1]
    nv = g['ntm'] * (Cp // 8) * P * 256
    assert getattr(lib, f'clamd_winograd{form}_input_elems')(B, H, W, Cp) == nv
    xa = _half(C, B * H * W, Cp, mult, 0, x)

    def launch():
        v = Rows(nv)
        L.call(f'clamd_winograd{form}_transform_input', xa.ptr, xa.ldc, L.ptr(sc), L.ptr(sh), v.ptr, B, H, W, Cp, s)
        _sync()
        return [v]

    v = _twice(what, launch)[0]
    assert torch.equal(_raw(xa.buf), _raw(xa.before)), what + ': the input was written'
    _check_v(what, f'winograd{form}_transform_input', form, exact, v, V, aV, FORM[form]['nV'] + (1 if affine else 0))


@pytest.mark.parametrize('form,i', [(form, i) for form in (24, 44) for i in range(len(XFORM))], ids=lambda v: str(v))
@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'random'])
def test_transform_input(C, form, i, exact):
    row = XFORM[i]
    _xform_case(C, f'winograd{form}_transform_input {"exact" if exact else "random"} {SH[form][row[0]]} {row[1:]}', form, exact, *row,
                seed=3000 + 100 * exact + i)


# ----------------------------------------------------------------------------------------------- clamd_wgrad_winograd{24,44}_pre
SPLIT, SK = dict(wgrad_streamk=0), dict(wgrad_streamk=2)


def _t(base, **kw):
    return dict(base, **kw)


#      shape Rp  (R, seg0, seg0p)  Cp  (C, seg0, seg0p)  gz as the n-th half  tuning  two calls
PRE = [(0, 256, _id(256), 256, _id(256), 1, _t(SPLIT), False),
       (1, 256, (200, 200, 256), 256, _id(256), 2, _t(SPLIT), False),                     # R padded
       (1, 256, _id(256), 256, (230, 230, 256), 1, _t(SPLIT, cu_reserve=128), True),      # C padded
       (2, 256, _id(256), 256, (200, 100, 128), 1, _t(SPLIT), False),                     # two-segment C (a concat input)
       (2, 256, (200, 100, 128), 256, _id(256), 1, _t(SPLIT, cu_reserve=128), False),     # two-segment R
       (3, 256, _id(256), 256, _id(256), 1, _t(SPLIT, cu_reserve=100), True),
       (2, 256, _id(256), 256, _id(256), 1, _t(SPLIT, cu_reserve=77), False),               # F(2x4): 6 splits of 48 tiles, the last one 16
       (0, 512, _id(512), 512, _id(512), 1, _t(SPLIT), False),                             # F(2x4) only: 96 items, one split, reduce<1>
       (0, 256, _id(256), 256, (200, 100, 128), 2, _t(SK), False),                        # stream-K, S = 16
       (1, 256, (200, 200, 256), 256, _id(256), 1, _t(SK), True),
       (2, 256, _id(256), 256, _id(256), 1, _t(SK), False),                               # Tp = 256: items of many slots
       (2, 256, _id(256), 256, (230, 230, 256), 1, _t(SK, cu_reserve=128), False),        # a reserve that changes Q
       (0, 512, _id(512), 256, _id(256), 1, _t(SK, cu_reserve=128), False),               # 512 channels: see the docstring (one-slot items)
       (0, 512, _id(512), 512, _id(512), 1, _t(SK, cu_reserve=128), False),               # F(2x4) only: Q = S = 16, one slot per item
       (3, 512, _id(512), 256, _id(256), 1, dict(cu_reserve=128), False),                 # the default plan on both sides of its switch
       (3, 512, _id(512), 256, _id(256), 1, dict(cu_reserve=127), False),
       (3, 512, _id(512), 256, _id(256), 1, dict(cu_reserve=64), False),
       (3, 512, _id(512), 256, _id(256), 1, dict(cu_reserve=63), False),
       (0, 128, _id(128), 128, _id(128), 1, dict(), False),                               # the wave-level plan
       (1, 128, (100, 100, 128), 256, (200, 100, 128), 2, dict(), True),
       (3, 256, (200, 100, 128), 128, (100, 100, 128), 1, dict(cu_reserve=128), False),
       (2, 384, _id(384), 256, _id(256), 1, dict(), False),
       (1, 384, (300, 300, 384), 256, _id(256), 1, dict(wgrad_streamk=0, cu_reserve=77), False)]


def _pre_rows(form):
    """(index, row) of the PRE rows a form runs: the 512 x 512 rows are for F(2x4) alone, whose 24 planes reach reduce<1> and a one-slot
    stream-K item only there; F(4x4) reaches both at 512 x 256."""
    return [(i, r) for i, r in enumerate(PRE) if not (form == 44 and r[1] == 512 and r[3] == 512)]


def _used_slots(pl, Rp, Cp):
    """[slots, P, Rp, Cp] bool: slot k of the item that owns (plane, r, c) is written (k < the item's slot count)."""
    blk, P = pl['blk'], pl['P']
    n = torch.tensor(_item_slots(pl), device=DEV).view(P, Rp // blk, Cp // blk)
    n = n.repeat_interleave(blk, 1).repeat_interleave(blk, 2)
    return torch.arange(pl['max_slots'], device=DEV).view(-1, 1, 1, 1) < n


def _pre_case(C, what, form, exact, si, Rp, rmap, Cp, cmap, gzm, tune, twocall, seed):
    L, lib, s = C._lib, C._lib.load(), C._lib.stream_ptr()
    shape = SH[form][si]
    B, H, W = shape
    g, td = _geom(form, shape), _td(tune)
    Tp, npix = g['Tp'], B * H * W
    ex = _expect(form, exact, shape, Rp, rmap, Cp, cmap, seed, g)
    pl = _pre_plan(form, Tp, Rp, Cp, td)
    P, kind = pl['P'], pl['kind']
    plan = {'split': 'split-K', 'sk': 'stream-K', 'skw': 'wave-level stream-K'}[kind]
    key = f'wgrad_winograd{form}_pre {plan}'
    what = f'{what} [{plan}, Tp {Tp}, ' + (f'nsplit {pl["nsplit"]} per {pl["per"]} reduce<{pl["phs"]}>]' if kind == 'split' else
                                           f'S {pl["S"]} Q {pl["Q"]}, slots per item {sorted(set(_item_slots(pl)))}]')
    tn = _tuning(C, tune)
    pre, wg = f'clamd_winograd{form}_', f'clamd_wgrad_winograd{form}_pre'
    nv, ny, slab = g['ntm'] * (Cp // 8) * P * 256, P * Tp * Rp, P * Rp * Cp
    need = pl['slots'] * slab
    assert getattr(lib, pre + 'input_elems')(B, H, W, Cp) == nv and getattr(lib, wg + '_operand_elems')(B, H, W, Rp) == ny
    assert 4 * need <= getattr(lib, wg + '_workspace_bytes')(B, H, W, Rp, Cp), what
    xa, ga = _half(C, npix, Cp, 1, 0, ex['x']), _half(C, npix, Rp, gzm, 0, ex['gz'])

    def launch_v():
        v = Rows(nv)
        L.call(pre + 'transform_input', xa.ptr, xa.ldc, None, None, v.ptr, B, H, W, Cp, s)
        _sync()
        return [v]

    v = _twice(what + ' input transform', launch_v)[0]
    v_bits = _raw(v.buf).clone()
    sg = _sign('pre%d' % form, form)
    _check_v(what, f'winograd{form}_transform_input', form, exact, v, ex['V'], ex['aV'], FORM[form]['nV'])
    args = (B, H, W, Rp, Cp, rmap[0], cmap[0], rmap[1], rmap[2], cmap[1], cmap[2], tn.ref(), s)

    def launch(short=0, two=False):
        yt, ws, out = Rows(ny), Rows(need), Rows(rmap[0], cmap[0], 9)
        if two:
            L.call(wg + '_transform', ga.ptr, ga.ldc, yt.ptr, B, H, W, Rp, s)
        rc = getattr(lib, wg)(None if two else ga.ptr, ga.ldc, v.ptr, yt.ptr, ws.ptr, 4 * need - short, out.ptr, *args)
        _sync()
        if short:
            msg = lib.clamd_last_error().decode()
            assert rc < 0 and 'workspace too small' in msg, (what, rc, msg)
            assert torch.equal(_raw(out.buf), _raw(out.before)), what + ': a refused launch wrote the gradient'
        else:
            L.check(rc, wg)
        return [yt, ws, out]

    launch(short=1)                                         # the plan is what this file's rules say: one byte less than its slabs is refused
    yt, ws, out = _twice(what, launch)
    if twocall:
        for a, b in zip(launch(two=True), (yt, ws, out)):
            assert a.guards_intact() and torch.equal(_raw(a.buf), _raw(b.buf)), what + ': the two-call form gives other bits'
    assert torch.equal(_raw(v.buf), v_bits), what + ': V was written'
    assert torch.equal(_raw(ga.buf), _raw(ga.before)), what + ': gz was written'
    # ---- Yt [P][Tp][Rp]
    Yk = ex['Y'].permute(1, 0, 2)
    assert not bool(torch.isnan(yt.view).any()), what + ': Yt holds NaN'
    if exact:
        _expect_vals(what + ' Yt', yt.view, Yk)
    else:
        _per_element(what + ' Yt', f'wgrad_winograd{form}_pre_transform', yt.view.view(P, Tp, Rp), Yk,
                     (FORM[form]['nY'] * EPS + 2.0 ** -50) * ex['aY'].permute(1, 0, 2))
    # ---- the workspace, in the kernels' sign convention
    Vk = ex['V'] * sg[None, :, None]
    if kind == 'split':
        wsv, nS = ws.view.view(pl['nsplit'], P, Rp, Cp), pl['nsplit'] + 2
        assert not bool(torch.isnan(wsv).any()), what + ': a slab element was not written'
        if exact:
            for k in range(pl['nsplit']):
                _expect_vals(f'{what} slab {k}', wsv[k], _usum(ex['Y'], Vk, k * pl['per'], min(Tp, (k + 1) * pl['per'])))
    else:
        ms = pl['max_slots']
        wsv, used, nS = ws.view[:ms * slab].view(ms, P, Rp, Cp), _used_slots(pl, Rp, Cp), max(_item_slots(pl))
        assert torch.equal(torch.isnan(wsv), ~used), what + ': the slots written are not the slots of the plan'
        if exact:
            _expect_vals(what + ' slot sums', wsv.masked_fill(~used, 0.0).double().sum(0), ex['U'] * sg[:, None, None])
        if kind == 'skw':
            red = ws.view[ms * slab:]
            assert not bool(torch.isnan(red).any()), what + ': the reduced planes hold NaN'
            if exact:
                _expect_vals(what + ' reduced planes', red, ex['U'] * sg[:, None, None])
    _check_out(what, key, form, exact, out, ex, Tp, nS)


@pytest.mark.parametrize('form,i', [(form, i) for form in (24, 44) for i, _ in _pre_rows(form)], ids=lambda v: str(v))
@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'random'])
def test_wgrad_pre(C, form, i, exact):
    row = PRE[i]
    _pre_case(C, f'wgrad_winograd{form}_pre {"exact" if exact else "random"} {SH[form][row[0]]} {row[1:]}', form, exact, *row,
              seed=4000 + 100 * exact + i)


# ------------------------------------------------------------------------------------ clamd_wgrad_winograd, clamd_wgrad_winograd24
ONE, S8, S9, U4 = (1, 8, 16), (2, 10, 20), (1, 18, 36), (1, 16, 32)          # 1 whole pixel tile; 8 ragged; 9 ragged; 4 whole


def _b(form, shape, Rp, Cp, target):
    """wgrad_blocks that asks for `target` splits on the whole chip."""
    return dict(wgrad_blocks=2 * target * _ink_plan(form, shape, Rp, Cp, TUNE0)['blocks'])


#       shape Rp (R, seg0, seg0p)  Cp  (C, seg0, seg0p)  gz, x as the n-th half  splits asked for, reserve
INK = [(ONE, 32, _id(32), 32, _id(32), 1, 1, 1, 0),
       (ONE, 64, (60, 60, 64), 96, _id(96), 2, 1, 3, 0),                    # asks for 3, one tile: nsplit 1
       (U4, 64, _id(64), 64, (40, 20, 32), 1, 2, 2, 0),                     # whole tiles, two-segment C, x the second half
       (U4, 96, (70, 35, 48), 32, _id(32), 1, 1, 4, 0),                     # whole tiles, two-segment R
       (U4, 32, _id(32), 64, _id(64), 1, 1, 3, 0),                          # 4 tiles in 2 + 2
       (S9, 32, (21, 21, 32), 64, (40, 40, 64), 1, 1, 1, 0),
       (S9, 64, _id(64), 32, (27, 27, 32), 2, 2, 2, 0),                     # 5 + 4 tiles: a short last split
       (S9, 96, _id(96), 96, _id(96), 1, 1, 3, 0),
       (S9, 32, _id(32), 32, _id(32), 1, 1, 5, 0),                          # 2 + 2 + 2 + 2 + 1
       (S9, 64, _id(64), 64, _id(64), 1, 1, 10, 128),                       # the reserve halves the target: 5
       (S8, 32, _id(32), 96, (72, 40, 64), 1, 1, 4, 0),
       (S8, 96, (80, 80, 96), 32, _id(32), 1, 1, 8, 0),
       (S8, 64, _id(64), 64, _id(64), 1, 1, 3, 0)]                          # 3 + 3 + 2


def _ink_tune(form, row):
    shape, Rp, _, Cp, _, _, _, target, reserve = row
    return dict(_b(form, shape, Rp, Cp, target), cu_reserve=reserve)


def _ink_case(C, what, form, exact, shape, Rp, rmap, Cp, cmap, am, bm, target, reserve, seed):
    L, lib, s = C._lib, C._lib.load(), C._lib.stream_ptr()
    B, H, W = shape
    npix = B * H * W
    tune = _ink_tune(form, (shape, Rp, rmap, Cp, cmap, am, bm, target, reserve))
    pl = _ink_plan(form, shape, Rp, Cp, _td(tune))
    ex = _expect(form, exact, shape, Rp, rmap, Cp, cmap, seed, None)
    ni, nj = _planes_n(form)
    fn = 'clamd_wgrad_winograd' + ('' if form == 22 else '24')
    key = fn[6:]
    what = f'{what} [nsplit {pl["nsplit"]} per {pl["per"]} of {pl["ntiles"]} tiles, RAGGED {pl["ragged"]}]'
    J, tn = pl['J'], _tuning(C, tune)
    need = pl['nsplit'] * 4 * Rp * Cp * J
    assert 4 * need <= getattr(lib, fn + '_workspace_bytes')(Rp, Cp), what
    ga, xa = _half(C, npix, Rp, am, 0, ex['gz']), _half(C, npix, Cp, bm, 0, ex['x'])
    args = (B, H, W, Rp, Cp, rmap[0], cmap[0], rmap[1], rmap[2], cmap[1], cmap[2], tn.ref(), s)

    def launch(short=0):
        ws, out = Rows(need), Rows(rmap[0], cmap[0], 9)
        rc = getattr(lib, fn)(ga.ptr, ga.ldc, xa.ptr, xa.ldc, ws.ptr, 4 * need - short, out.ptr, *args)
        _sync()
        if short:
            msg = lib.clamd_last_error().decode()
            assert rc < 0 and 'workspace too small' in msg, (what, rc, msg)
            assert torch.equal(_raw(out.buf), _raw(out.before)) and torch.equal(_raw(ws.buf), _raw(ws.before)), what + ': a refused launch wrote'
        else:
            L.check(rc, fn)
        return [ws, out]

    launch(short=1)
    ws, out = _twice(what, launch)
    assert torch.equal(_raw(ga.buf), _raw(ga.before)) and torch.equal(_raw(xa.buf), _raw(xa.before)), what + ': an input was written'
    wsv = ws.view.view(pl['nsplit'], ni, Rp, Cp, J)          # slabs [split][i][r][c][j], F(2x4): two floats of padding behind j = 5
    assert not bool(torch.isnan(wsv[..., :nj]).any()), what + ': a slab element was not written'
    assert bool(torch.isnan(wsv[..., nj:]).all()), what + ': the padding of a slab was written'
    if exact:
        Uk = (ex['U'] * _sign('ink%d' % form, form)[:, None, None]).view(ni, nj, Rp, Cp).permute(0, 2, 3, 1)
        _expect_vals(what + ' slab sums', wsv[..., :nj].double().sum(0), Uk)
    _check_out(what, key, form, exact, out, ex, npix // (FORM[form]['th'] * FORM[form]['tw']), pl['nsplit'] + 3)


@pytest.mark.parametrize('form,i', [(form, i) for form in (22, 24) for i in range(len(INK))], ids=lambda v: str(v))
@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'random'])
def test_wgrad_in_kernel(C, form, i, exact):
    row = INK[i]
    _ink_case(C, f'wgrad_winograd{"" if form == 22 else "24"} {"exact" if exact else "random"} {row}', form, exact, *row, seed=5000 + 100 * exact + i)


# -------------------------------------------------------------------------------------------------- what needs no device (test_host_cpu.py)
def check_wino_wgrad_plans():
    """The rows reach the paths the docstring lists, from this file's copies of the launchers' rules (no launch, no device)."""
    for form in (22, 24):
        plans = [(r, _ink_plan(form, r[0], r[1], r[3], _td(_ink_tune(form, r)))) for r in INK]
        for ragged in (False, True):
            ps = [(r, p) for r, p in plans if p['ragged'] == ragged]
            assert {r[1] for r, _ in ps} == {32, 64, 96} and {r[3] for r, _ in ps} == {32, 64, 96}, (form, ragged)
            assert len({p['nsplit'] for _, p in ps}) > 1
        ns = {p['nsplit'] for _, p in plans}
        assert {1, 2, 3, 5} <= ns and any(n % 4 == 0 for n in ns), ns
        assert any(p['ntiles'] % p['per'] for _, p in plans), 'a last split with fewer tiles'
        assert any(r[8] and p['nsplit'] < r[7] for r, p in plans), 'a reserve that lowers the split count'
        maps = {(r[2] == _id(r[1]), r[4] == _id(r[3]), r[2][2] < r[1], r[4][2] < r[3]) for r in INK}
        assert {(True, True, False, False), (False, True, False, False), (True, False, False, False)} <= maps
        assert any(m[2] for m in maps) and any(m[3] for m in maps), 'two-segment R and two-segment C'
        assert {r[5] for r in INK} == {1, 2} and {r[6] for r in INK} == {1, 2}
    for form in (24, 44):
        rows = [r for _, r in _pre_rows(form)]
        plans = [(r, _pre_plan(form, _geom(form, SH[form][r[0]])['Tp'], r[1], r[3], _td(r[6]))) for r in rows]
        split = [(r, p) for r, p in plans if p['kind'] == 'split']
        assert {p['phs'] for _, p in split} == {1, 2, 4}, (form, sorted({p['phs'] for _, p in split}))
        assert any(_geom(form, SH[form][r[0]])['Tp'] % p['per'] for r, p in split), 'a last split shorter than per'
        sk = [(r, p) for r, p in plans if p['kind'] == 'sk' and r[6].get('wgrad_streamk') == 2]
        counts = set().union(*[set(_item_slots(p)) for _, p in sk])
        assert 1 in counts and 2 in counts and any(c >= 3 for c in counts), counts
        assert any(p['S'] % p['Q'] for _, p in sk), 'a workgroup stops inside an item'
        assert any(r[6].get('cu_reserve') and p['Q'] != w24g_sk_plan(_geom(form, SH[form][r[0]])['Tp'], r[1], r[3], p['P'], NCU)['Q'] for r, p in sk), 'a reserve changes Q'
        assert {(r[1], r[3]) for r, p in plans if p['kind'] == 'skw'} >= {(128, 128), (128, 256), (256, 128), (384, 256)}
        dflt = {p['kind'] for r, p in plans if 'wgrad_streamk' not in r[6] and p['kind'] != 'skw'}
        assert dflt == {'split', 'sk'}, 'the default plan on both sides of its switch'
        maps = {(r[2] == _id(r[1]), r[4] == _id(r[3]), r[2][2] < r[1], r[4][2] < r[3]) for r in rows}
        assert {(True, True, False, False), (False, True, False, False), (True, False, False, False)} <= maps
        assert any(m[2] for m in maps) and any(m[3] for m in maps)
        assert {r[5] for r in rows} == {1, 2} and {r[7] for r in rows} == {False, True}
        assert {k for _, p in plans for k in [p['kind']]} == {'split', 'sk', 'skw'}
        assert max(_geom(form, s)['Tp'] for s in SH[form]) >= 256
    for form in (24, 44):
        assert {r[1] for r in XFORM} == {8, 40, 64} and {r[2] for r in XFORM} == {1, 2}
        assert {r[1] for r in XFORM if r[3]} == {8, 40, 64} and {r[1] for r in XFORM if r[3] and r[2] == 2} >= {40}
        wide = {(SH[form][si][2] >= 32, bool(SH[form][si][1] % _geom(form, SH[form][si])['PH'] or SH[form][si][2] % _geom(form, SH[form][si])['PW']))
                for si in {r[0] for r in XFORM}}
        assert wide == {(a, b) for a in (False, True) for b in (False, True)}, 'W < 32 and W >= 32, whole and ragged blocks'


def check_wino_exact_conditions():
    """The 2^24 conditions of every exact case and the identity G^T U G = direct sum of the reference's own matrices, from the references alone
    (no library call, no device): _expect and _xform_expect assert them."""
    for form in (24, 44):
        for i, row in enumerate(XFORM):
            _xform_expect(form, True, row[0], row[1], row[3], 3100 + i)
        for i, row in _pre_rows(form):
            shape = SH[form][row[0]]
            _expect(form, True, shape, row[1], row[2], row[3], row[4], 4100 + i, _geom(form, shape))
    for form in (22, 24):
        for i, row in enumerate(INK):
            _expect(form, True, row[0], row[1], row[2], row[3], row[4], 5100 + i, None)


def check_wino_layout_helpers():
    """The index helpers of the documented layouts round-trip, agree with the vectorised placement the tests use, and the tile order covers
    every output pixel of the image once (tiles of a ragged block outside the image cover none)."""
    for form in (24, 44):
        P = 24 if form == 24 else 36
        for shape in SH[form]:
            g = _geom(form, shape)
            B, H, W = shape
            seen = set()
            for t in range(g['Tp']):
                b, y0, x0 = _tile_origin(g, t)
                assert _tile_of(g, b, y0, x0) == t and _tile_of(g, b, y0 + g['th'] - 1, x0 + 3) == t
                seen |= {(b, y, x) for y in range(y0, min(y0 + g['th'], H)) for x in range(x0, min(x0 + 4, W))}
            assert len(seen) == B * H * W
            for Cp in (8, 40):
                n = g['Tp'] * P * Cp
                lay = _v_layout(torch.arange(n, dtype=torch.float64).view(g['Tp'], P, Cp))
                for off in list(range(0, n, max(1, n // 997))) + [n - 1]:
                    t, pl, c = _v_unindex(off, Cp, P)
                    assert _v_index(t, pl, c, Cp, P) == off and int(lay[off]) == (t * P + pl) * Cp + c
            assert _yt_index(g['Tp'] - 1, P - 1, 127, g['Tp'], 128) == P * g['Tp'] * 128 - 1
