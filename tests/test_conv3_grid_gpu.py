"""GPU: the direct 3x3 convolution kernels (csrc/igemm.hip MODE_CONV3, igemm_ws.hip, igemm_pws.hip) and the weight-gradient kernels
(csrc/wgrad.hip, wgrad_dma.hip), per element, over the grid their launchers can start.

Every case calls the C ABI directly.  Every output sits in a poisoned buffer (ActAt / Rows: guard bands in front and behind, the other half
of a concat neighbour, extra rows behind the statistics rows, the weight gradient and its split-K workspace between guard bands) that must
come back bit-identical outside the written region; every launch runs twice and must give the same bits.  References are float64 torch
evaluations of include/clamd.h's formulas on the same host-generated inputs -- nine shifted contractions over a zero-padded input for the
convolution, a sum over pixels for the weight gradient -- never F.conv2d, the oracle or another call into libclamd.so; the same
contraction on absolute values gives sum |a w| for the bounds.  The tests here need the device: inputs and references are device tensors.
What needs none -- the case lists against this file's copies of the launchers' rules (check_conv3x3_plans, check_wgrad_plans) and the 2^24
conditions of every exact case from the references alone (check_exact_conditions) -- is run by tests/test_host_cpu.py with DEV set to
the host, so it is verified where there is no GPU too.

Packed filters are written here from the documented layout [9][Cout_p][Cin_p] (tap t = 3 ky + kx reads the input pixel (y + ky - 1,
x + kx - 1); Cin innermost).  What clamd_pack stores, and the kernels read, is that array K-chunk-major, [Cin_p / kc][9][Cout_p][kc] with
kc = 32 (bf16) or 16 (fp32, bf16x3) channels = one 64-byte chunk, the [tap][n] slab of a chunk contiguous; bf16x3 splits the innermost kc = 16
into [16 x bf16 hi][16 x bf16 lo] (ops.split_encode).  test_pack_layouts reads the same order back.  One exact case per entry point also
packs through ops.PackTable.conv3x3 -- the forward packing and the tap-flipped, transposed data-gradient packing, with a one- and a
two-segment (concat) input -- and asserts the same bits (PACKED rows).

Exact-integer cases (activations in [-4, 4], weights and gradients in {-2 .. 2}, integer bias and bias table, about a quarter zeros): every
partial sum is an integer below 2^24, exact in fp32 in any order, so the output EQUALS storage(exact result) bit for bit; padded output
channels are +0 in all bits; every statistics row and five-sum row equals the int64 reference of ITS pixels taken on the fp32 value before
storage -- which pins the tile or workgroup a row belongs to (baseline and producer/consumer kernel: row = pixel tile; persistent kernel:
row mg = tiles mg, mg + gm, ...) -- the totals are added in int64; the row count equals clamd_stat_rows() and this file's copy of the
launch's rule; the weight gradient equals the integer sum under every split plan.  The 2^24 condition is asserted from the reference for
every output element and for every row's per-channel sum of absolute terms (a row is what one fp32 chain adds up).

Which value the kernels sum: every structure adds v = relu?(accumulator + bias), the fp32 value BEFORE the rounding to storage, into
sum / sum of squares, and g = the same fp32 value into the five sums (sum g, sum g y, sum g [y > 0], sum [y > 0], sum y), y = bn_y as
stored.  The baseline, the producer/consumer and the fp32 / bf16x3 persistent kernel start the MFMA chain at zero and add the bias (or the border-class entry) last;
the bf16 persistent kernel (channels-in-the-lane epilogue) starts the chain AT the bias, and with a border-class table at the interior
entry t4, adding fl(t_class - t4) to border pixels afterwards.

Random-valued cases (_normal: values the storage holds, bf16x3 with a live lo plane, |lo| <= 2^-9 |x|), bound per element, derived:
  convolution    n u (sum |a w| + |bias|), n = 9 Kp + 1 additions (fp32, bf16), 27 Kp + 1 (bf16x3: hi hi + hi lo + lo hi), u = UNIT[(kernel,
                 dtype)], EPS = 2^-24 unless a kernel whose exact cases pass exceeds it; + 2^-50 of the same sum for the float64 reference;
                 bf16x3: + 2^-18 sum |a w| for the dropped lo lo products.  bf16 persistent kernel with a table: |bias| = |t4| + |t_class -
                 t4| and n + 2 (the difference and its addition are two more roundings of at most u times that magnitude)
  weight grad    n u sum |a b|, n = B H W pixels summed (padding taps included), times 3 for bf16x3, plus the split-K slabs the reduce kernel
                 adds; + 2^-50 and (bf16x3) 2^-18 of the same sum; fp32 output: no storage term
  storage        + STORE_REL[dtype] (|ref| + the above)
  statistics     as test_bn_grid_gpu.py bounds its random sums: the per-element bounds of the fp32 values added up, + n EPS sum |terms|,
                 n the pixels per channel; for v^2 and g y the propagated 2 |v| e + e^2 and |y| e
Worst error / bound seen on the MI355X in one run of this file (exact cases: equality)
(34 tests in 11.0 s; UNIT is empty: no pair exceeds 1 with u = 2^-24.  bf16 outputs sit just under 1 because the half-ulp storage term is
sharp; the one-pixel weight gradients do because one product's rounding, or bf16x3's dropped lo lo, is all there is.)
                                                       fp32                    bf16                    bf16x3
  baseline            output / statistics / five sums  0.014 / 0.004 / 0.194   0.979 / 0.002 / 0.001   0.046 / 0.015 / 0.113
  producer/consumer   output / statistics / five sums  0.012 / 0.003 / 0.269   0.973 / 0.001 / 0.001   0.041 / 0.008 / 0.087
  persistent          output / statistics / two sums   0.019 / 0.002 / -       0.962 / 0.001 / 0.000   0.058 / 0.003 / -
  weight gradient     CONV3 / PW / UP2                 0.491 / 0.004 / 0.147   0.151 / 0.002 / 0.063   0.865 / 0.006 / 0.403

Paths.  Shapes: S16 = 2 x 17 x 18 (TW 16: ragged in both directions, W % 4 != 0; the last tile row is the image's bottom row), S32A =
1 x 9 x 36, S32B = 2 x 8 x 33 (TW 32, ragged), U16 = 1 x 16 x 16 and U32 = 1 x 8 x 32 (one whole tile: RAGGED = false), 1 x 1 x 1 and
1 x 1 x 5 (only the centre row of taps reads the image), 3 x 2 x 2 (no interior border class), 3 x 4 x 4 (smaller than a tile), WALK =
1 x 41 x 162 (36 ragged tiles) and WALKU = 2 x 40 x 128 (40 whole tiles).  x2 / y2: the operand is the second half of a buffer of twice
the pitch.  T = float | bf16_t | split_t, looped by every test.
  igemm_kernel<T, MODE_CONV3, EPI_NHWC, 16|32, 0|1|2>   BASE rows (igemm_pws 0, igemm_ws 0), igemm_variant per row (bf16x3 ignores it): every
                                      shape above but the walks; Kp 32 / 64 / 96 / 128, Np 32 (the n < Np guards) / 64 / 128 / 256, x2, y2,
                                      bias / none, ReLU on / off, statistics / five sums / none, m_fastest 0 / 1, grids of 1 .. 12 workgroups
  igemm_ws_kernel<T, 16, 1|2>, <T, 32, 1|2|4>           WS rows: igemm_ws 4 | 1 | 3 at W < 32 (3 clamps to 256-pixel tiles: <16, 2>) and W >= 32,
                                      the same operand variants, m_fastest 0 / 1, grids that are no multiple of 8 (xcd_remap)
  igemm_pws_kernel<float|split_t, 16|32, ragged|not, CLS 0|1, 0>   PWS rows (igemm_pws 2): CLS by the `tab` rows; pws_wres 0 / 1 at Kp 32 (two
                                      K-steps) and Kp 64 / 128; gm clamped to the tile count on the tiny images; WALK / WALKU with
                                      cu_reserve 128 and Np 256: 32 workgroups per slab walk 36 or 40 tiles, the last round ragged
                                      all 8: <16, ragged> S16 and the tiny images, <16, not> U16, <32, ragged> S32A / S32B / WALK, <32, not>
                                      U32 / WALKU, each with a `b` or plain row (CLS 0) and a `tab` row (CLS 1)
  igemm_pws_kernel<bf16_t, TW, RAGGED, CLS, CLM>        the PWS rows with Kp 64 / 128 (bf16 declines Kp 32 and 96), all 16, (shape Kp bias):
      <16, ragged, ., .>   CLM 1: S16 128 plain     CLM 2: S16 64 b, P1 / P44 64 b     CLS, 2: S16 64 / 128 tab, P22 64 tab     CLM 3: S16 64 bn, P5 64 bn
      <16, not, ., .>      CLM 1: U16 64 plain      CLM 2: U16 64 b                    CLS, 2: U16 64 tab                       CLM 3: U16 64 bn
      <32, ragged, ., .>   CLM 1: S32A 128 plain    CLM 2: S32A 64 b, S32B 128 b, WALK 64 b     CLS, 2: S32A 64 tab, WALK 64 tab     CLM 3: S32B 64 bn, WALK 64 bn
      <32, not, ., .>      CLM 1: U32 64, WALKU 128 plain     CLM 2: U32 128 b, WALKU 64 b     CLS, 2: U32 64 tab, WALKU 64 tab     CLM 3: U32 64 bn
                                      CLM 1 = no bias, ReLU or statistics; CLM 2 = bias or table, ReLU, statistics (the training step's
                                      kernel); CLM 3 = `bn` and nothing else: clamd_conv3x3_bn_sums() = 2, rows 0-1 per row, rows 2-4 NaN in every
                                      row.  pws_wres 0 / 1 at Kp 64 (two K-steps: the resident filter slab) and Kp 128.  check_conv3x3_plans
                                      computes the (TW, RAGGED, CLS, CLM) set of the rows per dtype with launch_pws_t's selection and asserts it
                                      complete (8 / 16 / 8), and test_conv3x3_persistent_exact asserts it again of the rows it ran
  declined by the persistent kernel   bf16 at Kp 32 and Kp 96 (Kp % 64): the PWS rows at those Kp run the structure igemm_ws names, the rows
                                      say so and clamd_conv3x3_border_bias_ok() answers 0.  fp32 / bf16x3 decline Kp % 32, which every entry
                                      point refuses before (Kp = 48: test_host_cpu.py), so that branch cannot be reached.  bn_y in fp32 /
                                      bf16x3, and in bf16 with bias, ReLU or statistics: five sums from the structure igemm_ws names
  refused                             test_border_table_refusals: the flag with the baseline or producer/consumer structure, with bias NULL,
                                      with H = 1: status -1, the message, the output untouched
  wgrad_kernel<T, CONV3|PW|UP2, 16|32, WS>   WGRAD rows: wgrad_ws 0 / 1 (CONV3 only has WS), wgrad_tw16 0 / 1 at W >= 32 (bf16x3 CONV3 is always
                                      16 wide), wgrad_xcd 0 / 1 with grids of 5, 6, 7 workgroups, identity / R-only / C-only / both padded /
                                      two-segment C / two-segment R maps, a and b as second halves
  wgrad_dma_kernel<16|32>             WGRAD rows with wgrad_dma 2 (bf16), and wgrad_dma 1 with rt ct = 2 (runs it) and 1 (does not)
  wgrad_reduce_kernel<1|4|16|64>      nsplit 1 and 2 (<1>), 3 .. 31 (<4>), 32 .. 63 and >= 64 with more than 8192 elements (<16>), >= 64 at PW /
                                      UP2 with 32-64 channels on 4 x 32 x 64 (<64>); a last slab with fewer tiles; cu_reserve halving the
                                      target.  check_wgrad_plans (test_host_cpu.py) asserts from this file's copy of the launcher's rule that the rows
                                      reach all of these for every dtype; each case pins nsplit itself: the workspace is exactly nsplit
                                      slabs long, and one byte less is refused
Left unreached: igemm_variant 3-6 (diagnostic builds only); the 2^31 grid and image limits; igemm_ws 2 (the heuristic takes Kp >= 256, past
the Kp <= 128 of the exact cases; it only chooses among the three tile heights run here); a second trip of wgrad_reduce_kernel's
grid-stride loop (more than 8192 workgroups: over 2 M gradient elements, i.e. 1024 x 256 channels of 3x3 filters).
bf16x3 with integer inputs has empty lo planes, and one missing lo hi term hides inside the random bound: test_*_bf16x3_live_lo_exact run
every row with x = i + j / 256 on one operand (hi + lo exact, lo lo = 0), where the output again EQUALS the exact result.
"""
import numpy as np
import pytest
import torch

from grid_util import (DEV, EPS, STORE_REL, Act, Rows, _dev, _expect_bits, _expect_rows, _half, _ints, _normal, _operand, _per_element, _raw,
                       _twice, _wgrad_ref)

pytestmark = pytest.mark.gpu

DT = [('fp32', 0), ('bf16', 1), ('bf16x3', 2)]
UNIT = {}                                      # (kernel, dtype code) -> u of the accumulation bound where EPS is exceeded (see above)
NCU = 256                                      # compute units of the MI355X (asserted against the device by the fixture)
S16, S32A, S32B, U16, U32 = (2, 17, 18), (1, 9, 36), (2, 8, 33), (1, 16, 16), (1, 8, 32)
P1, P5, P22, P44, WALK, WALKU = (1, 1, 1), (1, 1, 5), (3, 2, 2), (3, 4, 4), (1, 41, 162), (2, 40, 128)
KIND = ('baseline', 'producer/consumer', 'persistent')


@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    C._lib.load()
    assert torch.cuda.get_device_properties(0).multi_processor_count == NCU
    return C


def _sync():
    torch.cuda.synchronize()


def _live_lo(rng, v):
    """Integers -> integers + j / 256, j in {-3 .. 3}: hi = rne_bf16(x) and lo = x - hi hold x exactly, with a live lo plane."""
    return v + _ints(rng, tuple(v.shape), 3, 0.3) / 256.0


def _weights(rng, shape, dcode, exact):
    """Weights and gradients.  exact: True = integers in {-2 .. 2}; 'lo_w' (bf16x3) = those plus a live lo plane; False = _normal."""
    if not exact:
        return _normal(rng, shape, dcode, zeros=0.1)
    v = _ints(rng, shape, 2, 0.07)
    return _live_lo(rng, v) if exact == 'lo_w' else v


def _acts(rng, shape, dcode, exact):
    """Activations.  exact: True = integers in [-4, 4]; 'lo_a' (bf16x3) = those plus a live lo plane; False = _normal."""
    if not exact:
        return _normal(rng, shape, dcode)
    v = _ints(rng, shape, 4, 0.15)
    return _live_lo(rng, v) if exact == 'lo_a' else v


def _grain(exact):
    """What every exact partial sum is a multiple of: 1, or 2^-8 with a live lo plane on one operand (the limit is then 2^24 grains)."""
    return 256.0 if isinstance(exact, str) else 1.0


def _pmap(segs):
    """[(logical, physical), ...] -> physical channel -> logical channel | -1 (each segment padded on its own)."""
    out, base = [], 0
    for lg, ph in segs:
        out += [base + i if i < lg else -1 for i in range(ph)]
        base += lg
    return out


def _live(pm):
    return torch.tensor([p for p, l in enumerate(pm) if l >= 0], dtype=torch.long, device=DEV)


# ----------------------------------------------------------------------------------------------------- the launchers' rules, in Python
def _tiling(B, H, W, TW, TH):
    """Pixel -> pixel-tile index (tiles run x fastest, then y, then the image) and the tile count."""
    tx, ty = -(-W // TW), -(-H // TH)
    b, y, x = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), indexing='ij')
    return ((b * ty + y // TH) * tx + x // TW).reshape(-1).to(DEV), B * tx * ty


def _plan(shape, Kp, Np, dcode, td, bn, plain):
    """plan_conv3x3 / pws_rows / ws_rows for the tuning dict `td` -> (kind, partial rows, pixel -> row)."""
    B, H, W = shape
    TW = 32 if W >= 32 else 16
    kc = 32 if dcode == 1 else 16
    if (td['igemm_pws'] == 2 or (td['igemm_pws'] == 1 and Kp <= 256)) and Kp % (2 * kc) == 0 and not (bn and (dcode != 1 or not plain)):
        ids, ntm = _tiling(B, H, W, TW, 256 // TW)
        gm = min(max(1, max(8, NCU - max(td['cu_reserve'], 0)) // (-(-Np // 64))), ntm)
        return 2, gm, ids % gm
    mt = {1: 2, 3: 4, 4: 1}.get(td['igemm_ws'], 0)
    assert mt or td['igemm_ws'] == 0 or Kp < 256
    if mt:
        mt = min(mt, 2) if TW == 16 else mt
        return (1,) + _tiling(B, H, W, TW, 128 * mt // TW)[::-1]
    return (0,) + _tiling(B, H, W, TW, 256 // TW)[::-1]


def _pws_inst(dcode, row):
    """launch_pws_t's selection for a case row: the igemm_pws_kernel<T, TW, RAGGED, CLS, CLM> it starts as (TW, ragged, CLS, CLM), or None
    where the persistent kernel declines the shape (another structure runs; a table is then refused and nothing runs)."""
    shape, Kp, _, Np, _, bias, relu, mode, tune = row[:9]
    plain = not bias and not relu and mode != 'stats'
    if _plan(shape, Kp, Np, dcode, _td(tune), mode == 'bn', plain)[0] != 2:
        return None
    TW = 32 if shape[2] >= 32 else 16
    ragged = bool(shape[1] % (256 // TW) or shape[2] % TW)
    return TW, ragged, bias == 'tab', 0 if dcode != 1 else 3 if mode == 'bn' else 1 if plain else 2


def _pws_all(dcode):
    """Every instantiation launch_pws_t can start for a dtype: 8 (fp32, bf16x3: the table or not) or 16 (bf16: CLM 1, 2, 2 with the table, 3)."""
    epi = [(False, 1), (False, 2), (True, 2), (False, 3)] if dcode == 1 else [(False, 0), (True, 0)]
    return {(tw, rg, cls, clm) for tw in (16, 32) for rg in (False, True) for cls, clm in epi}


def _wgrad_plan(mode, shape, Rp, Cp, dcode, td):
    """clamd_wgrad's split plan -> dict(TW, ntiles, nsplit, per, grid, reduce, dma, NT)."""
    B, H, W = shape
    NT = (9, 1, 4)[mode]
    TW = 32 if (W >= 32 and not (dcode == 2 and mode == 0) and not td['wgrad_tw16']) else 16
    TH = (128 if dcode == 1 else 64) // (2 if mode == 2 else 1) // TW
    ntiles = -(-W // TW) * -(-H // TH) * B
    rt, ct = -(-Rp // 64), -(-Cp // 64)
    ws = bool(td['wgrad_ws']) and mode == 0
    target = td['wgrad_blocks'] * max(8, NCU - max(td['cu_reserve'], 0)) // NCU
    nsplit = min(max(1, (target // 2 if ws else target) // (rt * ct)), ntiles)
    per = -(-ntiles // nsplit)
    nsplit = -(-ntiles // per)
    reduce = 1 if nsplit <= 2 else 64 if (NT * Rp * Cp <= 8192 and nsplit >= 64) else 16 if nsplit >= 32 else 4
    dma = dcode == 1 and ws and (td['wgrad_dma'] == 2 or (td['wgrad_dma'] == 1 and rt * ct > 1))
    return dict(TW=TW, ntiles=ntiles, nsplit=nsplit, per=per, grid=rt * ct * nsplit, reduce=reduce, dma=dma, NT=NT, ws=ws)


TUNE0 = dict(igemm_pws=1, igemm_ws=2, igemm_variant=0, pws_wres=1, wgrad_ws=1, wgrad_dma=1, wgrad_xcd=1, wgrad_blocks=512, wgrad_tw16=0, cu_reserve=0)


def _td(tune):
    """The tuning fields the rules above read: the library's defaults (asserted by _tuning) overridden by the case."""
    return dict(TUNE0, **tune)


def _tuning(C, tune):
    tn = C._lib.Tuning(**tune)
    assert {k: v for k, v in tn.as_dict().items() if k in TUNE0} == _td(tune)
    return tn


# --------------------------------------------------------------------------------------------------------------------------- references
def _conv3_ref(x, wp, shape):
    """x [npix, Kp], wp [9][Np][Kp] (fp32 values) -> the float64 convolution [npix, Np] and the sum of the absolute terms: nine shifted
    contractions over the zero-padded input, tap t = 3 ky + kx reading pixel (y + ky - 1, x + kx - 1)."""
    B, H, W = shape
    Kp = x.shape[1]
    pad = torch.zeros(B, H + 2, W + 2, Kp, dtype=torch.float64, device=x.device)
    pad[:, 1:H + 1, 1:W + 1] = x.double().view(B, H, W, Kp)
    ref = torch.zeros(B * H * W, wp.shape[1], dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(ref)
    for t in range(9):
        ky, kx = divmod(t, 3)
        a, w = pad[:, ky:ky + H, kx:kx + W].reshape(B * H * W, Kp), wp[t].double()
        ref += a @ w.T
        mag += a.abs() @ w.abs().T
    return ref, mag


def _border_class(shape):
    """Pixel -> 3 (0 top row | 1 interior | 2 bottom row) + (0 left column | 1 interior | 2 right column); H, W >= 2."""
    B, H, W = shape
    _, y, x = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), indexing='ij')
    cls = 3 * torch.where(y == 0, 0, torch.where(y == H - 1, 2, 1)) + torch.where(x == 0, 0, torch.where(x == W - 1, 2, 1))
    return cls.reshape(-1).to(DEV)


def _acc_bound(key, dcode, n, mag, prod):
    """The bound of the fp32 accumulator value against the float64 reference (module docstring): n additions, the reference's own roundings,
    the dropped lo lo products of bf16x3."""
    return n * UNIT.get((key, dcode), EPS) * mag + 2.0 ** -50 * mag + (2.0 ** -18 * prod if dcode == 2 else 0.0)


def _per_row(ids, n, v):
    return torch.zeros(n, v.shape[1], dtype=v.dtype, device=DEV).index_add_(0, ids, v)


def _check_sums(what, key, dcode, exact, got, ids, n, terms, errs):
    """got [n][nk][Np] against the float64 per-pixel `terms` [nk][npix, Np].  exact: every row EQUALS the int64 sum of its pixels (`ids`: pixel ->
    row), the totals agree in int64; else the totals lie within sum(errs) + npix EPS sum |terms|."""
    npix = terms[0].shape[0]
    if exact:
        for t in terms:
            assert float(_per_row(ids, n, t.abs()).max()) < 2 ** 24, what + ': a row\'s per-channel sum of absolute terms reaches 2^24'
        exp = torch.stack([_per_row(ids, n, t.to(torch.int64)) for t in terms], 1)
        bad = _raw(got.contiguous()) != _raw(exp.float().contiguous())
        if bool(bad.any()):
            i = tuple(bad.nonzero()[0].tolist())
            raise AssertionError(f'{what}: {int(bad.sum())} (row, sum, channel) entries differ from the int64 reference of the row\'s pixels; first at {i}: '
                                 f'got {float(got[i])!r}, expected {int(exp[i])}')
        assert torch.equal(got.double().sum(0).to(torch.int64), exp.sum(0)), what + ': the totals differ from the int64 reference'
        return
    assert bool(torch.isfinite(got).all()), what + ': a row that is not finite'
    ref = torch.stack([t.sum(0) for t in terms])
    bound = torch.stack([e.sum(0) + (npix + 1) * EPS * (t.abs() + e).sum(0) for t, e in zip(terms, errs)])
    _per_element(what + ' rows', (key + ' rows', dcode), got.double().sum(0), ref, bound)


# ------------------------------------------------------------------------------------------------------------------------ clamd_conv3x3
B0, P0, W0 = dict(igemm_pws=0, igemm_ws=0), dict(igemm_pws=2, igemm_ws=0), dict(igemm_pws=0)


def _t(base, **kw):
    return dict(base, **kw)


#        shape Kp  x  Np   y  bias  relu mode     tuning                      m_fastest
BASE = [(S16, 32, 1, 32, 1, 'b', 1, 'stats', _t(B0, igemm_variant=0), 0),
        (S32A, 64, 2, 64, 2, '', 0, 'bn', _t(B0, igemm_variant=1), 1),
        (S32B, 96, 1, 128, 1, 'b', 0, 'stats', _t(B0, igemm_variant=2), 0),
        (U16, 128, 2, 256, 2, 'b', 1, '', _t(B0, igemm_variant=1), 1),
        (U32, 32, 1, 32, 1, '', 1, 'stats', _t(B0, igemm_variant=2), 1),
        (S16, 64, 1, 32, 2, '', 0, 'bn', _t(B0, igemm_variant=2), 0),
        (S32A, 128, 1, 64, 1, 'b', 1, 'bn', _t(B0, igemm_variant=0), 0),
        (P1, 32, 1, 32, 1, 'b', 0, 'stats', _t(B0, igemm_variant=0), 0),
        (P5, 64, 1, 64, 1, '', 0, 'bn', _t(B0, igemm_variant=1), 0),
        (P22, 32, 1, 128, 1, 'b', 1, 'stats', _t(B0, igemm_variant=1), 1),
        (P44, 96, 2, 32, 1, 'b', 0, 'stats', _t(B0, igemm_variant=2), 0)]
WS = [(S16, 32, 1, 32, 1, 'b', 1, 'stats', _t(W0, igemm_ws=4), 0),
      (S16, 64, 2, 64, 2, '', 0, 'bn', _t(W0, igemm_ws=1), 1),
      (S16, 96, 1, 128, 1, 'b', 0, 'stats', _t(W0, igemm_ws=3), 0),
      (S32A, 64, 2, 64, 2, 'b', 1, 'stats', _t(W0, igemm_ws=4), 1),
      (S32B, 128, 1, 256, 1, '', 0, 'bn', _t(W0, igemm_ws=1), 1),
      (S32A, 32, 1, 32, 1, 'b', 1, 'stats', _t(W0, igemm_ws=3), 0),
      (S32B, 64, 1, 32, 2, '', 0, 'bn', _t(W0, igemm_ws=3), 0),
      (U16, 64, 1, 64, 1, 'b', 1, 'stats', _t(W0, igemm_ws=1), 0),
      (U32, 128, 1, 128, 2, 'b', 0, '', _t(W0, igemm_ws=3), 1),
      (P1, 32, 1, 32, 1, 'b', 1, 'stats', _t(W0, igemm_ws=4), 0),
      (P5, 64, 1, 64, 1, '', 0, 'bn', _t(W0, igemm_ws=1), 0),
      (P22, 96, 1, 64, 1, 'b', 0, 'stats', _t(W0, igemm_ws=4), 1),
      (P44, 32, 2, 32, 1, '', 1, 'stats', _t(W0, igemm_ws=3), 0)]
PWS = [(S16, 32, 1, 32, 1, 'b', 1, 'stats', _t(P0, pws_wres=1), 0),                  # bf16 declines Kp 32 -> baseline
       (S16, 32, 1, 64, 1, 'tab', 1, 'stats', _t(P0, pws_wres=0), 0),                # (fp32 / bf16x3: two K-steps, both pws_wres)
       (S16, 64, 2, 64, 2, 'b', 1, 'stats', _t(P0, pws_wres=1), 0),                  # bf16: two K-steps
       (S16, 64, 1, 128, 1, 'tab', 1, 'stats', _t(P0, pws_wres=0), 1),
       (S16, 128, 1, 32, 2, 'tab', 0, '', _t(P0, pws_wres=1), 0),
       (S16, 128, 1, 64, 1, '', 0, '', _t(P0, pws_wres=0), 0),                       # bf16: CLM 1 at TW 16, ragged
       (S32A, 128, 2, 128, 2, '', 0, '', _t(P0, pws_wres=1), 0),                     # bf16: CLM 1
       (S32A, 64, 1, 64, 1, 'tab', 1, 'stats', _t(P0, pws_wres=1), 0),
       (S32B, 64, 1, 128, 1, '', 0, 'bn', _t(P0, pws_wres=1), 0),                    # bf16: CLM 3; fp32 / bf16x3 decline -> baseline
       (S16, 64, 1, 32, 2, '', 0, 'bn', _t(P0, pws_wres=0), 0),                      # Np 32 with five-sum rows
       (S32B, 96, 1, 64, 1, 'b', 0, 'stats', _t(P0, igemm_ws=1, pws_wres=1), 0),     # bf16 declines Kp 96 -> producer/consumer
       (S32B, 128, 1, 64, 2, 'b', 1, 'stats', _t(P0, pws_wres=0), 0),                # bf16: CLM 2 without a table at TW 32, ragged
       (S32A, 64, 1, 128, 1, 'b', 0, 'stats', _t(P0, pws_wres=1), 0),                # the same at two K-steps
       (S16, 64, 1, 64, 1, 'b', 0, 'bn', _t(P0, pws_wres=1), 0),                     # bn_y with a bias: every dtype declines -> baseline
       (S32A, 64, 1, 64, 1, '', 1, 'bn', _t(P0, igemm_ws=4, pws_wres=1), 0),         # bn_y with ReLU -> producer/consumer
       (U16, 64, 1, 32, 1, 'b', 0, 'stats', _t(P0, pws_wres=1), 0),
       (U16, 32, 1, 64, 1, 'tab', 1, 'stats', _t(P0, pws_wres=1), 0),
       (U16, 64, 1, 64, 1, 'tab', 1, 'stats', _t(P0, pws_wres=0), 0),                # bf16: CLM 2 with the table, one whole TW-16 tile
       (U16, 64, 2, 32, 1, '', 0, '', _t(P0, pws_wres=1), 0),                        # bf16: CLM 1, one whole TW-16 tile
       (U16, 64, 1, 64, 1, '', 0, 'bn', _t(P0, pws_wres=1), 0),
       (U32, 128, 1, 64, 2, 'b', 1, 'stats', _t(P0, pws_wres=0), 0),
       (U32, 64, 2, 64, 1, 'tab', 1, 'stats', _t(P0, pws_wres=1), 0),
       (U32, 64, 1, 64, 1, '', 0, '', _t(P0, pws_wres=1), 0),
       (U32, 64, 1, 64, 1, '', 0, 'bn', _t(P0, pws_wres=0), 0),
       (P1, 64, 1, 64, 1, 'b', 1, 'stats', _t(P0, pws_wres=1), 0),                   # gm clamped to 1 tile
       (P5, 64, 1, 32, 1, '', 0, 'bn', _t(P0, pws_wres=1), 0),
       (P22, 64, 1, 64, 1, 'tab', 1, 'stats', _t(P0, pws_wres=1), 0),                # gm clamped to 3 tiles, no interior class
       (P22, 32, 1, 32, 1, 'tab', 0, 'stats', _t(P0, pws_wres=1), 0),
       (P44, 64, 1, 128, 1, 'b', 1, 'stats', _t(P0, pws_wres=0), 0),
       (WALK, 64, 1, 256, 1, 'tab', 1, 'stats', _t(P0, pws_wres=1, cu_reserve=128), 0),   # 32 workgroups per slab walk 36 tiles
       (WALK, 32, 1, 256, 1, 'b', 1, 'stats', _t(P0, pws_wres=1, cu_reserve=128), 0),
       (WALK, 64, 1, 256, 1, 'b', 1, 'stats', _t(P0, pws_wres=0, cu_reserve=128), 0),     # bf16: the training step's kernel on a ragged walk
       (WALK, 32, 1, 256, 1, 'tab', 0, 'stats', _t(P0, pws_wres=0, cu_reserve=128), 0),
       (WALK, 64, 1, 256, 1, '', 0, 'bn', _t(P0, pws_wres=1, cu_reserve=128), 0),
       (WALKU, 64, 1, 256, 1, 'b', 1, 'stats', _t(P0, pws_wres=1, cu_reserve=128), 0),    # 32 workgroups per slab walk 40 tiles
       (WALKU, 64, 2, 256, 2, 'tab', 1, 'stats', _t(P0, pws_wres=0, cu_reserve=128), 0),
       (WALKU, 128, 1, 256, 1, '', 0, '', _t(P0, pws_wres=1, cu_reserve=128), 0)]
# PackTable rows: Np and (data gradient) Kp are powers of two, as ops.cpad pads them.  pack: f1 / f2 = forward packing with a one- / two-segment
# input, d1 / d2 = the flipped, transposed data-gradient packing whose OUTPUT channels (the convolution's input) are one / two segments
PACKED = [(S16, 64, 1, 32, 1, 'b', 1, 'stats', _t(B0), 0, 'f1'),
          (S32A, 64, 1, 64, 1, 'b', 1, 'stats', _t(W0, igemm_ws=1), 0, 'f2'),
          (S16, 64, 1, 64, 1, 'tab', 1, 'stats', _t(P0), 0, 'f2'),
          (S32A, 64, 1, 32, 1, '', 0, 'bn', _t(B0), 0, 'd1'),
          (S16, 32, 1, 64, 1, '', 0, 'bn', _t(W0, igemm_ws=4), 0, 'd2'),
          (S32B, 64, 1, 64, 1, '', 0, 'bn', _t(P0), 0, 'd2')]


def _segments(P, pack, side):
    """The channel segments of the K side (forward packings) or the N side (data-gradient packings): one segment padded at its end, or two
    halves each padded on its own (a concat input)."""
    if pack and pack[1] == '2' and side == ('k' if pack[0] == 'f' else 'n'):
        return [(P // 2 - 3, P // 2), (P // 2 - 2, P // 2)]
    return [(P - (3 if side == 'k' else 5), P)]


def _conv3_inputs(rng, dcode, exact, shape, Kp, Np, bias, pack=None):
    """x [npix, Kp]; the logical filters wl [Nl][Kl][3][3] and their documented packing wp [9][Np][Kp]; the bias table [9][Np] (one row
    repeated unless bias == 'tab'); bn_y [npix, Np]; the padded output channels."""
    npix = shape[0] * shape[1] * shape[2]
    kmap, nmap = _pmap(_segments(Kp, pack, 'k')), _pmap(_segments(Np, pack, 'n'))
    klive, nlive = _live(kmap), _live(nmap)
    Kl, Nl = klive.numel(), nlive.numel()
    x = torch.zeros(npix, Kp, device=DEV)
    x[:, klive] = _acts(rng, (npix, Kl), dcode, exact)
    wl = _weights(rng, (Nl, Kl, 3, 3), dcode, exact)
    rows = torch.zeros(9, Np, Kl, device=DEV)
    rows[:, nlive] = wl.permute(2, 3, 0, 1).reshape(9, Nl, Kl)
    wp = torch.zeros(9, Np, Kp, device=DEV)
    wp[:, :, klive] = rows
    nb = 9 if bias == 'tab' else 1
    tab = torch.zeros(nb, Np, device=DEV)
    tab[:, nlive] = _ints(rng, (nb, Nl), 3, 0.0) if exact else _normal(rng, (nb, Nl), 0, zeros=0.0)
    tab = tab.expand(9, Np).contiguous()
    y = _ints(rng, (npix, Np), 4, 0.15) if exact else _normal(rng, (npix, Np), dcode)
    npad = torch.ones(Np, dtype=torch.bool, device=DEV)
    npad[nlive] = False
    return x, wl, wp, tab, y, npad


def _stored(C, wp, dcode):
    """[9][Np][Kp] -> the device operand: K-chunk-major [Kp / kc][9][Np][kc] in the compute dtype (module docstring)."""
    kc = C.ops.PackTable.KC[dcode]
    _, Np, Kp = wp.shape
    return _operand(C, wp.view(9, Np, Kp // kc, kc).permute(2, 0, 1, 3).contiguous(), dcode)


def _pack_check(C, what, dcode, pack, wl, wdev, Kp, Np):
    """ops.PackTable.conv3x3 on the same logical filters gives the bits of the hand-written operand."""
    T = C.ops.TORCH_DT[dcode]
    dst = torch.full((wdev.numel(),), 7.5, dtype=T, device=DEV)
    tab = C.ops.PackTable(dcode)
    if pack[0] == 'f':                                      # the parameter [Cout][Cin][3][3] is the kernel's [N][K][3][3]
        assert C.ops.cpad(wl.shape[0]) == Np
        tab.conv3x3(wl.contiguous(), dst, None, _segments(Kp, pack, 'k'), wl.shape[0])
    else:                                                   # the kernel's N is the parameter's Cin, its K the parameter's Cout; taps flipped
        assert C.ops.cpad(wl.shape[1]) == Kp
        tab.conv3x3(wl.flip(2, 3).permute(1, 0, 2, 3).contiguous(), None, dst, _segments(Np, pack, 'n'), wl.shape[1])
    tab.finalize(DEV).run(dcode)
    _sync()
    assert torch.equal(_raw(dst), _raw(wdev.reshape(-1))), f'{what}: clamd_pack and the documented layout differ ({pack})'


def _conv3_expect(dcode, exact, shape, Kp, Np, bias, relu, mode, td, x, wp, tab, y):
    """Everything the launch is compared with, from the inputs alone (no library call): the plan, the float64 result, the per-element bound
    of the fp32 value before storage, the per-pixel terms of the sums."""
    plain = not bias and not relu and mode != 'stats'
    kind, nrows, ids = _plan(shape, Kp, Np, dcode, td, mode == 'bn', plain)
    ref, prod = _conv3_ref(x, wp, shape)
    mag, n = prod.clone(), (27 if dcode == 2 else 9) * Kp + 1
    if bias:
        b = tab[_border_class(shape)].double() if bias == 'tab' else tab[0].double().expand_as(ref)
        ref = ref + b
        if bias == 'tab' and dcode == 1 and kind == 2:
            # The one bound here that is not n u (sum |a w| + |bias|) as it stands.  The bf16 persistent kernel starts the MFMA chain at the
            # interior entry t4 and adds cls_tab = fl(t_class - t4) to a border pixel after the chain, so the bias enters as two terms of
            # magnitudes |t4| and |t_class - t4| (their sum can exceed |t_class|), and there are two more roundings than in a chain started
            # at t_class: the subtraction that fills cls_tab and the addition after the chain, each at most u times a partial sum of those
            # magnitudes.  For interior pixels (t_class = t4) the second term is zero and only n + 2 for n remains (2 in 9 Kp + 1 >= 577)
            mag, n = mag + tab[4].double().abs() + (b - tab[4].double()).abs(), n + 2
        else:
            mag = mag + b.abs()
    if relu:
        ref = ref.clamp_min(0.0)
    key = 'conv3x3 ' + KIND[kind]
    if exact:
        assert float(mag.max()) * _grain(exact) < 2 ** 24
        e = torch.zeros_like(ref)
    else:
        e = _acc_bound(key, dcode, n, mag, prod)
    if mode == 'stats':
        terms, errs = [ref, ref * ref], [e, 2 * ref.abs() * e + e * e]
    elif mode == 'bn':
        yd, pos, z = y.double(), (y > 0).double(), torch.zeros_like(ref)
        terms, errs = [ref, ref * yd, ref * pos, pos.clone(), yd.clone()], [e, e * yd.abs(), e * pos, z, z]
        if dcode == 1 and kind == 2:
            terms, errs = terms[:2], errs[:2]
    else:
        terms, errs = [], []
    if exact:
        for t in terms:
            assert float(_per_row(ids, nrows, t.abs()).max()) < 2 ** 24
    return dict(kind=kind, nrows=nrows, ids=ids, ref=ref, e=e, terms=terms, errs=errs, key=key)


def _conv3_case(C, what, dcode, exact, shape, Kp, xm, Np, ym, bias, relu, mode, tune, mf, pack=None, seed=0):
    L, s = C._lib, C._lib.stream_ptr()
    (B, H, W), rng, td = shape, np.random.default_rng(seed), _td(tune)
    npix = B * H * W
    x, wl, wp, tab, y, npad = _conv3_inputs(rng, dcode, exact, shape, Kp, Np, bias, pack)
    ex = _conv3_expect(dcode, exact, shape, Kp, Np, bias, relu, mode, td, x, wp, tab, y)
    kind, nrows, ids, ref, e = ex['kind'], ex['nrows'], ex['ids'], ex['ref'], ex['e']
    what = f'{what} [{KIND[kind]}]'
    tn = _tuning(C, tune)
    # the queries follow the same rules: rows of the PLAIN launch with these sizes, the table where a forward launch is persistent, two sums
    # where a plain bf16 data-gradient launch is
    assert L.stat_rows(L.OP_CONV3X3, B, H, W, Kp, Np, dcode, mode == 'bn', tn) == _plan(shape, Kp, Np, dcode, td, mode == 'bn', True)[1]
    fwd_kind = _plan(shape, Kp, Np, dcode, td, False, False)[0]
    assert L.load().clamd_conv3x3_border_bias_ok(B, H, W, Kp, Np, dcode, tn.ref()) == int(fwd_kind == 2 and H >= 2 and W >= 2), what
    two = dcode == 1 and _plan(shape, Kp, Np, dcode, td, True, True)[0] == 2
    assert L.load().clamd_conv3x3_bn_sums(B, H, W, Kp, Np, dcode, tn.ref()) == (2 if two else 5), what
    xa, wdev = _half(C, npix, Kp, xm, dcode, x), _stored(C, wp, dcode)
    if pack:
        _pack_check(C, what, dcode, pack, wl, wdev, Kp, Np)
    ya = Act(C, npix, Np, Np, dcode, y) if mode == 'bn' else None
    bdev = (tab if bias == 'tab' else tab[0].contiguous()) if bias else None
    w_before = wdev.clone()
    if bias == 'tab' and kind != 2:                         # the persistent kernel declined the shape: the table is refused, nothing is written
        out, st = _half(C, npix, Np, ym, dcode), Rows(nrows, 2, Np)
        rc = L.load().clamd_conv3x3(xa.ptr, xa.ldc, L.ptr(wdev), L.ptr(bdev), out.ptr, out.ldc, st.ptr if mode else None, None, None,
                                    nrows if mode else 0, B, H, W, Kp, Np, relu | 2, mf, dcode, tn.ref(), s)
        _sync()
        assert rc == -1 and 'border-class bias table' in L.load().clamd_last_error().decode(), (what, rc)
        assert torch.equal(_raw(out.buf), _raw(out.before)) and torch.equal(_raw(st.buf), _raw(st.before)), what + ': a refused launch wrote'
        return kind

    def launch():
        out = _half(C, npix, Np, ym, dcode)
        st, bn = Rows(nrows, 2, Np) if mode == 'stats' else None, Rows(nrows, 5, Np) if mode == 'bn' else None
        L.call('clamd_conv3x3', xa.ptr, xa.ldc, L.ptr(wdev), L.ptr(bdev), out.ptr, out.ldc, st.ptr if st else None, ya.ptr if ya else None,
               bn.ptr if bn else None, nrows if mode else 0, B, H, W, Kp, Np, relu | (2 if bias == 'tab' else 0), mf, dcode, tn.ref(), s)
        _sync()
        return [out] + [r for r in (st, bn) if r]

    outs = _twice(what, launch)
    assert xa.guards_intact() and torch.equal(_raw(xa.buf), _raw(xa.before)), what + ': the input was written'
    assert torch.equal(_raw(wdev), _raw(w_before)), what + ': the operand was written'
    out = outs[0]
    if exact:
        _expect_bits(what + ' output', out, ref.float())
    else:
        _per_element(what + ' output', (ex['key'], dcode), out.get(), ref, e + STORE_REL[dcode] * (ref.abs() + e))
    assert bool(out.zero_bits()[:, npad].all()), what + ': padded channels are not +0'
    if mode:
        nk = len(ex['terms'])
        got = outs[1].view
        _check_sums(what, ex['key'] + (' five sums' if mode == 'bn' else ''), dcode, exact, got[:, :nk], ids, nrows, ex['terms'], ex['errs'])
        if nk == 2 and mode == 'bn':
            assert bool(torch.isnan(got[:, 2:]).all()), what + ': rows 2-4 of the two-sum form are not NaN in every row'
    return kind


def _run(C, name, dcode, exact, rows, seed0):
    kinds = set()
    for i, row in enumerate(rows):
        kinds.add(_conv3_case(C, f'conv3x3 {name} {"exact" if exact else "random"} {row}', dcode, exact, *row, seed=seed0 + i))
    return kinds


@pytest.mark.parametrize('name,dcode', DT)
def test_conv3x3_baseline_exact(C, name, dcode):
    assert _run(C, name, dcode, True, BASE, 1000) == {0}


@pytest.mark.parametrize('name,dcode', DT)
def test_conv3x3_baseline_random(C, name, dcode):
    _run(C, name, dcode, False, BASE, 1100)


@pytest.mark.parametrize('name,dcode', DT)
def test_conv3x3_producer_consumer_exact(C, name, dcode):
    assert _run(C, name, dcode, True, WS, 1200) == {1}


@pytest.mark.parametrize('name,dcode', DT)
def test_conv3x3_producer_consumer_random(C, name, dcode):
    _run(C, name, dcode, False, WS, 1300)


@pytest.mark.parametrize('name,dcode', DT)
def test_conv3x3_persistent_exact(C, name, dcode):
    assert _run(C, name, dcode, True, PWS, 1400) == {0, 1, 2}          # the declined shapes fall through to both other structures
    assert {_pws_inst(dcode, row) for row in PWS} - {None} == _pws_all(dcode)          # what ran is every instantiation of the dtype


@pytest.mark.parametrize('name,dcode', DT)
def test_conv3x3_persistent_random(C, name, dcode):
    _run(C, name, dcode, False, PWS, 1500)


@pytest.mark.parametrize('name,dcode', DT)
def test_conv3x3_packed_by_pack_table(C, name, dcode):
    _run(C, name, dcode, True, PACKED, 1600)


@pytest.mark.parametrize('flavour', ['lo_a', 'lo_w'])
def test_conv3x3_bf16x3_live_lo_exact(C, flavour):
    """bf16x3 with a live lo plane on ONE operand and integers on the other (x = i + j / 256: hi + lo holds it exactly): lo lo is zero, so
    hi hi + lo hi + hi lo is the exact product and every partial sum a multiple of 2^-8 below 2^16 -- the output EQUALS storage(exact result).
    Integer inputs leave both lo planes empty and cannot see a missing lo hi or hi lo term; the random bound (27 Kp u sum |a w|) is wider
    than one such term.  Every row of the three lists, outputs only (sums of squares of such values are not exact in fp32)."""
    for lst, seed0 in ((BASE, 1800), (WS, 1830), (PWS, 1860)):
        for i, row in enumerate(lst):
            row = row[:7] + ('',) + row[8:]
            _conv3_case(C, f'conv3x3 bf16x3 exact, live lo ({flavour}) {row}', 2, flavour, *row, seed=seed0 + i)


def check_conv3x3_plans():
    """The case lists reach what the docstring's path table says, from this file's copy of the planner and of the launchers' selection (no
    launch, no device: test_host_cpu.py runs it): every instantiation launch_pws_t can start for the dtype, every tile width and variant of
    the baseline kernel, every <TW, MT> of the producer/consumer kernel, the persistent kernel's declined shapes per dtype, a persistent walk
    with a ragged last round, gm clamped to the tile count, both pws_wres at two K-steps and at a longer K."""
    for _, dcode in DT:
        inst = {}
        for row in PWS + PACKED:
            inst.setdefault(_pws_inst(dcode, row), []).append(row)
        inst.pop(None)
        assert set(inst) == _pws_all(dcode), (dcode, sorted(_pws_all(dcode) - set(inst)))
        two = 64 if dcode == 1 else 32                        # two K-steps: 2 kc channels
        ran = [r for rows in inst.values() for r in rows]
        assert {(r[1] == two, r[8]['pws_wres']) for r in ran if 'pws_wres' in r[8]} == {(a, b) for a in (False, True) for b in (0, 1)}
        assert {(16 if r[0][2] < 32 else 32, r[8]['igemm_variant']) for r in BASE} == {(tw, v) for tw in (16, 32) for v in (0, 1, 2)}
        got = {}
        for row in PWS:
            shape, Kp, _, Np, _, bias, relu, mode, tune, _ = row
            kind, nrows, ids = _plan(shape, Kp, Np, dcode, _td(tune), mode == 'bn', not bias and not relu and mode != 'stats')
            got.setdefault(kind, []).append((row, nrows, int(ids.max()) + 1, _tiling(*shape, 32 if shape[2] >= 32 else 16, 8 if shape[2] >= 32 else 16)[1]))
        assert set(got) == {0, 1, 2}
        walks = [(nrows, ntm) for _, nrows, _, ntm in got[2] if ntm > nrows]
        assert walks and all(ntm % nrows for nrows, ntm in walks), 'a workgroup walks several tiles, the last round ragged'
        assert any(nrows == ntm and ntm in (1, 3) for _, nrows, _, ntm in got[2]), 'gm clamped to the tile count'
        declined = {r[0][1] for k in (0, 1) for r in got.get(k, []) if r[0][7] != 'bn'}
        assert declined == ({32, 96} if dcode == 1 else set()), declined
        assert {1, 2, 4} == {min({1: 2, 3: 4, 4: 1}[r[8]['igemm_ws']], 4 if r[0][2] >= 32 else 2) for r in WS if r[0][2] >= 32}
        assert {1, 2} == {min({1: 2, 3: 4, 4: 1}[r[8]['igemm_ws']], 2) for r in WS if r[0][2] < 32}
        assert any(_plan(r[0], r[1], r[3], dcode, _td(r[8]), False, False)[1] * -(-r[3] // 64) % 8 for r in WS)


@pytest.mark.parametrize('name,dcode', DT)
def test_border_table_refusals(C, name, dcode):
    """relu | CLAMD_BIAS_BORDER_CLASSES where the table cannot be honoured: status -1, the message, nothing launched (the output and the
    statistics rows the call names are untouched)."""
    L, s = C._lib, C._lib.stream_ptr()
    rng = np.random.default_rng(1700)
    for why, shape, tune, with_bias in (('the baseline structure', S16, _t(B0), True), ('the producer/consumer structure', S16, _t(W0, igemm_ws=1), True),
                                        ('bias NULL', S16, _t(P0), False), ('H = 1', P5, _t(P0), True), ('W = 1', (2, 5, 1), _t(P0), True)):
        B, H, W = shape
        npix, Kp, Np = B * H * W, 64, 64
        x, _, wp, tab, _, _ = _conv3_inputs(rng, dcode, True, shape, Kp, Np, 'tab')
        xa, wdev, tn = _half(C, npix, Kp, 1, dcode, x), _stored(C, wp, dcode), _tuning(C, tune)
        nrows = L.stat_rows(L.OP_CONV3X3, B, H, W, Kp, Np, dcode, False, tn)          # a launch that would pass the row check
        out, st = _half(C, npix, Np, 1, dcode), Rows(nrows, 2, Np)
        rc = L.load().clamd_conv3x3(xa.ptr, xa.ldc, L.ptr(wdev), L.ptr(tab) if with_bias else None, out.ptr, out.ldc, st.ptr, None, None, nrows,
                                    B, H, W, Kp, Np, 3, 0, dcode, tn.ref(), s)
        _sync()
        msg = L.load().clamd_last_error().decode()
        assert rc == -1 and 'border-class bias table' in msg, (why, rc, msg)
        assert torch.equal(_raw(out.buf), _raw(out.before)) and torch.equal(_raw(st.buf), _raw(st.before)), f'{why}: a refused launch wrote'


# -------------------------------------------------------------------------------------------------------------------------- clamd_wgrad
def _id(p):
    return (p, p, p)


#         mode shape  Rp   (R, seg0, seg0p)  Cp   (C, seg0, seg0p)  a  b  tuning
WGRAD = [(0, S16, 32, _id(32), 32, _id(32), 1, 1, dict(wgrad_ws=0)),
         (0, S32A, 32, (21, 21, 32), 64, (40, 40, 64), 2, 2, dict(wgrad_ws=1, wgrad_dma=1)),               # rt ct = 1: no LDS-DMA
         (0, S32B, 128, _id(128), 64, (40, 20, 32), 1, 2, dict(wgrad_ws=1, wgrad_dma=1)),                   # rt ct = 2: wgrad_dma_kernel<32>
         (0, S16, 64, (60, 60, 64), 64, _id(64), 1, 1, dict(wgrad_ws=1, wgrad_dma=2)),                      # wgrad_dma_kernel<16>
         (0, S32A, 32, _id(32), 32, (21, 21, 32), 1, 1, dict(wgrad_ws=0, wgrad_tw16=1)),
         (0, S32B, 64, _id(64), 64, _id(64), 1, 1, dict(wgrad_ws=1, wgrad_dma=0, wgrad_tw16=1, wgrad_xcd=0, wgrad_blocks=14)),
         (0, S32B, 64, _id(64), 64, _id(64), 1, 1, dict(wgrad_ws=1, wgrad_dma=2, wgrad_tw16=1, wgrad_xcd=1, wgrad_blocks=10)),
         (0, S16, 32, _id(32), 64, _id(64), 1, 1, dict(wgrad_ws=0, wgrad_blocks=1)),                        # nsplit 1
         (0, S16, 64, _id(64), 32, _id(32), 1, 1, dict(wgrad_ws=0, wgrad_blocks=2)),                        # nsplit 2
         (0, S16, 32, (21, 21, 32), 32, (27, 27, 32), 1, 1, dict(wgrad_ws=0, wgrad_blocks=7, wgrad_xcd=1)),  # 7 (bf16: 6) workgroups
         (0, (1, 33, 18), 32, _id(32), 32, _id(32), 1, 1, dict(wgrad_ws=0, wgrad_blocks=4, wgrad_xcd=0)),   # 18 (bf16: 10) tiles in 4 slabs of 5 (3): a short last slab
         (0, (1, 33, 18), 32, _id(32), 32, _id(32), 1, 1, dict(wgrad_ws=0, wgrad_blocks=8, wgrad_xcd=0, cu_reserve=128)),   # the target halved: the same plan
         (0, (4, 32, 64), 32, _id(32), 32, _id(32), 1, 1, dict(wgrad_ws=0)),                                # nsplit >= 64, 9216 elements: <16>
         (0, U16, 64, _id(64), 64, _id(64), 1, 1, dict(wgrad_ws=1)),
         (0, U32, 32, _id(32), 32, _id(32), 1, 1, dict(wgrad_ws=0)),
         (0, P1, 32, (21, 21, 32), 32, (27, 27, 32), 1, 1, dict(wgrad_ws=0)),
         (0, P5, 32, _id(32), 32, _id(32), 1, 1, dict(wgrad_ws=1, wgrad_dma=2)),
         (0, P22, 64, (40, 20, 32), 32, _id(32), 1, 1, dict(wgrad_ws=0)),
         (0, P44, 32, _id(32), 64, (40, 20, 32), 1, 1, dict(wgrad_ws=1)),
         (1, S16, 32, (21, 21, 32), 64, (40, 40, 64), 1, 2, dict()),
         (1, S32A, 64, _id(64), 32, _id(32), 2, 1, dict()),
         (1, S32B, 32, (21, 21, 32), 32, _id(32), 1, 1, dict(wgrad_tw16=1, wgrad_blocks=5)),
         (1, (4, 32, 64), 64, _id(64), 64, (40, 20, 32), 1, 1, dict()),                                     # nsplit >= 64, 4096 elements: <64>
         (1, (4, 32, 64), 64, _id(64), 64, _id(64), 1, 1, dict(wgrad_blocks=40)),                           # nsplit 32 .. 63: <16>
         (2, S16, 64, (40, 20, 32), 32, (21, 21, 32), 1, 1, dict()),                                        # two-segment R
         (2, S32A, 32, _id(32), 64, _id(64), 2, 2, dict()),
         (2, S32B, 32, (27, 27, 32), 32, (21, 21, 32), 1, 1, dict(wgrad_tw16=1, wgrad_blocks=6)),
         (2, (4, 32, 64), 32, _id(32), 64, _id(64), 1, 1, dict()),                                          # nsplit >= 64, 8192 elements: <64>
         (2, P22, 32, _id(32), 32, _id(32), 1, 1, dict())]


def _wg_map(m, Lp):
    """(L, seg0, seg0p) -> physical channel -> logical channel | -1, as include/clamd.h words it."""
    L, seg0, seg0p = m
    out = []
    for p in range(Lp):
        if p < seg0p:
            out.append(p if p < seg0 else -1)
        else:
            out.append(seg0 + (p - seg0p) if seg0 + (p - seg0p) < L else -1)
    assert sorted(l for l in out if l >= 0) == list(range(L))
    return out


def _wgrad_expect(dcode, exact, mode, shape, Rp, rmap, Cp, cmap, tune, seed):
    """Everything the launch is compared with, from the inputs alone (no library call): the operands, the split plan, the float64 gradient
    of all physical channels (what the slabs add up to) and of the logical ones, the sum of the absolute terms."""
    npix = shape[0] * shape[1] * shape[2]
    rng, nb = np.random.default_rng(seed), 4 * npix if mode == 2 else npix
    # padded channels hold values too: the reduce kernel must leave them out
    a = (_weights if mode != 2 else _acts)(rng, (npix, Rp), dcode, exact)          # CONV3, PW: a is a gradient; UP2: the ConvTranspose2d input
    b = (_acts if mode != 2 else _weights)(rng, (nb, Cp), dcode, exact)
    pl = _wgrad_plan(mode, shape, Rp, Cp, dcode, _td(tune))
    full, mag = _wgrad_ref(mode, a, b, shape)
    if exact:
        assert float(mag.max()) * _grain(exact) < 2 ** 24
    rl, cl = _live(_wg_map(rmap, Rp)), _live(_wg_map(cmap, Cp))
    return a, b, pl, full, full[rl][:, cl], mag[rl][:, cl]


def _wgrad_case(C, what, dcode, exact, mode, shape, Rp, rmap, Cp, cmap, am, bm, tune, seed):
    L, s = C._lib, C._lib.stream_ptr()
    B, H, W = shape
    npix = B * H * W
    nb = 4 * npix if mode == 2 else npix
    a, b, pl, full, ref, mag = _wgrad_expect(dcode, exact, mode, shape, Rp, rmap, Cp, cmap, tune, seed)
    NT, need = pl['NT'], pl['nsplit'] * pl['NT'] * Rp * Cp
    what = f'{what} [nsplit {pl["nsplit"]} per {pl["per"]} of {pl["ntiles"]} tiles, TW {pl["TW"]}, reduce<{pl["reduce"]}>{", LDS-DMA" if pl["dma"] else ""}]'
    assert 4 * need <= L.load().clamd_wgrad_workspace_bytes(mode, B, H, W, Rp, Cp, dcode)
    aa, ba, tn = _half(C, npix, Rp, am, dcode, a), _half(C, nb, Cp, bm, dcode, b), _tuning(C, tune)
    args = (B, H, W, Rp, Cp, rmap[0], cmap[0], rmap[1], rmap[2], cmap[1], cmap[2], dcode, tn.ref(), s)

    def launch(short=0):
        out, ws = Rows(rmap[0], cmap[0], NT), Rows(need)
        rc = L.load().clamd_wgrad(mode, aa.ptr, aa.ldc, ba.ptr, ba.ldc, ws.ptr, 4 * need - short, out.ptr, *args)
        _sync()
        if short:
            msg = L.load().clamd_last_error().decode()
            assert rc == -1 and 'workspace too small' in msg, (what, rc, msg)
            assert torch.equal(_raw(out.buf), _raw(out.before)) and torch.equal(_raw(ws.buf), _raw(ws.before)), what + ': a refused launch wrote'
        else:
            L.check(rc, 'clamd_wgrad')
        return [out, ws]

    launch(short=1)                                         # nsplit is what this file's rule says: one byte less than its slabs is refused
    out, ws = _twice(what, launch)
    assert aa.guards_intact() and torch.equal(_raw(aa.buf), _raw(aa.before)) and ba.guards_intact() and torch.equal(_raw(ba.buf), _raw(ba.before))
    assert not bool(torch.isnan(out.view).any()), what + ': a logical element was not written'
    if exact:
        assert float(mag.max()) * _grain(exact) < 2 ** 24
        _expect_rows(what, out, ref.float())
        slabs = ws.view.view(pl['nsplit'], Rp, Cp, NT).double().sum(0)          # [split][r][c][tap]: the parameter's element order
        assert torch.equal(slabs, full), what + ': the split-K slabs do not add up to the integer sum'
    else:
        n = npix * (3 if dcode == 2 else 1) + pl['nsplit']
        _per_element(what, ('wgrad ' + ('CONV3', 'PW', 'UP2')[mode], dcode), out.view, ref, _acc_bound('wgrad', dcode, n, mag, mag))


@pytest.mark.parametrize('name,dcode', DT)
def test_wgrad_exact(C, name, dcode):
    for i, row in enumerate(WGRAD):
        _wgrad_case(C, f'wgrad {name} exact {row}', dcode, True, *row, seed=2000 + i)


@pytest.mark.parametrize('name,dcode', DT)
def test_wgrad_random(C, name, dcode):
    for i, row in enumerate(WGRAD):
        _wgrad_case(C, f'wgrad {name} random {row}', dcode, False, *row, seed=2100 + i)


@pytest.mark.parametrize('flavour', ['lo_a', 'lo_w'])
def test_wgrad_bf16x3_live_lo_exact(C, flavour):
    """As test_conv3x3_bf16x3_live_lo_exact: the gradient (lo_w) or the activation (lo_a) operand carries a live lo plane, the other is
    integer; the rows of up to 1024 pixels, where every sum of absolute terms stays below 2^16 (asserted)."""
    for i, row in enumerate(WGRAD):
        if row[1][0] * row[1][1] * row[1][2] <= 1024:
            _wgrad_case(C, f'wgrad bf16x3 exact, live lo ({flavour}) {row}', 2, flavour, *row, seed=2200 + i)


def check_wgrad_plans():
    """The WGRAD rows reach every reduce kernel, every class of nsplit, a short last slab, both tile widths and (bf16) both LDS-DMA kernels and
    both sides of the heuristic, for every dtype -- from this file's copy of clamd_wgrad's rule (no launch, no device: test_host_cpu.py
    runs it)."""
    for _, dcode in DT:
        plans = [(row, _wgrad_plan(row[0], row[1], row[2], row[4], dcode, _td(row[8]))) for row in WGRAD]
        assert {p['reduce'] for _, p in plans} == {1, 4, 16, 64}
        ns = [p['nsplit'] for _, p in plans]
        assert 1 in ns and 2 in ns and any(3 <= n < 32 for n in ns) and any(32 <= n < 64 for n in ns) and any(n >= 64 for n in ns)
        assert any(p['reduce'] == 16 and p['nsplit'] >= 64 for _, p in plans)
        assert any(p['ntiles'] % p['per'] for _, p in plans), 'a last slab with fewer tiles'
        halved = [p for r, p in plans if r[8].get('cu_reserve')]
        assert halved and all(p['nsplit'] == 4 and _wgrad_plan(0, (1, 33, 18), 32, 32, dcode, _td(dict(wgrad_ws=0, wgrad_blocks=8)))['nsplit'] > 4 for p in halved)
        for mode in (0, 1, 2):
            assert {p['TW'] for r, p in plans if r[0] == mode} == ({16} if dcode == 2 and mode == 0 else {16, 32})
        assert {p['ws'] for r, p in plans if r[0] == 0} == {False, True}
        for xcd in (0, 1):
            assert any(p['grid'] % 8 for r, p in plans if _td(r[8])['wgrad_xcd'] == xcd)
        if dcode == 1:
            assert {p['TW'] for _, p in plans if p['dma']} == {16, 32}
            h = [(r[2] > 64 or r[4] > 64, p['dma']) for r, p in plans if p['ws'] and _td(r[8])['wgrad_dma'] == 1]
            assert (True, True) in h and (False, False) in h
        else:
            assert not any(p['dma'] for _, p in plans)


def check_exact_conditions():
    """The 2^24 conditions of every exact case, from the references alone (no library call, no device: test_host_cpu.py runs it): the inputs
    and the expectations of every row as the GPU tests build them -- _conv3_expect and _wgrad_expect assert that every output element's and every
    statistics / five-sum row's per-channel sum of absolute terms stays below 2^24 (2^24 grains of 2^-8 with a live lo plane)."""
    cases = [(dcode, True, lst, seed0) for _, dcode in DT for lst, seed0 in ((BASE, 1000), (WS, 1200), (PWS, 1400), (PACKED, 1600))]
    cases += [(2, flavour, lst, seed0) for flavour in ('lo_a', 'lo_w') for lst, seed0 in ((BASE, 1800), (WS, 1830), (PWS, 1860))]
    for dcode, exact, lst, seed0 in cases:
        for i, row in enumerate(lst):
            shape, Kp, _, Np, _, bias, relu, mode, tune = row[:9]
            mode = mode if exact is True else ''
            x, _, wp, tab, y, _ = _conv3_inputs(np.random.default_rng(seed0 + i), dcode, exact, shape, Kp, Np, bias, row[10] if len(row) > 10 else None)
            _conv3_expect(dcode, exact, shape, Kp, Np, bias, relu, mode, _td(tune), x, wp, tab, y)
    for dcode, exact, seed0 in [(dcode, True, 2000) for _, dcode in DT] + [(2, 'lo_a', 2200), (2, 'lo_w', 2200)]:
        for i, row in enumerate(WGRAD):
            if exact is True or row[1][0] * row[1][1] * row[1][2] <= 1024:
                _wgrad_expect(dcode, exact, row[0], row[1], row[2], row[3], row[4], row[5], row[8], seed0 + i)
