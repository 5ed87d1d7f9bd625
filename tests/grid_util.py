"""Shared helpers of the per-element GPU grid tests (test_bn_grid_gpu.py, test_pointwise_grid_gpu.py, test_conv3_grid_gpu.py,
test_wino_wgrad_grid_gpu.py, test_wino_pre_fwd_grid_gpu.py, test_sgd_gpu.py, test_adam_grid_gpu.py): poisoned buffers with guard bands, the second half of a concat buffer, host-generated inputs, the bit-for-bit
expectations, the two-runs check, the storage rounding of the three dtypes, the per-element comparison against a float64 reference and the
float64 weight-gradient reference (a sum over pixels per tap), and what the two Winograd files share: the transform matrices, the tile
geometry of the pre-transformed forms and the V / Yt / U layouts."""
import math

import numpy as np
import torch

DEV = torch.device('cuda', 0)
EPS = 2.0 ** -24
STORE_REL = {0: 0.0, 1: 2.0 ** -8, 2: 2.0 ** -16 + EPS * (1 + 2.0 ** -16)}
POISON = 7.5                                  # exact in bf16 too
GUARD = 64                                    # elements: 256 bytes of fp32 (a bf16x3 base stays 64-byte aligned), 128 of bf16
EXTRA_ROWS = 3
RATIOS = {}                                   # (kernel, dtype) -> largest error / bound seen (printed by every case)


def _raw(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


class Act:
    """`npix` pixels x `cp` channels at pitch `ldc` in the storage of dtype code `dcode`, inside a buffer poisoned in front, behind and in
    the pitch gap.  Filled with `values` (fp32 [npix, cp], values the storage holds exactly) or NaN."""

    def __init__(self, C, npix, cp, ldc, dcode, values=None):
        self.C, self.npix, self.cp, self.ldc, self.dcode = C, npix, cp, ldc, dcode
        self.buf = torch.full((2 * GUARD + npix * ldc,), POISON, dtype=C.ops.TORCH_DT[dcode], device=DEV)
        self.view = self.buf[GUARD:GUARD + npix * ldc].view(npix, ldc)
        assert DEV.type != 'cuda' or self.view.data_ptr() % 64 == 0
        v = torch.full((npix, cp), float('nan'), device=DEV) if values is None else values.to(DEV, torch.float32)
        self.view[:, :cp] = C.ops.split_encode(v) if dcode == 2 else v.to(self.buf.dtype)
        self.before = self.buf.clone()

    @property
    def ptr(self):
        return self.view.data_ptr()

    def get(self):
        s = self.view[:, :self.cp]
        return self.C.ops.split_decode(s) if self.dcode == 2 else s.float()

    def guards_intact(self):
        a = self.buf.clone()
        a[GUARD:GUARD + self.npix * self.ldc].view(self.npix, self.ldc)[:, :self.cp] = self.view_of(self.before)[:, :self.cp]
        return torch.equal(_raw(a), _raw(self.before))

    def view_of(self, buf):
        return buf[GUARD:GUARD + self.npix * self.ldc].view(self.npix, self.ldc)

    def zero_bits(self):
        """[npix, cp] bool: the stored element is +0 (all bits clear; bf16x3: hi and lo)."""
        s = self.view[:, :self.cp].contiguous()
        if self.dcode != 2:
            return _raw(s) == 0
        r = s.view(torch.int16).reshape(self.npix, self.cp // 16, 2, 16)
        return ((r[:, :, 0] == 0) & (r[:, :, 1] == 0)).reshape(self.npix, self.cp)


class Rows:
    """fp32 [n, *shape] (partial rows, or a C-sized vector with n = C) with guard bands and, behind the n rows, EXTRA_ROWS poisoned rows."""

    def __init__(self, n, *shape, fill=float('nan'), dtype=torch.float32):
        per = math.prod(shape) if shape else 1
        self.n, self.per = n, per
        self.buf = torch.full((2 * GUARD + (n + EXTRA_ROWS) * per,), POISON if dtype.is_floating_point else int(POISON), dtype=dtype, device=DEV)
        self.view = self.buf[GUARD:GUARD + n * per].view(n, *shape)
        self.view.fill_(fill)
        self.before = self.buf.clone()

    @property
    def ptr(self):
        return self.view.data_ptr()

    def guards_intact(self):
        a = self.buf.clone()
        a[GUARD:GUARD + self.n * self.per] = self.before[GUARD:GUARD + self.n * self.per]
        return torch.equal(_raw(a), _raw(self.before))


class Banded:
    """fp32 tensors of `sizes` inside one flat poisoned buffer, tensor i starting at element phase phases[i] (mod 4) behind a guard band."""

    def __init__(self, sizes, phases, values=None):
        offs, cur = [], 0
        for n, ph in zip(sizes, phases):
            start = (cur + 3) // 4 * 4 + GUARD + ph
            offs.append(start)
            cur = start + n
        self.offs = offs
        self.flat = torch.full((cur + GUARD + 3,), POISON, dtype=torch.float32, device=DEV)
        assert self.flat.data_ptr() % 16 == 0
        self.views = [self.flat[o:o + n] for o, n in zip(offs, sizes)]
        self.guard = torch.ones(self.flat.shape, dtype=torch.bool, device=DEV)
        for o, n in zip(offs, sizes):
            self.guard[o:o + n] = False
        if values is not None:
            for v, x in zip(self.views, values):
                v.copy_(x)
        self.before = self.flat.clone()
        for v, ph in zip(self.views, phases):
            assert (v.data_ptr() // 4) % 4 == ph

    def restore(self):
        self.flat.copy_(self.before)

    def guards_intact(self):
        return bool(torch.equal(self.flat[self.guard].view(torch.int32), self.before[self.guard].view(torch.int32)))


def _twice(what, launch):
    """launch() -> list of Act / Rows it wrote (synchronised).  Twice: the same bits; guard bands intact."""
    a, b = launch(), launch()
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.guards_intact() and y.guards_intact(), f'{what}: output {i}: a store outside the written region'
        assert torch.equal(_raw(x.buf), _raw(y.buf)), f'{what}: output {i}: two runs differ'
    return a


def _store_round(x, dcode):
    """The fp32 value that the storage of `dcode` holds for the fp32 value x (Vec8<T>::store, then Vec8<T>::load)."""
    if dcode == 0:
        return x.clone()
    hi = x.to(torch.bfloat16).float()
    return hi if dcode == 1 else hi + (x - hi).to(torch.bfloat16).float()


def _per_element(what, key, got, ref, bound):
    """|got - ref| <= bound for every element; the worst element's index and error / bound on failure (and printed always)."""
    err = (got.double() - ref).abs()
    ratio = torch.where(err <= bound, err / bound.clamp_min(1e-300), torch.full_like(err, float('inf')))
    ratio = torch.where(err == 0, torch.zeros_like(err), ratio)
    worst = float(ratio.max())
    idx = np.unravel_index(int(ratio.argmax()), tuple(ratio.shape))
    RATIOS[key] = max(RATIOS.get(key, 0.0), worst)
    print(f'{what}: worst error / bound {worst:.3f} at {idx} (largest so far for {key}: {RATIOS[key]:.3f})')
    assert worst <= 1.0, (f'{what}: element {idx}: got {float(got[idx])!r}, reference {float(ref[idx])!r}, bound {float(bound[idx]):.3e}, '
                          f'error / bound {worst:.3f}')


# ------------------------------------------------------------------------------------------------------------------------------ buffers
class ActAt(Act):
    """An Act whose `cp` channels start at channel `c0` of the pitch: the second half of a concat buffer, the first half poisoned."""

    def __init__(self, C, npix, cp, ldc, dcode, c0=0, values=None):
        super().__init__(C, npix, cp, ldc, dcode, values)
        self.c0 = c0
        if c0:
            filled = self.view[:, :cp].clone()
            self.buf.fill_(POISON)
            self.view = self.view_of(self.buf)
            self.view[:, :cp] = filled
            self.before = self.buf.clone()

    def view_of(self, buf):
        return buf.as_strided((self.npix, self.ldc - self.c0), (self.ldc, 1), GUARD + self.c0)

    def guards_intact(self):
        a = self.buf.clone()
        self.view_of(a)[:, :self.cp] = self.view_of(self.before)[:, :self.cp]
        return torch.equal(_raw(a), _raw(self.before))


def _half(C, npix, cp, mult, dcode, values=None):
    """mult 1: the tensor at its own pitch; 2: the second half of a buffer of pitch 2 cp."""
    return ActAt(C, npix, cp, mult * cp, dcode, (mult - 1) * cp, values)


def _expect_bits(what, out, exp32):
    """The stored bits of `out` are storage(exp32) (fp32 [npix, cp]); the worst element on failure."""
    exp = out.C.ops.split_encode(exp32.contiguous()) if out.dcode == 2 else exp32.to(out.buf.dtype)
    got = out.view[:, :out.cp].contiguous()
    if torch.equal(_raw(got), _raw(exp)):
        return
    gv, ev = out.get().double(), _store_round(exp32, out.dcode).double()
    d = torch.nan_to_num((gv - ev).abs(), nan=float('inf'))
    idx = np.unravel_index(int(d.argmax()), tuple(d.shape))
    raise AssertionError(f'{what}: {int((d != 0).sum())} elements differ from storage(exact result); worst at (pixel, channel) {idx}: '
                         f'got {float(gv[idx])!r}, expected {float(ev[idx])!r}' + (' (the values agree: a sign of zero)' if not bool(d.any()) else ''))


def _expect_rows(what, rows, exp):
    """fp32 / int64 rows equal `exp` bit for bit; the worst element on failure."""
    got = rows.view.reshape(exp.shape)
    if torch.equal(_raw(got.contiguous()), _raw(exp.to(got.dtype).contiguous())):
        return
    d = torch.nan_to_num((got.double() - exp.double()).abs(), nan=float('inf'))
    idx = np.unravel_index(int(d.argmax()), tuple(d.shape))
    raise AssertionError(f'{what}: {int((d != 0).sum())} elements differ; worst at {idx}: got {float(got[idx])!r}, expected {float(exp[idx])!r}')


def _expect_vals(what, got, exp):
    """`got` equals the float64 `exp` element for element as NUMBERS (a zero's sign is free, NaN never passes); the worst element on failure."""
    got = got.reshape(exp.shape).double()
    if torch.equal(got, exp):
        return
    d = torch.nan_to_num((got - exp).abs(), nan=float('inf'))
    idx = np.unravel_index(int(d.argmax()), tuple(d.shape))
    raise AssertionError(f'{what}: {int((d != 0).sum())} of {d.numel()} elements differ; worst at {idx}: got {float(got[idx])!r}, expected {float(exp[idx])!r}')


# ------------------------------------------------------------------------------------------------------------------------------- inputs
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ints(rng, shape, amax, zeros):
    """Integers in [-amax, amax] with `zeros` of them cleared on top of the uniform share: about a quarter zeros in all."""
    v = rng.integers(-amax, amax + 1, size=shape)
    v[rng.random(shape) < zeros] = 0
    return _dev(v.astype(np.float32))


def _normal(rng, shape, dcode, zeros=0.25):
    """Standard normal, a quarter exact zeros, rounded to what the storage holds; bf16x3: lo = rne(x - hi) kept where |lo| <= 2^-9 |x|."""
    x = torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    x[torch.from_numpy(rng.random(shape) < zeros)] = 0.0
    if dcode:
        hi = x.to(torch.bfloat16).float()
        lo = (x - hi).to(torch.bfloat16).float()
        x = hi if dcode == 1 else hi + torch.where(lo.abs() <= 2.0 ** -9 * (hi + lo).abs(), lo, torch.zeros(()))
    x = x.to(DEV)
    assert torch.equal(_store_round(x, dcode), x)
    if dcode == 2:
        hi = x.to(torch.bfloat16).float()
        assert bool((x != hi).any()) and bool(((x - hi).abs() <= 2.0 ** -9 * x.abs()).all())
    return x


def _pad2(w, n, k):
    out = torch.zeros(n, k, device=w.device, dtype=w.dtype)
    out[:w.shape[0], :w.shape[1]] = w
    return out


def _operand(C, w, dcode):
    """fp32 [..., K] in a documented packed layout -> the device operand of the compute dtype (bf16x3: split on the innermost dimension)."""
    w = w.contiguous()
    return C.ops.split_encode(w) if dcode == 2 else w.to(C.ops.TORCH_DT[dcode])


# --------------------------------------------------------------------------------------------------------------------------- references
def _wgrad_ref(mode, a, b, shape):
    """a [npix, Rp], b [npix | 4 npix, Cp] (fp32 values) -> float64 [Rp][Cp][taps] = sum over pixels of a[p, r] b[nbr_t(p), c] and the sum of the
    absolute terms.  CONV3: nbr_t(p) = p + (ky - 1, kx - 1), zero outside the image; PW: p; UP2: (2 y + dy, 2 x + dx), t = 2 dy + dx."""
    B, H, W = shape
    Cp, ad = b.shape[1], a.double()
    if mode == 0:
        pad = torch.zeros(B, H + 2, W + 2, Cp, dtype=torch.float64, device=a.device)
        pad[:, 1:H + 1, 1:W + 1] = b.double().view(B, H, W, Cp)
        taps = [pad[:, ky:ky + H, kx:kx + W].reshape(B * H * W, Cp) for ky in range(3) for kx in range(3)]
    elif mode == 1:
        taps = [b.double()]
    else:
        bv = b.double().view(B, H, 2, W, 2, Cp)
        taps = [bv[:, :, dy, :, dx].reshape(B * H * W, Cp) for dy in range(2) for dx in range(2)]
    return torch.stack([ad.T @ t for t in taps], -1), torch.stack([ad.abs().T @ t.abs() for t in taps], -1)


# ------------------------------------------------------------------------------ Winograd: the matrices, as the kernel comments print them
BT4 = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
BT6 = [[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]]
A4 = [[1, 0], [1, 1], [1, -1], [0, -1]]
A6 = [[1, 0, 0, 0], [1, 1, 1, 1], [1, -1, 1, -1], [1, 2, 4, 8], [1, -2, 4, -8], [0, 0, 0, 1]]
G4 = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]
G6 = [[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]]
# th x tw output tile; (rows, columns) matrices; roundings of the two transforms and of the reduce's G^T . G, counted in the docstring of
# test_wino_wgrad_grid_gpu.py
FORM = {22: dict(th=2, tw=2, BT=(BT4, BT4), A=(A4, A4), G=(G4, G4), nV=2, nY=2, nG=4),
        24: dict(th=2, tw=4, BT=(BT4, BT6), A=(A4, A6), G=(G4, G6), nV=3, nY=3, nG=7),
        44: dict(th=4, tw=4, BT=(BT6, BT6), A=(A6, A6), G=(G6, G6), nV=4, nY=4, nG=10)}
# sign conventions of what the kernels keep in memory, (plane rows i, plane columns j) that are stored negated (the reduce flips them back):
# V of the pre-transformed F(2x4) form carries row 2 of B4^T negated; the in-kernel kernels leave out the sign of B4^T row 2 and of A4 row 3,
# and F(2x2) also that of A4's column 3
SIGN = {'pre24': ((2,), ()), 'pre44': ((), ()), 'ink24': ((2, 3), ()), 'ink22': ((2, 3), (3,))}


def _m(rows, absolute=False):
    t = torch.tensor(rows, dtype=torch.float64, device=DEV)
    return t.abs() if absolute else t


def _planes_n(form):
    return len(FORM[form]['BT'][0]), len(FORM[form]['BT'][1])


def _sign(kind, form):
    """[ni * nj] float64: -1 where the stored plane is the negated true one."""
    ni, nj = _planes_n(form)
    s = torch.ones(ni, nj, dtype=torch.float64, device=DEV)
    for i in SIGN[kind][0]:
        s[i] *= -1
    for j in SIGN[kind][1]:
        s[:, j] *= -1
    return s.reshape(-1)


# --------------------------------------------------------------------------------------------------- Winograd: tile geometry and layouts
def _geom(form, shape):
    """Tile blocks of the pre-transformed forms: 32 tiles each, 8 across x 4 down (W >= 32) or 4 across x 8 down; tile t = 32 * block + tile in
    block, blocks x fastest, then y, then the image (w24_tile / w44_block)."""
    B, H, W = shape
    th = FORM[form]['th']
    TXN = 8 if W >= 32 else 4
    TYN = 32 // TXN
    PW, PH = 4 * TXN, th * TYN
    bx, by = -(-W // PW), -(-H // PH)
    return dict(TXN=TXN, TYN=TYN, PW=PW, PH=PH, bx=bx, by=by, ntm=B * bx * by, Tp=32 * B * bx * by, th=th)


def _tile_origin(g, t):
    """Tile t -> (image, first output row, first output column)."""
    tm, r = divmod(t, 32)
    b, rem = divmod(tm, g['bx'] * g['by'])
    yb, xb = divmod(rem, g['bx'])
    return b, yb * g['PH'] + g['th'] * (r // g['TXN']), xb * g['PW'] + 4 * (r % g['TXN'])


def _tile_of(g, b, y, x):
    """The tile that holds output pixel (b, y, x): the inverse of _tile_origin."""
    yb, xb = y // g['PH'], x // g['PW']
    r = ((y % g['PH']) // g['th']) * g['TXN'] + (x % g['PW']) // 4
    return ((b * g['by'] + yb) * g['bx'] + xb) * 32 + r


def _v_index(t, pl, c, Cp, P):
    """Float offset of (tile t, plane pl = 6 i + j, channel c) in V [tile block][Cp / 8][P][2][32][4]."""
    return (((t >> 5) * (Cp // 8) + c // 8) * P + pl) * 256 + ((c % 8) // 4) * 128 + (t & 31) * 4 + c % 4


def _v_unindex(off, Cp, P):
    off, e = divmod(off, 4)
    off, r = divmod(off, 32)
    off, h = divmod(off, 2)
    off, pl = divmod(off, P)
    tm, kc = divmod(off, Cp // 8)
    return 32 * tm + r, pl, 8 * kc + 4 * h + e


def _yt_index(t, pl, r, Tp, Rp):
    """Float offset of (plane, tile, channel) in Yt [P][Tp][Rp]."""
    return (pl * Tp + t) * Rp + r


def _v_layout(V):
    """[Tp, P, Cp] -> V as the kernels store it, [Tp / 32][Cp / 8][P][2][32][4], flat."""
    Tp, P, Cp = V.shape
    return V.reshape(Tp // 32, 32, P, Cp // 8, 2, 4).permute(0, 3, 2, 4, 1, 5).reshape(-1)


def _patches(v, shape, th, tw, halo, Hp, Wp):
    """[npix, Ch] -> float64 [B, Hp / th, Wp / tw, Ch, th + 2 halo, tw + 2 halo]: every tile's patch of the image zero-padded to Hp x Wp (+ halo)."""
    B, H, W = shape
    pad = torch.zeros(B, Hp + 2 * halo, Wp + 2 * halo, v.shape[1], dtype=torch.float64, device=v.device)
    pad[:, halo:halo + H, halo:halo + W] = v.double().view(B, H, W, -1)
    return pad.unfold(1, th + 2 * halo, th).unfold(2, tw + 2 * halo, tw)


def _tile_order(p, g):
    """[B, tiles down, tiles across, ...] -> [T, ...]: raster order (g None) or the block order of the pre-transformed forms."""
    if g is None:
        return p.reshape(-1, *p.shape[3:])
    rest = tuple(range(5, 5 + p.dim() - 3))
    p = p.reshape(p.shape[0], g['by'], g['TYN'], g['bx'], g['TXN'], *p.shape[3:]).permute(0, 1, 3, 2, 4, *rest)
    return p.reshape(g['Tp'], *p.shape[5:])


def _xform(form, which, v, shape, g, absolute=False):
    """The float64 contraction M_rows patch M_cols^T of every tile with the TRUE matrices (BT: input side, halo 1; A: gradient side) ->
    [T, P, Ch]; absolute: the same with |M| on |v| (what every partial sum of the transform is bounded by)."""
    f = FORM[form]
    B, H, W = shape
    Hp, Wp = (g['by'] * g['PH'], g['bx'] * g['PW']) if g else (H, W)
    p = _tile_order(_patches(v.abs() if absolute else v, shape, f['th'], f['tw'], 1 if which == 'BT' else 0, Hp, Wp), g).contiguous()
    Mr, Mc = (_m(m, absolute) for m in f[which])
    out = torch.einsum('ia,tcab,jb->tijc', Mr, p, Mc)
    return out.reshape(out.shape[0], -1, out.shape[-1])


def _wg_map(m, Lp):
    """(L, seg0, seg0p) -> the physical channels that hold a logical one, in logical order (include/clamd.h)."""
    L, seg0, seg0p = m
    out = [p for p in range(Lp) if (p < seg0 if p < seg0p else seg0 + (p - seg0p) < L)]
    assert len(out) == L
    return torch.tensor(out, dtype=torch.long, device=DEV)


def _u_index(c, pl, n, Np, P):
    """Float offset of (input channel c, plane pl = 6 i + j, output channel n) in the packed filters U [Kp / 8][P][Np][8]."""
    return (((c // 8) * P + pl) * Np + n) * 8 + c % 8


def _u_unindex(off, Np, P):
    off, k8 = divmod(off, 8)
    off, n = divmod(off, Np)
    kc, pl = divmod(off, P)
    return 8 * kc + k8, pl, n


def _u_layout(U):
    """[Kp, P, Np] -> U as the pack kernels store it, [Kp / 8][P][Np][8], flat."""
    Kp, P, Np = U.shape
    return U.reshape(Kp // 8, 8, P, Np).permute(0, 2, 3, 1).reshape(-1)


def _untile(y, g, shape):
    """[Tp, th, 4, N] output tiles in the block order of the pre-transformed forms -> the image [B, H, W, N] (tiles outside it are cropped)."""
    B, H, W = shape
    y = y.reshape(B, g['by'], g['bx'], g['TYN'], g['TXN'], g['th'], 4, -1).permute(0, 1, 3, 5, 2, 4, 6, 7)
    return y.reshape(B, g['by'] * g['PH'], g['bx'] * g['PW'], -1)[:, :H, :W]
