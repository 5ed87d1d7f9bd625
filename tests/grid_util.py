"""Shared helpers of the per-element GPU grid tests (test_bn_grid_gpu.py, test_pointwise_grid_gpu.py, test_conv3_grid_gpu.py,
test_wino_wgrad_grid_gpu.py, test_sgd_gpu.py, test_adam_grid_gpu.py): poisoned buffers with guard bands, the second half of a concat buffer, host-generated inputs, the bit-for-bit
expectations, the two-runs check, the storage rounding of the three dtypes, the per-element comparison against a float64 reference and the
float64 weight-gradient reference (a sum over pixels per tap)."""
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
