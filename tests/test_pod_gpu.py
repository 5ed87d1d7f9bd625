"""GPU: the Local POD kernels of csrc/pod.hip through the C ABI, per element, on the smallest shapes at which each mechanism can go wrong.

Every case calls clamd_local_pod_fwd_bwd with d a, the workspace and the loss inside NaN guard bands (d a itself pre-filled with NaN: an
element the kernels do not write fails the case) and compares with the float64 restatement of include/clamd.h's definition
(test_pod_cpu.pod_closed_form, which test_pod_cpu.py holds to torch autograd):
    |d a - ref64| <= c * 2^-24 * max_n |ref64|   per element, the maximum per image;   |loss - ref64| <= c_loss * 2^-24 * |ref64|.
How c was obtained (the rule of tests/test_loss_grid_gpu.py): the same formulas evaluated in plain float32 in torch on the host give
`fp32 r`, the largest ratio over this file's cases and flag combinations (test_pod_cpu.RESTATEMENT_MAX, evaluated again by
test_pod_cpu.test_fp32_restatement_stays_within_its_bound); c is that times 4, rounded up to a power of two, separately for the
independent inputs (normal a and b at scales 1 and 10: c = 64, c_loss = 32) and the close ones (a = b + 1e-3 noise, conditioned by
1 / distance once normalised: c = 32768, c_loss = 2048).  The assert message prints both ratios.

The cases (test_pod_cpu.CASES) and what each reaches in pod.hip:
  4x4 (levels 3)            one-pixel regions; wf = 1: the general row-sum form (one value per segment over the whole wave), NPX = 4
  8x12, 12x8, 16x20         wf = 3, 2, 5: general form; segments that cut a lane's four pixels
  6x6-l2, 5x7-l1            W % 4 != 0: the one-element variant (strip and gradient)
  8x12-offset, 8x16-offset  a starts 4 bytes past a 16-byte boundary: the one-element variant by alignment; 8x16: its grouped form (g = 4)
  8x16-l2, 16x32            the grouped form, 16-byte accesses: 2 lanes per segment (one shuffle); 16x32 with Ca = C + 2, Cb = C + 1
  b1, b3, c1, ca=c+2, cb=c+3   the channel cases; c1 and ca=c+2 with and without the merge
  k21-23                    the logits form at K = 21 -> 23, 64x96: 2 bands per row segment (nb = 8), several waves per row
  4x2048                    segments wider than a wave (g = 64, two slots per segment) AND the second trip of the strip kernel's column
                            loop in the 16-byte form (a workgroup covers 1024 columns per trip)
  4x1032                    the second trip in the general 16-byte form (wf = 258)
  2x261-l1                  the second trip of the one-element variant (256 columns per trip)
The strip kernel has no other loop or grid cap (its grid is bands x channels x 2 B, the gradient's pixels x channels x B, uncapped); the
finalize kernel's item loop takes a second trip whenever C (H + W) > 256, which 16x20 and every larger case do."""
import itertools
import math

import pytest
import torch

from test_pod_cpu import CASES, C_BOUND, EPS, FAMILIES, family_class, pod_closed_form, pod_inputs, pod_ratios

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
GUARD = 64
NAN = float('nan')
LAM = 0.7


@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    C._lib.load()
    return C


def _guarded(n, shift=0):
    """n floats of NaN inside a NaN buffer, 256-byte aligned plus `shift` floats."""
    buf = torch.full((n + 2 * GUARD + shift,), NAN, device=DEV)
    view = buf[GUARD + shift:GUARD + shift + n]
    assert view.data_ptr() % 256 == 4 * shift
    return buf, view


def _guards_intact(buf, view):
    lo = (view.data_ptr() - buf.data_ptr()) // 4
    return bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[lo + view.numel():]).all())


def _on_device(t, shift):
    _, v = _guarded(t.numel(), shift)
    v = v.view(t.shape)
    v.copy_(t)
    return v


def _abi(C, a, b, Cc, merge, square, normalize, levels, gs=1.0, with_da=True, lam=LAM):
    """One call -> (loss [1], d a or None).  The guard bands of d a, the workspace and the loss are checked here."""
    lib, ptr = C._lib, C._lib.ptr
    B, Ca, H, W = a.shape
    wsb = lib.load().clamd_pod_workspace_bytes(B, Cc, H, W, levels)
    assert wsb > 0 and wsb % 16 == 0
    wbuf, ws = _guarded(wsb // 4)
    lbuf, loss = _guarded(1)
    dbuf, d = _guarded(a.numel()) if with_da else (None, None)
    lib.call('clamd_local_pod_fwd_bwd', ptr(a), Ca, ptr(b), b.shape[1], Cc, int(merge), int(square), int(normalize), levels, lam,
             ptr(d), ptr(loss), ptr(ws), wsb, B, H, W, float(gs), lib.stream_ptr())
    torch.cuda.synchronize()
    assert _guards_intact(wbuf, ws) and _guards_intact(lbuf, loss), 'a store outside the workspace or the loss'
    if with_da:
        assert _guards_intact(dbuf, d), 'a store outside d a'
        d = d.view(a.shape)
    return loss, d


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_case_against_the_restatement(C, case):
    name, B, Ca, Cb, Cc, H, W, levels, merges, shift = case
    for merge, family in itertools.product(merges, FAMILIES):
        ah, bh = pod_inputs(case, family, merge)
        a, b = _on_device(ah, shift), _on_device(bh, 0)
        assert a.data_ptr() % 16 == 4 * shift
        c, c_loss = C_BOUND[family_class(family)]
        for square, normalize in itertools.product((False, True), (False, True)):
            what = f'{name} {family} merge{int(merge)} square{int(square)} norm{int(normalize)}'
            l64, d64, mag = pod_closed_form(ah.double(), bh.double(), Cc, merge, square, normalize, levels, LAM)
            l32, d32, _ = pod_closed_form(ah, bh, Cc, merge, square, normalize, levels, LAM)
            r32, rl32 = pod_ratios(l32, d32, l64, d64)
            # 1. loss and d a per element
            loss, d = _abi(C, a, b, Cc, merge, square, normalize, levels)
            assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(loss).all()), what + ': an element was not written'
            rk, rlk = pod_ratios(loss.cpu()[0], d.cpu(), l64, d64)
            print(f'{what}: d a fp32 r {r32:.2f} kernel r {rk:.2f} (c {c:g}); loss fp32 r {rl32:.2f} kernel r {rlk:.2f} (c {c_loss:g})')
            assert rk <= c, (what, 'kernel r', rk, 'fp32 r', r32, 'c', c)
            assert rlk <= c_loss, (what, 'loss: kernel r', rlk, 'fp32 r', rl32, 'c', c_loss)
            # 6. channels >= C without the merge
            if not merge and Ca > Cc:
                assert int((d[:, Cc:] != 0).sum()) == 0, what
            if merge and Ca > Cc:
                assert all(torch.equal(_bits(d[:, k]), _bits(d[:, 0])) for k in range(Cc, Ca)), what
            # 2. twice: identical bits
            loss2, d2 = _abi(C, a, b, Cc, merge, square, normalize, levels)
            assert torch.equal(_bits(loss2), _bits(loss)) and torch.equal(_bits(d2), _bits(d)), what + ': two runs differ'
            # 3. without d a: the same loss bits (the guards of the workspace and the loss are checked inside)
            loss0, _ = _abi(C, a, b, Cc, merge, square, normalize, levels, with_da=False)
            assert torch.equal(_bits(loss0), _bits(loss)), what + ': the loss depends on d a'
            # 4. grad_scale: the loss does not move; d a is 0.375 x the unit-scale one up to the roundings of the two fp32 table entries,
            # their sum and (square) the product on either side: 2^-24 * 0.375 * (2 |row| + 2 |col| + 4 |row + col|) * |2 value| <= 6 * mag
            gs = 0.375
            lossg, dg = _abi(C, a, b, Cc, merge, square, normalize, levels, gs=gs)
            assert torch.equal(_bits(lossg), _bits(loss)), what
            lim = 6.0 * EPS * gs * mag * 1.01 + 1e-44
            over = (dg.cpu().double() - gs * d.cpu().double()).abs() > lim
            assert int(over.sum()) == 0, (what, 'grad_scale is not a scaling', int(over.sum()))
            assert pod_ratios(loss.cpu()[0], dg.cpu() / gs, l64, d64)[0] <= c, what
    # 5. identical tensors (C = Ca = Cb): exactly zero
    for square, normalize in itertools.product((False, True), (False, True)):
        lossi, di = _abi(C, a, a.clone(), Ca, False, square, normalize, levels)
        assert float(lossi) == 0.0 and int((di != 0).sum()) == 0, (name, square, normalize, float(lossi))


def test_refused_arguments_launch_nothing(C):
    lib, ptr = C._lib, C._lib.ptr
    a, b = torch.randn(2, 4, 8, 12, device=DEV), torch.randn(2, 3, 8, 12, device=DEV)
    wsb = lib.load().clamd_pod_workspace_bytes(2, 3, 8, 12, 3)
    wbuf, ws = _guarded(wsb // 4)
    lbuf, loss = _guarded(1)
    dbuf, d = _guarded(a.numel())

    def call(Cc=3, levels=3, H=8, W=12, wsb_=wsb):
        lib.call('clamd_local_pod_fwd_bwd', ptr(a), 4, ptr(b), 3, Cc, 1, 0, 1, levels, 1.0, ptr(d), ptr(loss), ptr(ws), wsb_, 2, H, W, 1.0,
                 lib.stream_ptr())

    for kw, msg in ((dict(Cc=0), 'C must be'), (dict(Cc=4), 'C must be'), (dict(levels=0), 'levels'), (dict(levels=4), 'levels'),
                    (dict(H=6, W=16), 'multiples'), (dict(wsb_=wsb - 16), 'workspace'), (dict(wsb_=0), 'workspace')):
        with pytest.raises(RuntimeError, match=msg):
            call(**kw)
    torch.cuda.synchronize()
    for buf in (wbuf, lbuf, dbuf):
        assert bool(torch.isnan(buf).all()), 'a refused call wrote something'
    call()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(loss).all())
