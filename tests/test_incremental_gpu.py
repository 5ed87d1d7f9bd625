"""GPU: the class-incremental task step (build-defined: the reference has no continual-learning code, parity unpinned).

clamd_ce_unbiased_fwd_bwd and UnbiasedDistillationCrossEntropy against the float64 restatement of tests/test_incremental_cpu.py (pinned
there against the closed-form gradients), head growth with the optimiser / consolidation state carried over, and a whole two-task
incremental run against the same procedure composed from stock torch ops on the same device."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

from conftest import rel_l2
from oracle import torch_cpu as TC
from test_incremental_cpu import unbiased_losses

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
DT = [('fp32', 0), ('bf16', 1), ('bf16x3', 2)]
CASES = [(21, 11, 2, 16, 16), (21, 1, 2, 16, 20), (32, 31, 1, 8, 8), (5, 5, 3, 8, 12), (21, 16, 16, 256, 256)]


@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    C._lib.load()
    return C


def _case(K, c_old, B, H, W, scale, seed=0, k_old_total=None):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, K, H, W, generator=g) * scale
    zo = torch.randn(B, k_old_total or c_old, H, W, generator=g) * scale
    y = torch.randint(0, K, (B, H, W), generator=g)
    y[0, 0, :3] = -100; y[0, 1, 0] = K + 2; y[-1, -1, -1] = -7          # ignored, out of range, negative non-ignore
    return z, zo, y


def _reference(z, y, zo, c_old, lam):
    zz = z.double().to(DEV).requires_grad_()
    tot, ce, kd = unbiased_losses(zz, y.to(DEV), None if zo is None else zo.double().to(DEV), c_old, lam)
    g, = torch.autograd.grad(tot, zz)
    return [float(tot), float(ce), float(kd)], g


def _abi(C, z, y, zo, c_old, lam, nhwc=None, dcode=0, k=None):
    """One call through the C ABI on device tensors -> (loss3, dlogits, bad-label count)."""
    lib, ptr, s = C._lib, C._lib.ptr, C._lib.stream_ptr()
    L = lib.load()
    B, K, H, W = z.shape
    wsb = L.clamd_ce_workspace_bytes()
    off = L.clamd_ce_bad_label_count_offset() // 4
    ws = torch.full((wsb // 4,), float('nan'), device=DEV)
    d, l3 = torch.empty_like(z), torch.empty(3, device=DEV)
    lib.call('clamd_ce_count', ptr(y), B, K, H, W, -100, ptr(ws), wsb, s)
    lib.call('clamd_ce_unbiased_fwd_bwd', ptr(z), ptr(y), ptr(zo), 0 if zo is None else zo.shape[1], c_old, float(lam), ptr(d),
             ptr(nhwc), 0 if nhwc is None else nhwc.shape[-1], dcode, ptr(l3), ptr(ws), wsb, B, K, H, W, -100, 1.0, s)
    torch.cuda.synchronize()
    return l3, d, int(ws[off:off + 1].view(torch.int32))


def _check(got3, gotd, ref3, refd, what, nvalid=None):
    errs = [abs(float(a) - b) / max(1.0, abs(b)) for a, b in zip(got3, ref3)]
    if nvalid is not None and float(refd.abs().max()) == 0.0:
        # no new classes and no distillation: the reference gradient is exactly zero (softmax_all == softmax_old), a relative error does not
        # exist.  The kernel subtracts two fp32 roundings of the same number <= 1 / nvalid: a few ulp of that, 8 * 2^-24 / nvalid, bounds it.
        m = float(gotd.abs().max())
        print(f'{what}: zero reference gradient, max |d logits| {m:.3e} (bound {8 * 2.0 ** -24 / nvalid:.3e})')
        assert max(errs) < 1e-5 and m <= 8 * 2.0 ** -24 / nvalid, (what, errs, m)
        return
    rd = rel_l2(gotd.double().cpu().numpy(), refd.cpu().numpy())
    print(f'{what}: loss rel errors (total, ce, kd) {errs}, d logits rel_l2 {rd:.3e}')
    assert max(errs) < 1e-5 and rd < 1e-5, (what, errs, rd)
    assert bool(torch.isfinite(gotd).all())


@pytest.mark.parametrize('K,c_old,B,H,W', CASES)
@pytest.mark.parametrize('scale', [3.0, 30.0])
def test_kernel_and_criterion_vs_restatement(C, K, c_old, B, H, W, scale):
    lam = 10.0
    z, zo, y = _case(K, c_old, B, H, W, scale, k_old_total=c_old + (1 if c_old < K else 0))
    ref3, refd = _reference(z, y, zo, c_old, lam)
    zd, zod, yd = z.to(DEV), zo.to(DEV), y.to(DEV)
    l3, d, bad = _abi(C, zd, yd, zod, c_old, lam)
    assert bad == 2
    _check(l3, d, ref3, refd, f'abi K{K} c{c_old} x{scale}')
    crit = C.UnbiasedDistillationCrossEntropy(c_old, lam)
    t = zd.clone().requires_grad_()
    loss = crit(t, yd, zod); loss.backward(); torch.cuda.synchronize()
    assert int(crit.bad_labels) == 2 and float(loss) == float(crit.parts[0])
    _check(crit.parts, t.grad, ref3, refd, f'criterion K{K} c{c_old} x{scale}')
    # the CE term alone: old_logits None, and lam == 0 with old logits given (not read)
    ref3c, refdc = _reference(z, y, None, c_old, 0.0)
    nvalid = int(((y >= 0) & (y < K)).sum())
    for zo_arg, lam_arg in ((None, lam), (zod, 0.0)):
        l3, d, _ = _abi(C, zd, yd, zo_arg, c_old, lam_arg)
        assert float(l3[2]) == 0.0
        _check(l3, d, ref3c, refdc, f'ce only K{K} c{c_old} x{scale}', nvalid=nvalid)


def test_groups_far_apart_do_not_underflow(C):
    """Old and new logits 200 apart (exp underflows in fp32): the rebased groups keep LSE(old) - LSE(all), softmax_old and LSE(bgnew) exact."""
    z, zo, y = _case(21, 11, 2, 16, 16, 3.0, seed=5)
    z[:, 11:] += 200.0
    z[1, 1:11] += 400.0          # second image: bgnew far below the other old classes
    y[0, 4:8] = 3
    ref3, refd = _reference(z, y, zo, 11, 10.0)
    l3, d, _ = _abi(C, z.to(DEV), y.to(DEV), zo.to(DEV), 11, 10.0)
    _check(l3, d, ref3, refd, 'far apart')


def test_all_pixels_ignored(C):
    z, zo, y = _case(21, 11, 1, 16, 16, 50.0)
    y[:] = -100
    l3, d, bad = _abi(C, z.to(DEV), y.to(DEV), None, 11, 0.0)
    assert bad == 0 and [float(v) for v in l3] == [0.0, 0.0, 0.0] and float(d.abs().max()) == 0.0
    l3, d, _ = _abi(C, z.to(DEV), y.to(DEV), zo.to(DEV), 11, 10.0)        # ignored labels still distil
    ref3, refd = _reference(z, y, zo, 11, 10.0)
    assert float(l3[1]) == 0.0
    _check(l3, d, ref3, refd, 'all ignored, kd only')


@pytest.mark.parametrize('K,B,H,W', [(5, 2, 8, 12), (21, 3, 16, 20), (32, 1, 4, 4), (21, 16, 256, 256)])
def test_c_old_1_without_distillation_is_the_plain_loss_bit_for_bit(C, K, B, H, W):
    """c_old == 1, lam == 0: every operation on the way to the loss and to d logits is the one clamd_ce_fwd_bwd_counted makes (same
    exponentials relative to the pixel's maximum, the same sequential sum, LSE(old) = z_0 exactly, softmax_old_0 = e_0 / e_0 = 1), so
    the results are bit-equal -- also for large logits."""
    lib, ptr, s = C._lib, C._lib.ptr, C._lib.stream_ptr()
    wsb = lib.load().clamd_ce_workspace_bytes()
    for scale in (4.0, 40.0):
        z, _, y = _case(K, 1, B, H, W, scale, seed=K)
        zd, yd = z.to(DEV), y.to(DEV)
        ws = torch.zeros(wsb // 4, device=DEV)
        d0, l0 = torch.empty_like(zd), torch.empty(3, device=DEV)
        lib.call('clamd_ce_count', ptr(yd), B, K, H, W, -100, ptr(ws), wsb, s)
        lib.call('clamd_ce_fwd_bwd_counted', ptr(zd), ptr(yd), ptr(d0), None, 0, 0, ptr(l0), ptr(ws), wsb, B, K, H, W, -100, 1.0, s)
        l1, d1, _ = _abi(C, zd, yd, None, 1, 0.0)
        ndiff = int((d0.view(torch.int32) != d1.view(torch.int32)).sum())
        assert ndiff == 0 and torch.equal(l0, l1), (K, scale, ndiff, l0.tolist(), l1.tolist())


@pytest.mark.parametrize('name,dcode', DT)
def test_nhwc_copy_and_scaled_backward(C, name, dcode):
    lib, ptr, s = C._lib, C._lib.ptr, C._lib.stream_ptr()
    for (K, c_old, B, H, W), with_kd in ((CASES[0], True), (CASES[2], True), (CASES[3], False), ((21, 11, 1, 6, 5), True)):
        z, zo, y = _case(K, c_old, B, H, W, 4.0, seed=3)
        zd, yd, zod = z.to(DEV), y.to(DEV), (zo.to(DEV) if with_kd else None)
        nh = torch.full((B, H, W, 32), 5.0, dtype=C.ops.TORCH_DT[dcode], device=DEV)
        l3, d, _ = _abi(C, zd, yd, zod, c_old, 10.0, nhwc=nh, dcode=dcode)
        l3b, db, _ = _abi(C, zd, yd, zod, c_old, 10.0)
        assert torch.equal(d, db) and torch.equal(l3, l3b)
        conv = C.ops.to_nhwc(d, dcode, cp=32)
        nbad = int((conv.view(torch.int16) != nh.view(torch.int16)).sum())
        assert nbad == 0, (name, K, H, W, nbad)
    # through the UNet: the engine takes the copy, loss * 0.5 scales both
    torch.manual_seed(0)
    m = C.UNet(21, 3, 8, compute_dtype=name).to(DEV)
    x = torch.randn(2, 3, 32, 32, device=DEV)
    yy = torch.randint(0, 21, (2, 32, 32), device=DEV)
    zo = torch.randn(2, 11, 32, 32, device=DEV)
    crit = C.UnbiasedDistillationCrossEntropy(11, 10.0)
    grads = []
    for f in (1.0, 0.5):
        out = m(x)
        m.zero_grad()
        (crit(out, yy, zo) * f).backward()
        torch.cuda.synchronize()
        grads.append(torch.cat([p.grad.reshape(-1) for p in m.parameters()]).clone())
    C.loss.HANDOVER, keep = False, C.loss.HANDOVER
    try:
        out = m(x); m.zero_grad(); crit(out, yy, zo).backward(); torch.cuda.synchronize()
    finally:
        C.loss.HANDOVER = keep
    plain = torch.cat([p.grad.reshape(-1) for p in m.parameters()])
    assert torch.equal(grads[0], plain), 'the handed-over NHWC copy and the converted NCHW gradient give different parameter gradients'
    r = float((grads[1] - 0.5 * grads[0]).norm() / (0.5 * grads[0]).norm())
    assert r < (1e-6 if name == 'fp32' else 2e-2), r


def test_odd_sizes_take_the_one_pixel_variant(C):
    for K, c_old, B, H, W in ((21, 11, 2, 7, 9), (5, 2, 1, 3, 3)):
        z, zo, y = _case(K, c_old, B, H, W, 3.0, seed=8)
        ref3, refd = _reference(z, y, zo, c_old, 10.0)
        l3, d, bad = _abi(C, z.to(DEV), y.to(DEV), zo.to(DEV), c_old, 10.0)
        assert bad == 2
        _check(l3, d, ref3, refd, f'odd {H}x{W}')
    # a misaligned view of an aligned size: same numbers as the aligned tensor, bit for bit (same arithmetic per pixel)
    z, zo, y = _case(21, 11, 2, 16, 16, 3.0, seed=9)
    zd, zod, yd = z.to(DEV), zo.to(DEV), y.to(DEV)
    l3, d, _ = _abi(C, zd, yd, zod, 11, 10.0)
    buf = torch.empty(zd.numel() + 1, device=DEV)
    zs = buf[1:].view_as(zd); zs.copy_(zd)
    assert zs.data_ptr() % 16 == 4
    l3s, ds, _ = _abi(C, zs, yd, zod, 11, 10.0)
    assert torch.equal(ds, d)
    assert max(abs(float(a) - float(b)) / max(1.0, abs(float(b))) for a, b in zip(l3s, l3)) < 1e-6      # another grid: other partial sums
    crit = C.UnbiasedDistillationCrossEntropy(11, 10.0)
    t = z[:, :, :7, :9].to(DEV).requires_grad_()
    loss = crit(t, y[:, :7, :9].to(DEV), zo[:, :, :7, :9].to(DEV)); loss.backward()
    ref3, refd = _reference(z[:, :, :7, :9], y[:, :7, :9], zo[:, :, :7, :9], 11, 10.0)
    _check(crit.parts, t.grad, ref3, refd, 'criterion on sliced views')


def test_benchmark_shape_is_deterministic(C):
    z, zo, y = _case(*CASES[4], 3.0, seed=2)
    zd, zod, yd = z.to(DEV), zo.to(DEV), y.to(DEV)
    l0, d0, _ = _abi(C, zd, yd, zod, 16, 10.0)
    for _ in range(4):
        l, d, _ = _abi(C, zd, yd, zod, 16, 10.0)
        assert torch.equal(l, l0) and torch.equal(d, d0)


def test_argument_errors(C):
    z, zo, y = _case(5, 2, 1, 4, 4, 1.0)
    zd, zod, yd = z.to(DEV), zo.to(DEV), y.to(DEV)
    with pytest.raises(RuntimeError, match='c_old'):
        _abi(C, zd, yd, zod, 6, 1.0)
    with pytest.raises(RuntimeError, match='c_old'):
        _abi(C, zd, yd, zod, 0, 1.0)
    with pytest.raises(RuntimeError, match='K_old_total'):
        _abi(C, zd, yd, zod[:, :1].contiguous(), 2, 1.0)
    with pytest.raises(RuntimeError, match='pitch'):
        _abi(C, zd, yd, zod, 2, 1.0, nhwc=torch.zeros(1, 4, 4, 16, device=DEV))
    lib, ptr = C._lib, C._lib.ptr
    wsb = lib.load().clamd_ce_workspace_bytes()
    ws, big = torch.zeros(wsb // 4, device=DEV), torch.zeros(1, 33, 4, 4, device=DEV)
    with pytest.raises(RuntimeError, match=r'\[1, 32\]'):
        lib.call('clamd_ce_unbiased_fwd_bwd', ptr(big), ptr(yd), None, 0, 2, 0.0, ptr(torch.empty_like(big)), None, 0, 0, ptr(torch.empty(3, device=DEV)),
                 ptr(ws), wsb, 1, 33, 4, 4, -100, 1.0, lib.stream_ptr())


# ---------------------------------------------------------------------------------------------------------------- growth on the device
def _batches(C, n, B=4, size=64, nc=21, lo=0, hi=11, first=0):
    return [(torch.from_numpy(C.synth.images(9, B, 3, size, size, first_image=(first + i) * B)).to(DEV),
             torch.from_numpy(C.synth.labels(9, B, size, size, nc, first_image=(first + i) * B, class_lo=lo, class_hi=hi)).to(DEV))
            for i in range(n)]


@pytest.mark.parametrize('ewc,l2', [(0.0, 0.0), (50.0, 0.01)])
def test_growth_on_the_device(C, ewc, l2):
    torch.manual_seed(5)
    task1, task2 = _batches(C, 2), _batches(C, 2, lo=11, hi=21)
    cfg = C.default_config(n_iters=100, lr=1e-3, num_classes=11, conv_dim=8, stats_every=1)
    tr = C.Trainer(task1, cfg)
    for x, y in task1:
        tr.train_step(x, y)
    m = tr.model
    m.eval()
    x = task1[0][0]
    with torch.no_grad():
        z0 = m(x).clone()
    pred0 = m.predict(x).clone()
    m.train()
    old_params = list(m.parameters())
    mom0 = [(tr.optim.state[p]['exp_avg'].clone(), tr.optim.state[p]['exp_avg_sq'].clone()) for p in old_params]
    step0 = float(tr.optim.state[old_params[0]]['step'])
    assert step0 == 2.0
    tr.begin_task2(c_old=11, distill_lambda=10.0, new_classes=10, unbiased=True, ewc_lambda=ewc, l2_lambda=l2)
    assert m.num_classes == 21 and cfg.num_classes == 21 and tr.old_model.num_classes == 11 and not m._engines
    assert isinstance(tr.distill, C.UnbiasedDistillationCrossEntropy)
    # (a) the softmax identity at fp32, and the arg-max up to the background fold
    m.eval()
    with torch.no_grad():
        z1 = m(x).clone()
    pred1 = m.predict(x)
    m.train()
    # (b) a new engine of the new width
    (eng,) = m._engines.values()
    assert eng.K == 21 and tuple(z1.shape) == (4, 21, 64, 64)
    p0, p1 = torch.softmax(z0.double(), 1), torch.softmax(z1.double(), 1)
    e_old = float((p1[:, 1:11] - p0[:, 1:]).abs().max())
    e_bg = float((p1[:, 0] + p1[:, 11:].sum(1) - p0[:, 0]).abs().max())
    assert e_old < 1e-6 and e_bg < 1e-6, (e_old, e_bg)
    fold = torch.where(pred1 >= 11, torch.zeros_like(pred1), pred1)
    settled = (p0.topk(2, 1).values[:, 0] - p0.topk(2, 1).values[:, 1]) > 1e-5        # ties of the background's share aside
    assert torch.equal(fold[settled & (pred0 > 0)], pred0[settled & (pred0 > 0)])
    # (c) Adam's moments
    new_params = list(m.parameters())
    assert len(new_params) == 82 and all(a is b for a, b in zip(new_params, tr.optim.param_groups[0]['params']))
    for i, (p, (m0, v0)) in enumerate(zip(new_params, mom0)):
        st = tr.optim.state[p]
        n0 = m0.shape[0]
        assert torch.equal(st['exp_avg'][:n0], m0) and torch.equal(st['exp_avg_sq'][:n0], v0), i
        assert float(st['exp_avg'][n0:].abs().sum()) == 0.0 and float(st['exp_avg_sq'][n0:].abs().sum()) == 0.0
        assert float(st['step']) == step0
    assert all(p not in tr.optim.state for p in old_params[-2:])
    # (d) the step runs with the regularisers; no importance on the new rows
    if ewc > 0:
        assert float(tr.consolidation.importance[-2][11:].abs().sum()) == 0.0 and float(tr.consolidation.importance[-1][11:].abs().sum()) == 0.0
        assert float(tr.consolidation.importance[-2][:11].abs().sum()) > 0.0
        assert torch.equal(tr.consolidation.anchor[-1][11:], new_params[-1].detach()[11:])
    w_new0 = new_params[-2].detach()[11:].clone()
    b_old0 = new_params[-1].detach()[:11].clone()
    for x2, y2 in task2:
        out, loss = tr.train_step(x2, y2)
        assert tuple(out.shape) == (4, 21, 64, 64) and bool(torch.isfinite(loss))
    # the re-homed state steps with the optimiser's hyper-parameters (their device copy is re-created with the moment buffers)
    assert [float(v) for v in tr.optim._hyper[:4]] == pytest.approx([1e-3, cfg.beta1, cfg.beta2, 1e-8], rel=1e-6)
    moved = (new_params[-1].detach()[:11] - b_old0).abs()
    # two Adam steps: |m^ / sqrt(v^)| <= (1 - beta1) / sqrt(1 - beta2) = 5 per step whatever the history; lr = 0 would leave the rows where they were
    assert 0.0 < float(moved.max()) <= 2 * 1e-3 * 5.0, float(moved.max())
    st = tr.optim.state[new_params[-2]]
    assert float(st['step']) == step0 + 2 and float(st['exp_avg'][11:].abs().sum()) > 0.0 and not torch.equal(new_params[-2].detach()[11:], w_new0)
    if ewc > 0:
        assert float(tr.optim.consolidation_penalty()) >= 0.0
    # (e) the grown checkpoint loads into stock torch and gives the same logits
    ref = TC.build_unet(21, 3, 8).to(DEV)
    ref.load_state_dict(m.state_dict(), strict=True)
    m.eval(); ref.eval()
    with torch.no_grad():
        r = rel_l2(m(x).cpu().numpy(), ref(x).cpu().numpy())
    assert r < 1e-4, r


def _torch_head_grow(ref, n):
    """The stock-torch counterpart of UNet.expand_classes(n, 'background')."""
    old = ref.last[6]
    K = old.out_channels
    new = nn.Conv2d(old.in_channels, K + n, 1, 1).to(old.weight.device)
    with torch.no_grad():
        new.weight[:K] = old.weight; new.bias[:K] = old.bias
        new.weight[K:] = old.weight[:1]
        b0 = old.bias[0] - float(np.log(n + 1))
        new.bias[0] = b0; new.bias[K:] = b0
    ref.last[6] = new
    return old, new


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3'])
def test_incremental_run_vs_stock_torch(C, dtype):
    """Task 1 with 11 outputs, begin_task2(c_old=11, new_classes=10, unbiased=True, distill_lambda=10), task 2, against the same procedure
    composed from stock torch ops (fp32 restatement of the two terms, torch.optim.Adam with the moments carried over by hand)."""
    import copy
    lr, c_old, lam, B, size, n1, n2 = 1e-3, 11, 10.0, 4, 64, 6, 6
    task1, task2 = _batches(C, n1), _batches(C, n2, lo=11, hi=21)
    torch.manual_seed(5)
    ref = TC.build_unet(11, 3, 8).to(DEV)
    cfg = C.default_config(n_iters=100, lr=lr, num_classes=11, conv_dim=8, compute_dtype=dtype, stats_every=1)
    tol = 2e-3 if dtype == 'fp32' else 5e-2

    def run(unbiased):
        tr = C.Trainer(task1, copy.copy(cfg))
        tr.model.load_state_dict(ref_state)
        l1 = [float(tr.train_step(x, y)[1].detach()) for x, y in task1]
        if unbiased:
            tr.begin_task2(c_old=c_old, distill_lambda=lam, new_classes=10, unbiased=True)
        else:
            tr.begin_task2(c_old=c_old, distill_lambda=lam, temperature=1.0, new_classes=10, unbiased=False)
        return tr, l1

    ref_state = {k: v.clone() for k, v in ref.state_dict().items()}
    tr, losses1 = run(True)
    # ---- the torch composition
    opt = torch.optim.Adam(ref.parameters(), lr=lr, betas=(cfg.beta1, cfg.beta2))
    ref.train()
    want1 = []
    for x, y in task1:
        opt.zero_grad(); l = nn.functional.cross_entropy(ref(x), y); l.backward(); opt.step(); want1.append(float(l))
    assert losses1 == pytest.approx(want1, rel=tol)
    old = copy.deepcopy(ref).eval()
    ow, nw = _torch_head_grow(ref, 10)
    opt2 = torch.optim.Adam(ref.parameters(), lr=lr, betas=(cfg.beta1, cfg.beta2))
    for p_old, p_new in zip(opt.param_groups[0]['params'], opt2.param_groups[0]['params']):
        st = opt.state[p_old]
        grown = {k: torch.zeros_like(p_new) for k in ('exp_avg', 'exp_avg_sq')}
        for k in grown:
            grown[k][:p_old.shape[0]] = st[k]
        opt2.state[p_new] = {'step': st['step'].clone(), **grown}
    names = [n for n, _ in tr.model.named_parameters()]
    for i, (x, y) in enumerate(task2):
        with torch.no_grad():
            zo = old(x)
        opt2.zero_grad()
        tot, ce, kd = unbiased_losses(ref(x), y, zo, c_old, lam)
        tot.backward()
        if i == 0 and dtype == 'fp32':
            # the gradient check of the first task-2 step, at IDENTICAL weights (the two runs' weights already differ by six Adam steps'
            # rounding, which this network's deep layers amplify: DESIGN section 2, conditioning across steps): a stock-torch probe holding
            # this path's own weights and old model
            probe, probe_old = TC.build_unet(21, 3, 8).to(DEV), TC.build_unet(11, 3, 8).to(DEV)
            probe.load_state_dict(tr.model.state_dict()); probe_old.load_state_dict(tr.old_model.state_dict())
            probe.train(); probe_old.eval()
            with torch.no_grad():
                pzo = probe_old(x)
            unbiased_losses(probe(x), y, pzo, c_old, lam)[0].backward()
        out, loss = tr.train_step(x, y)
        got = [float(v) for v in tr.distill.parts]
        print(f'incremental {dtype} step {i}: ours {got} torch {[float(tot), float(ce), float(kd)]}')
        assert float(loss.detach()) == got[0]
        assert got == pytest.approx([float(tot), float(ce), float(kd)], rel=tol, abs=tol * 1e-2), i
        if i == 0 and dtype == 'fp32':
            rels = {}
            for n_, p, q in zip(names, tr.model.parameters(), probe.parameters()):
                if float(q.grad.norm()) > 1e-6:          # conv biases in front of a train-mode BatchNorm have ~0 gradient (as test_unet_gpu.py)
                    rels[n_] = rel_l2(p.grad.cpu().numpy(), q.grad.cpu().numpy())
            print('incremental fp32: first task-2 step, gradient rel_l2 per tensor:', {k: f'{v:.2e}' for k, v in rels.items()})
            # what the norm filter left out: conv biases in front of a train-mode BatchNorm and nothing else
            bn_fed = {f'{st["name"]}{".block" if st["wrapped"] else ""}.{ci}.bias' for st in tr.model._table for ci, _, _, _ in st['convs']}
            skipped = set(names) - set(rels)
            assert skipped <= bn_fed, sorted(skipped - bn_fed)
            assert max(rels.values()) < 2e-3, max(rels.items(), key=lambda kv: kv[1])
        opt2.step()
    # ---- the point of the feature, as a property: task-1 mIoU is not lower than with the biased loss on the same seeds
    def miou(t, data):
        t.model.eval()
        conf = None
        with torch.no_grad():
            for x, y in data:
                c, _ = C.metrics.argmax_confusion(t.model(x), y, 21)
                conf = c if conf is None else conf + c
        return float(C.metrics.metrics_from_confusion(conf)[2])

    tb, _ = run(False)
    for x, y in task2:
        tb.train_step(x, y)
    a, b = miou(tr, task1), miou(tb, task1)
    print(f'incremental {dtype}: task-1 mIoU after task 2: unbiased {a:.4f}, plain CE + KD {b:.4f}; task-2 mIoU {miou(tr, task2):.4f} / {miou(tb, task2):.4f}')
    assert a >= b - 0.02, (a, b)


# ------------------------------------------------------------------------------------------------------- two ranks through growth
DDP = dict(k1=5, n_new=3, conv_dim=8, size=64, batch=2, steps=3)


def _ddp_incremental(ddp, head_init, rank=0):
    """Task 1, begin_task2 with head growth (unbiased criterion, consolidation and L2 term on), task 2, on ONE shard; under ddp through
    ddp.GradSync.  -> (losses of both tasks, final flat weights, summed gradient of the first task-2 step)."""
    import continual_learning_amd as C
    dev = torch.device('cuda', 0)
    k1, kn, b, s = DDP['k1'], DDP['k1'] + DDP['n_new'], DDP['batch'], DDP['size']
    mk = lambda lo, hi, first: [(torch.from_numpy(C.synth.images(99, b, 3, s, s, first_image=(first + i) * b)).to(dev),
                                 torch.from_numpy(C.synth.labels(99, b, s, s, kn, first_image=(first + i) * b, class_lo=lo, class_hi=hi)).to(dev))
                                for i in range(DDP['steps'])]
    task1, task2 = mk(0, k1, 0), mk(k1, kn, 10)
    torch.manual_seed(7)
    tr = C.Trainer(task1, C.default_config(n_iters=100, lr=1e-3, num_classes=k1, conv_dim=DDP['conv_dim'], stats_every=1))
    if ddp:
        C.ddp.broadcast_parameters(tr.model)
        C.ddp.GradSync(tr.model, tr.optim, min_bucket_bytes=16 << 10, grad_dtype='fp32')
    losses = [float(tr.train_step(x, y)[1].detach()) for x, y in task1]
    torch.manual_seed(100 + rank)          # ranks differ in RNG state: with head_init='default' only grow_head's broadcast keeps them equal
    tr.begin_task2(c_old=k1, distill_lambda=10.0, new_classes=DDP['n_new'], unbiased=True, head_init=head_init, ewc_lambda=50.0, l2_lambda=0.01)
    grad0 = None
    for x, y in task2:
        losses.append(float(tr.train_step(x, y)[1].detach()))
        if grad0 is None:
            grad0 = torch.cat([p.grad.reshape(-1) for p in tr.model.parameters()]).cpu()
    torch.cuda.synchronize()
    assert tr.model.num_classes == kn
    return losses, torch.cat([p.detach().reshape(-1) for p in tr.model.parameters()]).cpu(), grad0


def _ddp_worker(rank, world, port, head_init, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        losses, flat, grad0 = _ddp_incremental(True, head_init, rank)
        q.put((rank, losses, flat.numpy(), grad0.numpy()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('head_init', ['background', 'default'])
def test_ddp_identical_shards_through_growth_reproduce_single_process(head_init):
    """Two gloo ranks on the one card, identical shards (the pattern of test_ddp_gpu.py): the summed gradient is exactly twice the local
    one and (g + g) * 0.5 == g, so the run through head growth must reproduce the single-process run bit for bit -- losses of both tasks,
    the first task-2 step's gradient, the final weights.  The single process draws 'default' rows with rank 0's RNG state."""
    ref_losses, ref_flat, ref_grad = _ddp_incremental(False, head_init)
    world = 2
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    ps = [ctx.Process(target=_ddp_worker, args=(r, world, port, head_init, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = sorted((q.get(timeout=300) for _ in range(world)), key=lambda r: r[0])
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    for rank, losses, flat, grad0 in res:
        g = torch.from_numpy(grad0)
        assert torch.equal(g, 2 * ref_grad), f'rank {rank}: summed gradient of the first task-2 step is not exactly 2x the local one ' \
                                             f'(rel {float((g - 2 * ref_grad).norm() / (2 * ref_grad).norm()):.2e})'
        assert losses == ref_losses, f'rank {rank}: {losses} vs {ref_losses}'
        assert torch.equal(torch.from_numpy(flat), ref_flat), f'rank {rank}: weights after task 2 differ'
