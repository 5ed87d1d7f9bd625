"""GPU: pseudo-labelling of the old classes in the task step (build-defined: the reference has no continual-learning code, parity unpinned).

clamd_pseudo_entropy_hist, clamd_pseudo_label and clamd_ce_fwd_bwd_weighted against the restatement of tests/test_pseudo_label_cpu.py
(pinned there).  The histogram and the relabelling are compared EXACTLY: the inputs keep every candidate pixel at least 2e-5 away from a
bin edge (masked_case), where the step functions of a float32 and a float64 evaluation agree.  Then PseudoLabeler / CrossEntropyLoss /
Trainer.begin_task2(pseudo_label=True) against the same step composed from stock torch ops on the same device."""
import copy
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

from conftest import rel_l2
from oracle import torch_cpu as TC
from test_incremental_gpu import _batches, _check, _torch_head_grow
from test_pseudo_label_cpu import MASK_CAP, SHAPES, masked_case, pseudo_reference, weighted_ce

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
NB = 100
DT = [('fp32', 0), ('bf16', 1), ('bf16x3', 2)]
# (B, c_old, H, W, scale, K_old_total or None): the five shapes of the CPU file, H * W % 4 != 0, a wider old model, c_old == 1, 32 old classes
HIST_CASES = [s + (None,) for s in SHAPES] + [(2, 11, 7, 9, 3.0, None), (3, 11, 16, 16, 3.0, 14), (2, 1, 16, 16, 3.0, 4), (2, 32, 16, 24, 3.0, None)]


@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    C._lib.load()
    return C


def _hist(C, zo, y, c_old, hist=None, nb=NB):
    lib, ptr = C._lib, C._lib.ptr
    if hist is None:
        hist = torch.zeros(c_old, nb, dtype=torch.int64, device=DEV)
    B, Ko, H, W = zo.shape
    lib.call('clamd_pseudo_entropy_hist', ptr(zo), Ko, c_old, ptr(y), ptr(hist), nb, B, H, W, lib.stream_ptr())
    torch.cuda.synchronize()
    return hist


def _label(C, zo, y, c_old, tau, min_factor=0.0, want_nu=True, ign=-100):
    """-> (labels_out, counts [B, 2], nu or None); counts and nu start as garbage: the entry point owns them."""
    lib, ptr = C._lib, C._lib.ptr
    B, Ko, H, W = zo.shape
    out = torch.full_like(y, 77)
    counts = torch.full((B, 2), 12345, dtype=torch.int32, device=DEV)
    nu = torch.full((B,), float('nan'), device=DEV) if want_nu else None
    lib.call('clamd_pseudo_label', ptr(zo), Ko, c_old, ptr(y), ptr(tau), ptr(out), ptr(counts), ptr(nu), float(min_factor), B, H, W, ign,
             lib.stream_ptr())
    torch.cuda.synchronize()
    return out, counts, nu


def _loss(C, z, y, nu, nhwc=None, dcode=0):
    """clamd_ce_count + clamd_ce_fwd_bwd_weighted (nu a tensor) or clamd_ce_fwd_bwd_counted (nu None) -> (loss3, d logits, bad labels)."""
    lib, ptr, s = C._lib, C._lib.ptr, C._lib.stream_ptr()
    L = lib.load()
    B, K, H, W = z.shape
    wsb = L.clamd_ce_workspace_bytes()
    off = L.clamd_ce_bad_label_count_offset() // 4
    ws = torch.full((wsb // 4,), float('nan'), device=DEV)
    d, l3 = torch.full_like(z, float('nan')), torch.empty(3, device=DEV)
    ldc = 0 if nhwc is None else nhwc.shape[-1]
    lib.call('clamd_ce_count', ptr(y), B, K, H, W, -100, ptr(ws), wsb, s)
    if nu is None:
        lib.call('clamd_ce_fwd_bwd_counted', ptr(z), ptr(y), ptr(d), ptr(nhwc), ldc, dcode, ptr(l3), ptr(ws), wsb, B, K, H, W, -100, 1.0, s)
    else:
        lib.call('clamd_ce_fwd_bwd_weighted', ptr(z), ptr(y), ptr(nu), ptr(d), ptr(nhwc), ldc, dcode, ptr(l3), ptr(ws), wsb, B, K, H, W, -100, 1.0, s)
    torch.cuda.synchronize()
    return l3, d, int(ws[off:off + 1].view(torch.int32))


def _inputs(B, c_old, H, W, scale, kt, seed=None):
    zo, y, share = masked_case(B, c_old, H, W, scale, seed=c_old + H if seed is None else seed, k_total=kt)
    assert share <= MASK_CAP, share
    if B > 1:
        y[-1][y[-1] == 0] = 1          # the last image has no candidate: nu = 1
    return zo, y


# ------------------------------------------------------------------------------------------------------------ histogram and relabelling
@pytest.mark.parametrize('B,c_old,H,W,scale,kt', HIST_CASES)
def test_histogram_and_relabelling_are_exact(C, B, c_old, H, W, scale, kt):
    zo, y = _inputs(B, c_old, H, W, scale, kt)
    ref = pseudo_reference(zo, y, c_old, NB, torch.float64)
    zod, yd = zo.to(DEV), y.to(DEV)
    y_before = yd.clone()
    hist = _hist(C, zod, yd, c_old)
    nd = int((hist.cpu() != ref['hist']).sum())
    print(f'hist B{B} c{c_old} {H}x{W}: {int(ref["hist"].sum())} candidates, {nd} bins differ')
    assert nd == 0
    assert torch.equal(_hist(C, zod, yd, c_old, hist).cpu(), 2 * ref['hist']), 'a second call must add to what is there'
    tau = C.thresholds_from_histogram(ref['hist'], NB)
    for mf in (0.0, 0.3):
        want = pseudo_reference(zo, y, c_old, NB, torch.float64, thresholds=tau, min_factor=mf)
        out, counts, nu = _label(C, zod, yd, c_old, tau.to(DEV), mf)
        nl = int((out.cpu() != want['labels_out']).sum())
        print(f'label B{B} c{c_old} {H}x{W} min_factor {mf}: {nl} labels differ, counts {counts.tolist()[:3]}, nu {nu.tolist()[:3]}')
        assert nl == 0
        assert torch.equal(counts.cpu().long(), want['counts'])
        assert torch.equal(nu.cpu(), want['nu']), (nu.tolist(), want['nu'].tolist())
        if B > 1:
            assert counts[-1].tolist() == [0, 0] and float(nu[-1]) == 1.0
        assert float(nu.min()) >= mf
    # pass-through of everything that is not a candidate (new classes, ignore_index, out-of-range values); labels_in untouched
    keep = y != 0
    assert torch.equal(out.cpu()[keep], y[keep]) and int((y == -100).sum()) >= 1 and int(((y < 0) & (y != -100)).sum()) + int((y > 31).sum()) >= 1
    assert torch.equal(yd, y_before)
    # image_weight NULL: labels and counts alone
    out2, counts2, _ = _label(C, zod, yd, c_old, tau.to(DEV), 0.3, want_nu=False)
    assert torch.equal(out2, out) and torch.equal(counts2, counts)


def test_misaligned_tensors_take_the_one_pixel_variant(C):
    B, c_old, H, W = 2, 11, 16, 16
    zo, y = _inputs(B, c_old, H, W, 3.0, None, seed=21)
    ref = pseudo_reference(zo, y, c_old, NB, torch.float64)
    tau = C.thresholds_from_histogram(ref['hist'], NB)
    want = pseudo_reference(zo, y, c_old, NB, torch.float64, thresholds=tau)
    buf = torch.empty(zo.numel() + 1, device=DEV)
    zs = buf[1:].view_as(zo); zs.copy_(zo)
    lbuf = torch.empty(y.numel() + 1, dtype=torch.int64, device=DEV)
    ys = lbuf[1:].view_as(y); ys.copy_(y)
    assert zs.data_ptr() % 16 == 4 and ys.data_ptr() % 32 == 8
    for zz, yy in ((zs, y.to(DEV)), (zo.to(DEV), ys), (zs, ys)):
        assert torch.equal(_hist(C, zz, yy, c_old).cpu(), ref['hist'])
        out, counts, nu = _label(C, zz, yy, c_old, tau.to(DEV))
        assert torch.equal(out.cpu(), want['labels_out']) and torch.equal(counts.cpu().long(), want['counts']) and torch.equal(nu.cpu(), want['nu'])


def test_equal_maxima_give_the_lowest_index(C):
    """Old logits drawn from three values: most pixels have several equal maxima.  Every threshold 2 accepts every candidate (u <= 1), so
    labels_out IS c*; the histogram's row sums count the candidates per c* whatever their bins."""
    g = torch.Generator().manual_seed(3)
    for B, c_old, H, W in ((2, 11, 16, 16), (1, 5, 7, 9), (2, 32, 8, 8)):
        zo = torch.randint(0, 3, (B, c_old, H, W), generator=g).float()
        zo[0, :, 0, 0] = 1.0                                          # all equal: class 0
        zo[0, :, 0, 1] = 0.0; zo[0, c_old - 2:, 0, 1] = 5.0           # the last two tie
        y = torch.zeros(B, H, W, dtype=torch.int64)
        first = zo.argmax(1)
        assert int((zo == zo.max(1, keepdim=True).values).sum(1).max()) > 1
        assert int(first[0, 0, 0]) == 0 and int(first[0, 0, 1]) == c_old - 2
        out, counts, _ = _label(C, zo.to(DEV), y.to(DEV), c_old, torch.full((c_old,), 2.0, device=DEV))
        assert torch.equal(out.cpu(), first)
        assert counts.tolist() == [[H * W, H * W]] * B
        hist = _hist(C, zo.to(DEV), y.to(DEV), c_old)
        assert torch.equal(hist.sum(1).cpu(), torch.bincount(first.reshape(-1), minlength=c_old))


def test_pass_argument_errors(C):
    zo, y = torch.zeros(1, 4, 4, 4, device=DEV), torch.zeros(1, 4, 4, dtype=torch.int64, device=DEV)
    tau = torch.zeros(33, device=DEV)
    with pytest.raises(RuntimeError, match='K_old_total'):
        _hist(C, zo, y, 5)
    with pytest.raises(RuntimeError, match=r'\[1, 32\]'):
        _label(C, torch.zeros(1, 40, 4, 4, device=DEV), y, 33, tau)
    with pytest.raises(RuntimeError, match='8192'):
        _hist(C, zo, y, 4, nb=4096)
    with pytest.raises(RuntimeError, match='image_weight'):          # required: the unweighted loss is clamd_ce_fwd_bwd_counted
        C._lib.call('clamd_ce_fwd_bwd_weighted', zo.data_ptr(), y.data_ptr(), None, zo.data_ptr(), None, 0, 0, zo.data_ptr(), zo.data_ptr(), 0,
                    1, 4, 4, 4, -100, 1.0, C._lib.stream_ptr())


# ------------------------------------------------------------------------------------------------------------------- the weighted loss
def _loss_case(K, B, H, W, scale, seed=0):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, K, H, W, generator=g) * scale
    y = torch.randint(0, K, (B, H, W), generator=g)
    y[0, 0, :3] = -100; y[0, 1, 0] = K + 2; y[-1, -1, -1] = -7
    nu = torch.rand(B, generator=g)
    if B > 1:
        nu[0] = 1.0
    if B > 2:
        nu[1] = 0.0
    return z, y, nu


def _loss_reference(z, y, nu):
    zz = z.double().to(DEV).requires_grad_()
    loss = weighted_ce(zz, y.to(DEV), nu.to(DEV))
    g, = torch.autograd.grad(loss, zz)
    return [float(loss), float(loss), 0.0], g


@pytest.mark.parametrize('K,B,H,W', [(21, 2, 16, 16), (5, 3, 8, 12), (32, 1, 8, 8), (11, 4, 7, 9), (21, 16, 256, 256)])
@pytest.mark.parametrize('scale', [3.0, 30.0])
def test_weighted_loss_vs_restatement(C, K, B, H, W, scale):
    z, y, nu = _loss_case(K, B, H, W, scale, seed=K)
    ref3, refd = _loss_reference(z, y, nu)
    l3, d, bad = _loss(C, z.to(DEV), y.to(DEV), nu.to(DEV))
    assert bad == 2 and float(l3[2]) == 0.0 and float(l3[0]) == float(l3[1])
    _check(l3, d, ref3, refd, f'weighted abi K{K} {H}x{W} x{scale}')
    crit = C.CrossEntropyLoss()
    t = z.to(DEV).requires_grad_()
    loss = crit(t, y.to(DEV), nu.to(DEV)); loss.backward(); torch.cuda.synchronize()
    assert int(crit.bad_labels) == 2
    _check([loss.detach()] * 2 + [0.0], t.grad, ref3, refd, f'weighted criterion K{K} {H}x{W} x{scale}')


@pytest.mark.parametrize('name,dcode', DT)
@pytest.mark.parametrize('K,B,H,W', [(21, 16, 256, 256), (5, 2, 8, 12), (32, 1, 4, 4), (11, 3, 16, 20)])
def test_unit_weights_are_the_plain_loss_bit_for_bit(C, name, dcode, K, B, H, W):
    one = torch.ones(B, device=DEV)
    for scale in (4.0, 40.0):
        z, y, _ = _loss_case(K, B, H, W, scale, seed=K + 1)
        zd, yd = z.to(DEV), y.to(DEV)
        l0, d0, bad0 = _loss(C, zd, yd, None)
        l1, d1, bad1 = _loss(C, zd, yd, one)
        ndiff = int((d0.view(torch.int32) != d1.view(torch.int32)).sum())
        assert ndiff == 0 and torch.equal(l0, l1) and bad0 == bad1 == 2, (K, scale, ndiff, l0.tolist(), l1.tolist())
        nh0 = torch.full((B, H, W, 32), 5.0, dtype=C.ops.TORCH_DT[dcode], device=DEV)
        nh1 = torch.full((B, H, W, 32), 7.0, dtype=C.ops.TORCH_DT[dcode], device=DEV)
        l0n, d0n, _ = _loss(C, zd, yd, None, nhwc=nh0, dcode=dcode)
        l1n, d1n, _ = _loss(C, zd, yd, one, nhwc=nh1, dcode=dcode)
        assert torch.equal(d0n, d0) and torch.equal(d1n, d0) and torch.equal(l0n, l0) and torch.equal(l1n, l0)
        w = torch.int16 if dcode == 1 else torch.int32
        nbad = int((nh0.view(w) != nh1.view(w)).sum())
        assert nbad == 0, (name, K, scale, nbad)


@pytest.mark.parametrize('name,dcode', DT)
def test_weighted_nhwc_copy_is_the_converted_gradient(C, name, dcode):
    for K, B, H, W in ((21, 2, 16, 16), (5, 3, 8, 12), (11, 2, 7, 9)):          # the last: the one-pixel variant
        z, y, nu = _loss_case(K, B, H, W, 4.0, seed=3)
        nh = torch.full((B, H, W, 32), 5.0, dtype=C.ops.TORCH_DT[dcode], device=DEV)
        l3, d, _ = _loss(C, z.to(DEV), y.to(DEV), nu.to(DEV), nhwc=nh, dcode=dcode)
        l3b, db, _ = _loss(C, z.to(DEV), y.to(DEV), nu.to(DEV))
        assert torch.equal(d, db) and torch.equal(l3, l3b)
        conv = C.ops.to_nhwc(d, dcode, cp=32)
        w = torch.int16 if dcode == 1 else torch.int32
        nbad = int((conv.view(w) != nh.view(w)).sum())
        assert nbad == 0, (name, K, H, W, nbad)


def test_weighted_all_pixels_ignored(C):
    z, y, nu = _loss_case(21, 2, 16, 16, 50.0)
    y[:] = -100
    for zz in (z, z[:, :, :7, :9].contiguous()):
        yy = y[:, :zz.shape[2], :zz.shape[3]].contiguous()
        l3, d, bad = _loss(C, zz.to(DEV), yy.to(DEV), nu.to(DEV))
        assert bad == 0 and [float(v) for v in l3] == [0.0, 0.0, 0.0] and float(d.abs().max()) == 0.0 and bool(torch.isfinite(d).all())


def test_one_pixel_variant_equals_the_four_pixel_variant(C):
    """A misaligned view of an aligned size: the same arithmetic per pixel, so d logits is bit-equal; the loss is added over another grid
    (other partial sums): equal to fp32 summation accuracy."""
    z, y, nu = _loss_case(21, 3, 16, 16, 3.0, seed=9)
    zd, yd, nud = z.to(DEV), y.to(DEV), nu.to(DEV)
    l3, d, _ = _loss(C, zd, yd, nud)
    buf = torch.empty(zd.numel() + 1, device=DEV)
    zs = buf[1:].view_as(zd); zs.copy_(zd)
    assert zs.data_ptr() % 16 == 4
    l3s, ds, _ = _loss(C, zs, yd, nud)
    assert torch.equal(ds, d)
    assert max(abs(float(a) - float(b)) / max(1.0, abs(float(b))) for a, b in zip(l3s, l3)) < 1e-6


def test_through_the_unet_with_hand_over_and_scaled_backward(C):
    for name in ('fp32', 'bf16'):
        torch.manual_seed(0)
        m = C.UNet(21, 3, 8, compute_dtype=name).to(DEV)
        x = torch.randn(2, 3, 32, 32, device=DEV)
        yy = torch.randint(0, 21, (2, 32, 32), device=DEV)
        nu = torch.tensor([0.25, 0.75], device=DEV)
        crit = C.CrossEntropyLoss()
        grads = []
        for f in (1.0, 0.5):
            out = m(x); m.zero_grad(); (crit(out, yy, nu) * f).backward(); torch.cuda.synchronize()
            grads.append(torch.cat([p.grad.reshape(-1) for p in m.parameters()]).clone())
        C.loss.HANDOVER, keep = False, C.loss.HANDOVER
        try:
            out = m(x); m.zero_grad(); crit(out, yy, nu).backward(); torch.cuda.synchronize()
        finally:
            C.loss.HANDOVER = keep
        plain = torch.cat([p.grad.reshape(-1) for p in m.parameters()])
        assert torch.equal(grads[0], plain), 'the handed-over NHWC copy and the converted NCHW gradient give different parameter gradients'
        r = float((grads[1] - 0.5 * grads[0]).norm() / (0.5 * grads[0]).norm())
        assert r < (1e-6 if name == 'fp32' else 2e-2), r
        # unit weights through the module: the plain criterion's gradients, bit for bit
        out = m(x); m.zero_grad(); crit(out, yy, torch.ones(2, device=DEV)).backward()
        a = torch.cat([p.grad.reshape(-1) for p in m.parameters()]).clone()
        out = m(x); m.zero_grad(); crit(out, yy).backward()
        assert torch.equal(a, torch.cat([p.grad.reshape(-1) for p in m.parameters()]))


# ------------------------------------------------------------------------------------------------------------------------- determinism
def test_benchmark_shape_is_deterministic(C):
    zo, y = _inputs(16, 11, 256, 256, 3.0, None)
    zod, yd = zo.to(DEV), y.to(DEV)
    tau = C.thresholds_from_histogram(_hist(C, zod, yd, 11).cpu(), NB).to(DEV)
    z, y2, nu = _loss_case(21, 16, 256, 256, 3.0, seed=2)
    zd, y2d, nud = z.to(DEV), y2.to(DEV), nu.to(DEV)
    runs = []
    for _ in range(2):
        h = _hist(C, zod, yd, 11)
        out, counts, w = _label(C, zod, yd, 11, tau, 0.3)
        l3, d, _ = _loss(C, zd, y2d, nud)
        runs.append((h, out, counts, w, l3, d))
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


# ------------------------------------------------------------------------------------------------------------------------- the labeller
def test_pseudo_labeler_module(C):
    zo, y = _inputs(4, 11, 64, 64, 3.0, 13)
    zod, yd = zo.to(DEV), y.to(DEV)
    lab = C.PseudoLabeler(11, bins=NB, adaptive=True, min_factor=0.3)
    with pytest.raises(RuntimeError, match='thresholds'):
        lab(zod, yd)
    lab.accumulate(zod[:2], yd[:2]).accumulate(zod[2:], yd[2:]).finish()
    ref = pseudo_reference(zo, y, 11, NB, torch.float64)
    assert torch.equal(lab.hist.cpu(), ref['hist']) and lab.thresholds.is_cuda and lab.thresholds.dtype == torch.float32
    tau = C.thresholds_from_histogram(ref['hist'], NB)
    assert torch.equal(lab.thresholds.cpu(), tau)
    want = pseudo_reference(zo, y, 11, NB, torch.float64, thresholds=tau, min_factor=0.3)
    out, nu = lab(zod, yd)
    assert torch.equal(out.cpu(), want['labels_out']) and torch.equal(nu.cpu(), want['nu']) and torch.equal(lab.counts.cpu().long(), want['counts'])
    fixed = C.PseudoLabeler(11, adaptive=False, thresholds=tau)
    out2, none = fixed(zod, yd)
    assert none is None and torch.equal(out2, out)
    # calibrate(): a stand-in old model whose forward returns the stored logits
    class Old(nn.Module):
        def forward(self, x):
            return zod[int(x[0, 0, 0, 0]):int(x[0, 0, 0, 0]) + 2]
    loader = [(torch.full((2, 1, 1, 1), float(i)), y[i:i + 2]) for i in (0, 2)]
    cal = C.PseudoLabeler(11, bins=NB).calibrate(Old(), loader, DEV)
    assert torch.equal(cal.hist, lab.hist) and torch.equal(cal.thresholds, lab.thresholds)
    half = C.PseudoLabeler(11, bins=NB).calibrate(Old(), loader, DEV, max_batches=1)
    assert int(half.hist.sum()) == int((y[:2] == 0).sum())


# ------------------------------------------------------------------------------------------------------------------- trainer, end to end
def _miou(C, t, data):
    modes = [(mod, mod.training) for mod in t.model.modules()]
    t.model.eval()
    conf = None
    with torch.no_grad():
        for x, y in data:
            c, _ = C.metrics.argmax_confusion(t.model(x), y, 21)
            conf = c if conf is None else conf + c
    for mod, mode in modes:
        mod.training = mode
    return float(C.metrics.metrics_from_confusion(conf)[2])


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3'])
def test_pseudo_label_run_vs_stock_torch(C, dtype):
    """Task 1 with 11 outputs, begin_task2(c_old=11, distill_lambda=0, new_classes=10, pseudo_label=True, pseudo_adaptive=True), task 2,
    against the same procedure composed from stock torch ops: the old model's logits, pseudo_reference with the trainer's thresholds, then
    weighted_ce; torch.optim.Adam with the moments carried over by hand (the procedure of test_incremental_run_vs_stock_torch).
    The stock-torch OLD model holds the trainer's snapshot: the labels are a step function of the old model's logits, and two snapshots that
    differ by six Adam steps' rounding (which this network amplifies) relabel about 1 % of the pixels differently -- that
    would compare two labelings, not two implementations of one.  What remains are the few near-threshold pixels that flip between the two
    forwards of the SAME old model (printed per step); the trained model is torch's own, stepped by torch.optim.Adam, as in that test."""
    lr, c_old, B, size, n1, n2 = 1e-3, 11, 4, 64, 6, 6
    task1, task2 = _batches(C, n1), _batches(C, n2, lo=11, hi=21)
    torch.manual_seed(5)
    ref = TC.build_unet(11, 3, 8).to(DEV)
    cfg = C.default_config(n_iters=100, lr=lr, num_classes=11, conv_dim=8, compute_dtype=dtype, stats_every=1)
    tol = 2e-3 if dtype == 'fp32' else 5e-2
    ref_state = {k: v.clone() for k, v in ref.state_dict().items()}

    def run(pseudo):
        tr = C.Trainer(task1, copy.copy(cfg))
        tr.model.load_state_dict(ref_state)
        l1 = [float(tr.train_step(x, y)[1].detach()) for x, y in task1]
        tr.train_data_loader = task2                       # the new task's loader: what the labeller calibrates on by default
        if pseudo:
            tr.begin_task2(c_old=c_old, distill_lambda=0, new_classes=10, pseudo_label=True, pseudo_adaptive=True)
        else:
            tr.begin_task2(c_old=c_old, distill_lambda=0, new_classes=10)
        return tr, l1

    tr, losses1 = run(True)
    assert tr.distill is None and tr.pseudo is not None and tr.pseudo.adaptive and tr.model.num_classes == 21
    tau = tr.pseudo.thresholds
    print(f'pseudo {dtype}: thresholds {[round(float(t), 2) for t in tau]}, calibrated on {int(tr.pseudo.hist.sum())} background pixels')
    assert int(tr.pseudo.hist.sum()) == sum(int((y == 0).sum()) for _, y in task2)
    # ---- the torch composition
    opt = torch.optim.Adam(ref.parameters(), lr=lr, betas=(cfg.beta1, cfg.beta2))
    ref.train()
    want1 = []
    for x, y in task1:
        opt.zero_grad(); l = nn.functional.cross_entropy(ref(x), y); l.backward(); opt.step(); want1.append(float(l))
    assert losses1 == pytest.approx(want1, rel=tol)
    own_old = copy.deepcopy(ref).eval()          # torch's independently trained snapshot: reported below, not asserted
    old = TC.build_unet(11, 3, 8).to(DEV)
    old.load_state_dict(tr.old_model.state_dict())
    old.eval()
    _torch_head_grow(ref, 10)
    opt2 = torch.optim.Adam(ref.parameters(), lr=lr, betas=(cfg.beta1, cfg.beta2))
    for p_old, p_new in zip(opt.param_groups[0]['params'], opt2.param_groups[0]['params']):
        st = opt.state[p_old]
        grown = {k: torch.zeros_like(p_new) for k in ('exp_avg', 'exp_avg_sq')}
        for k in grown:
            grown[k][:p_old.shape[0]] = st[k]
        opt2.state[p_new] = {'step': st['step'].clone(), **grown}
    names = [n for n, _ in tr.model.named_parameters()]
    for i, (x, y) in enumerate(task2):
        y_before = y.clone()
        with torch.no_grad():
            zo = old(x)
        opt2.zero_grad()
        pr = pseudo_reference(zo, y, c_old, NB, torch.float32, thresholds=tau)
        zr = ref(x)
        tot = weighted_ce(zr, pr['labels_out'], pr['nu'])
        tot.backward()
        with torch.no_grad():
            ours_labels, ours_nu = tr.pseudo(tr.old_model(x), y)          # what the step below will use (both passes are deterministic)
            # the named procedure's own old model (six separately rounded Adam steps away): how far its labelling is from the snapshot's
            po = pseudo_reference(own_old(x), y, c_old, NB, torch.float32, thresholds=tau)
            tot_own = float(weighted_ce(zr.detach(), po['labels_out'], po['nu']))
        print(f'pseudo {dtype} step {i}: with torch\'s independently trained old model {int((po["labels_out"] != ours_labels).sum())} of {y.numel()} labels '
              f'differ and the torch loss is {tot_own:.6f} (with the snapshot {float(tot):.6f}: {abs(tot_own - float(tot)) / float(tot):.2e} relative)')
        if i == 0 and dtype == 'fp32':
            # the gradient check of the first task-2 step at IDENTICAL weights, as in test_incremental_run_vs_stock_torch
            probe, probe_old = TC.build_unet(21, 3, 8).to(DEV), TC.build_unet(11, 3, 8).to(DEV)
            probe.load_state_dict(tr.model.state_dict()); probe_old.load_state_dict(tr.old_model.state_dict())
            probe.train(); probe_old.eval()
            with torch.no_grad():
                pzo = probe_old(x)
            pp = pseudo_reference(pzo, y, c_old, NB, torch.float32, thresholds=tau)
            weighted_ce(probe(x), pp['labels_out'], pp['nu']).backward()
            print(f'pseudo fp32: first task-2 step at identical weights: {int((pp["labels_out"] != ours_labels).sum())} of {y.numel()} labels differ '
                  f'between the two old-model forwards; nu ours {ours_nu.tolist()} torch {pp["nu"].tolist()}')
        out, loss = tr.train_step(x, y)
        assert torch.equal(y, y_before), 'train_step must not modify the labels it is given'
        got = float(loss.detach())
        print(f'pseudo {dtype} step {i}: ours {got:.6f} torch {float(tot):.6f}; {int((pr["labels_out"] != ours_labels).sum())} of {y.numel()} labels differ, '
              f'accepted {tr.pseudo.counts[:, 1].tolist()} of {tr.pseudo.counts[:, 0].tolist()}')
        assert int(tr.c_loss.bad_labels) == 0
        assert got == pytest.approx(float(tot), rel=tol, abs=tol * 1e-2), i
        if i == 0 and dtype == 'fp32':
            rels = {}
            for n_, p, q in zip(names, tr.model.parameters(), probe.parameters()):
                if float(q.grad.norm()) > 1e-6:          # conv biases in front of a train-mode BatchNorm have ~0 gradient (as test_unet_gpu.py)
                    rels[n_] = rel_l2(p.grad.cpu().numpy(), q.grad.cpu().numpy())
            print('pseudo fp32: first task-2 step, gradient rel_l2 per tensor:', {k: f'{v:.2e}' for k, v in rels.items()})
            bn_fed = {f'{st["name"]}{".block" if st["wrapped"] else ""}.{ci}.bias' for st in tr.model._table for ci, _, _, _ in st['convs']}
            skipped = set(names) - set(rels)
            assert skipped <= bn_fed, sorted(skipped - bn_fed)
            assert max(rels.values()) < 2e-3, max(rels.items(), key=lambda kv: kv[1])
        opt2.step()
    # ---- forgetting, reported (six steps on synthetic data do not pin the effect): against plain fine-tuning on the same seeds
    tb, _ = run(False)
    assert tb.pseudo is None and tb.distill is None
    for x, y in task2:
        tb.train_step(x, y)
    print(f'pseudo {dtype}: after task 2, task-1 mIoU pseudo-labels {_miou(C, tr, task1):.4f} / plain fine-tuning {_miou(C, tb, task1):.4f}; '
          f'task-2 mIoU {_miou(C, tr, task2):.4f} / {_miou(C, tb, task2):.4f}')


def test_pseudo_labels_with_the_other_regularisers(C):
    task1, task2 = _batches(C, 3), _batches(C, 3, lo=11, hi=21)
    torch.manual_seed(5)
    cfg = C.default_config(n_iters=100, lr=1e-3, num_classes=11, conv_dim=8, stats_every=1)
    tr = C.Trainer(task1, cfg)
    for x, y in task1:
        tr.train_step(x, y)
    tr.begin_task2(c_old=11, distill_lambda=1.0, l2_lambda=0.01, ewc_lambda=50.0, new_classes=10, freeze_bn=True,
                   pseudo_label=True, pseudo_adaptive=False, pseudo_bins=50, pseudo_loader=task2)
    assert isinstance(tr.distill, C.DistillationCrossEntropy) and tr.pseudo.bins == 50 and not tr.pseudo.adaptive
    for x, y in task2:
        out, loss = tr.train_step(x, y)
        assert bool(torch.isfinite(loss)) and int(tr.distill.bad_labels) == 0 and tuple(out.shape) == (4, 21, 64, 64)
        assert int(tr.pseudo.counts[:, 1].sum()) > 0, 'no background pixel was relabelled'
    # the statistics of train_epoch use the ORIGINAL labels: an epoch runs, and the loader's labels are what they were
    before = [y.clone() for _, y in task2]
    tr.train_data_loader = task2
    stats = tr.train_epoch(0)
    assert all(torch.equal(a, y) for a, (_, y) in zip(before, task2)) and stats['mean_iu'] == stats['mean_iu'] and stats['loss'] == stats['loss']
    # a later plain begin_task2 switches the labeller off again
    tr.begin_task2(c_old=21, distill_lambda=0.0)
    assert tr.pseudo is None


# --------------------------------------------------------------------------------------------------------------------------- two ranks
def _ddp_thresholds(ddp):
    import continual_learning_amd as C
    dev = torch.device('cuda', 0)
    mk = lambda lo, hi, first: [(torch.from_numpy(C.synth.images(99, 2, 3, 64, 64, first_image=(first + i) * 2)).to(dev),
                                 torch.from_numpy(C.synth.labels(99, 2, 64, 64, 8, first_image=(first + i) * 2, class_lo=lo, class_hi=hi)).to(dev))
                                for i in range(2)]
    task1, task2 = mk(0, 5, 0), mk(5, 8, 10)
    torch.manual_seed(7)
    tr = C.Trainer(task1, C.default_config(n_iters=100, lr=1e-3, num_classes=5, conv_dim=8, stats_every=1))
    if ddp:
        C.ddp.broadcast_parameters(tr.model)
        C.ddp.GradSync(tr.model, tr.optim, min_bucket_bytes=16 << 10, grad_dtype='fp32')
    for x, y in task1:
        tr.train_step(x, y)
    tr.begin_task2(c_old=5, distill_lambda=0, new_classes=3, pseudo_label=True, pseudo_adaptive=True, pseudo_loader=task2)
    losses = [float(tr.train_step(x, y)[1].detach()) for x, y in task2]
    torch.cuda.synchronize()
    return tr.pseudo.thresholds.cpu(), tr.pseudo.hist_total.cpu(), losses


def _ddp_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        tau, hist, losses = _ddp_thresholds(True)
        q.put((rank, tau.numpy(), hist.numpy(), losses))
    finally:
        dist.destroy_process_group()


def test_ddp_identical_shards_give_the_single_process_thresholds():
    """Two gloo ranks on the one card with identical shards: the summed histogram is twice the local one, whose per-class medians are the
    same bins, so both ranks derive the single-process thresholds and (identical gradients) its losses."""
    ref_tau, ref_hist, ref_losses = _ddp_thresholds(False)
    world = 2
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    ps = [ctx.Process(target=_ddp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = sorted((q.get(timeout=300) for _ in range(world)), key=lambda r: r[0])
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    for rank, tau, hist, losses in res:
        assert torch.equal(torch.from_numpy(hist), 2 * ref_hist), rank
        assert torch.equal(torch.from_numpy(tau), ref_tau), (rank, tau.tolist(), ref_tau.tolist())
        assert losses == ref_losses, (rank, losses, ref_losses)
