"""CPU-only tests of the cross-entropy + soft Dice loss's host side: the closed-form gradient of include/clamd.h against float64 autograd
through the loss itself (tests/dice_ref.py states both), a hand-computed case, the C ABI's validation before any launch, the criterion's
constructor and the trainer's configuration checks.  No kernel is launched here."""
import ctypes
import itertools
import math

import pytest
import torch

import dice_ref


@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    return C


def _inputs(B=3, K=5, H=6, W=7, seed=0, ign=-100):
    """Class K - 1 absent from the batch, class 1 absent from image 0, image 1 all ignored, ignored pixels and two bad labels elsewhere."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, K, H, W, generator=g, dtype=torch.float64) * 3
    y = torch.randint(0, max(K - 1, 1), (B, H, W), generator=g)
    if K > 2:
        y[0][y[0] == 1] = 2
    if B > 1:
        y[1] = ign
    y[0, 0, :3] = ign; y[0, 1, 0] = K + 2; y[-1, -1, -1] = -7
    return z, y


def _autograd(z, y, **kw):
    zz = z.clone().requires_grad_()
    tot, ce, dice = dice_ref.dice_ce(zz, y, **kw)
    g, = torch.autograd.grad(tot, zz)
    return float(tot.detach()), float(ce.detach()), float(dice.detach()), g


@pytest.mark.parametrize('per_image,present_only,first_class', list(itertools.product((False, True), (False, True), (0, 1))))
def test_closed_form_equals_float64_autograd(per_image, present_only, first_class):
    kw = dict(w_ce=0.7, w_dice=1.3, smooth=1e-5, first_class=first_class, present_only=present_only, per_image=per_image)
    for K, smooth in ((5, 1e-5), (5, 0.0), (2, 1.0), (1, 1e-5)):
        z, y = _inputs(K=K, seed=K)
        k2 = dict(kw, smooth=smooth)
        tot, ce, dice, g = _autograd(z, y, **k2)
        cf = dice_ref.closed_form(z, y, **k2)
        assert float((cf - g).abs().max()) <= 1e-12, (K, smooth, float((cf - g).abs().max()))
        assert tot == pytest.approx(ce + dice, abs=1e-15)
        invalid = ~((y != -100) & (y >= 0) & (y < K))
        assert float(g.permute(0, 2, 3, 1)[invalid].abs().max()) == 0.0 and float(cf.permute(0, 2, 3, 1)[invalid].abs().max()) == 0.0
        s, nvalid, nbad = dice_ref.pixel_scale(z, y, 2.0, **k2)
        assert nbad == 2 and nvalid == int((~invalid).sum()) and bool(((s > 0) == ~invalid).all())
        if K == 1:                      # one class: softmax is 1 everywhere and nothing depends on the logits
            assert float(g.abs().max()) == 0.0 and ce == 0.0
        if K == 5 and first_class == 0 and not present_only and smooth > 0:
            c, a, nS = dice_ref.coefficients(z, y, 1.3, smooth, 0, False, per_image)
            assert nS.tolist() == [5] * (3 if per_image else 1)
            assert bool((c[:, 4] > 0).all())            # an absent class outside present_only still pushes its probability down


@pytest.mark.parametrize('per_image', [False, True])
@pytest.mark.parametrize('present_only', [False, True])
def test_all_pixels_ignored_gives_zero(per_image, present_only):
    z, y = _inputs()
    y[:] = -100
    tot, ce, dice, g = _autograd(z, y, present_only=present_only, per_image=per_image, smooth=1e-5)
    assert (tot, ce, dice) == (0.0, 0.0, 0.0) and float(g.abs().max()) == 0.0
    assert float(dice_ref.closed_form(z, y, present_only=present_only, per_image=per_image).abs().max()) == 0.0
    # smooth = 0 as well: D == 0 makes every dice 1
    tot, ce, dice, g = _autograd(z, y, present_only=present_only, per_image=per_image, smooth=0.0)
    assert (tot, ce, dice) == (0.0, 0.0, 0.0) and float(g.abs().max()) == 0.0


def test_present_only_without_a_class_at_or_above_first_class():
    z, y = _inputs()
    y[(y != -100) & (y >= 0) & (y < 5)] = 0                    # background only
    tot, ce, dice, g = _autograd(z, y, first_class=1, present_only=True)
    assert dice == 0.0 and tot == ce > 0
    zz = z.clone().requires_grad_()
    plain, = torch.autograd.grad(dice_ref.dice_ce(zz, y, w_dice=0.0)[0], zz)
    assert torch.equal(g, plain)


def test_hand_computed_two_pixels():
    """K = 2, pixels (p = (1/2, 1/2), y = 0) and (p = (3/4, 1/4), y = 1), smooth = 0, batch Dice over both classes:
    I = (1/2, 1/4), P = (5/4, 3/4), Y = (1, 1): dice = (1 / (9/4), (1/2) / (7/4)) = (4/9, 2/7), L = 1 - (4/9 + 2/7) / 2 = 40/63;
    CE = (ln 2 + ln 4) / 2.  u = 1/2: c = (8/81, 4/49), a = (-4/9, -4/7); on pixel 0 g = (8/81 - 4/9, 4/49) and
    d L / d z_0 = p_0 (g_0 - (g_0 + g_1) / 2) = (g_0 - g_1) / 4 = -424/3969, d L / d z_1 the opposite."""
    z = torch.tensor([[[[0.0, math.log(3.0)]], [[0.0, 0.0]]]], dtype=torch.float64)
    y = torch.tensor([[[0, 1]]])
    tot, ce, dice = dice_ref.dice_ce(z, y, smooth=0.0, present_only=False)
    assert float(dice) == pytest.approx(40 / 63, rel=1e-14) and float(ce) == pytest.approx(1.5 * math.log(2.0), rel=1e-14)
    assert float(tot) == pytest.approx(40 / 63 + 1.5 * math.log(2.0), rel=1e-14)
    c, a, nS = dice_ref.coefficients(z, y, smooth=0.0, present_only=False)
    assert c[0].tolist() == pytest.approx([8 / 81, 4 / 49], rel=1e-14) and a[0].tolist() == pytest.approx([-4 / 9, -4 / 7], rel=1e-14)
    assert nS.tolist() == [2]
    g = dice_ref.closed_form(z, y, w_ce=0.0, smooth=0.0, present_only=False)
    assert g[0, :, 0, 0].tolist() == pytest.approx([-424 / 3969, 424 / 3969], rel=1e-13)
    _, _, _, ga = _autograd(z, y, w_ce=0.0, smooth=0.0, present_only=False)
    assert float((g - ga).abs().max()) <= 1e-15


_ARGS = ('logits labels dlogits dl_nhwc dl_ldc dl_dtype loss3 workspace ws_bytes B K H W ignore_index w_ce w_dice smooth first_class '
         'present_only per_image grad_scale stream').split()


def test_entry_point_rejects_bad_arguments_before_any_launch(C):
    """Pattern of test_sgd_cpu.py: every call fails validation on the host (the non-null pointers are host memory that nothing
    dereferences), returns a negative status, and clamd_last_error() names the problem."""
    lib = C._lib.load()
    buf = ctypes.create_string_buffer(4096)
    a = (ctypes.addressof(buf) + 63) & ~63
    B, K, H, W = 2, 5, 8, 12
    need = lib.clamd_ce_dice_workspace_bytes(B, K, H, W, 1)
    assert need > lib.clamd_ce_workspace_bytes() and need % 4 == 0
    assert lib.clamd_ce_dice_workspace_bytes(B, K, H, W, 0) < need               # one group's table instead of B
    for bad in ((0, K, H, W), (B, 0, H, W), (B, 33, H, W), (B, K, 0, W), (B, K, H, -1), (2049, K, H, W)):
        assert lib.clamd_ce_dice_workspace_bytes(*bad, 0) == 0
    assert lib.clamd_ce_dice_workspace_bytes(2048, 32, 4, 4, 1) > 0
    base = dict(logits=a, labels=a, dlogits=a, dl_nhwc=None, dl_ldc=0, dl_dtype=0, loss3=a, workspace=a, ws_bytes=need, B=B, K=K, H=H, W=W,
                ignore_index=-100, w_ce=1.0, w_dice=1.0, smooth=1e-5, first_class=0, present_only=1, per_image=1, grad_scale=1.0, stream=None)
    inf, nan = float('inf'), float('nan')
    cases = [('number of classes must be in [1, 32]', dict(K=0)), ('number of classes must be in [1, 32]', dict(K=33)),
             ('first_class must be 0 or 1', dict(first_class=2)), ('first_class must be 0 or 1', dict(first_class=-1))]
    cases += [('must be finite and >= 0', {k: v}) for k in ('w_ce', 'w_dice', 'smooth') for v in (-1e-9, inf, nan)]
    cases += [('pitch >= 32', dict(dl_nhwc=a, dl_ldc=24)), ('pitch >= 32', dict(dl_nhwc=a, dl_ldc=0)),
              ('workspace too small', dict(ws_bytes=need - 4)), ('workspace too small', dict(ws_bytes=lib.clamd_ce_workspace_bytes())),
              ('workspace too small', dict(ws_bytes=0)), ('workspace must be 16-byte aligned', dict(workspace=a + 8)),
              ('more than 2048 images', dict(B=2049, ws_bytes=1 << 40))]
    cases += [('null pointer or empty shape', {k: None}) for k in ('logits', 'labels', 'dlogits', 'loss3', 'workspace')]
    cases += [('null pointer or empty shape', {k: 0}) for k in ('B', 'H', 'W')]
    for needle, kw in cases:
        args = dict(base, **kw)
        with pytest.raises(RuntimeError) as e:
            C._lib.call('clamd_ce_dice_fwd_bwd', *[args[k] for k in _ARGS])
        assert needle in str(e.value) and 'ce_dice' in str(e.value), (kw, str(e.value))
        msg = lib.clamd_last_error().decode()
        assert needle in msg and msg.startswith('ce_dice: '), msg
    assert bytes(buf) == bytes(4096)                   # untouched


def test_constructor_errors_and_exports(C):
    for kw in (dict(ce_weight=-1.0), dict(dice_weight=-0.5), dict(smooth=-1e-6), dict(ce_weight=0.0, dice_weight=0.0),
               dict(dice_weight=float('inf')), dict(smooth=float('nan'))):
        with pytest.raises(ValueError, match='DiceCrossEntropyLoss'):
            C.DiceCrossEntropyLoss(**kw)
    crit = C.DiceCrossEntropyLoss()
    assert (crit.ce_weight, crit.dice_weight, crit.smooth, crit.include_background, crit.present_only, crit.per_image, crit.ignore_index) == \
        (1.0, 1.0, 1e-5, True, True, False, -100)
    assert crit.parts is None and crit.bad_labels is None
    C.DiceCrossEntropyLoss(ce_weight=0.0)
    C.DiceCrossEntropyLoss(dice_weight=0.0, smooth=0.0)
    assert 'DiceCrossEntropyLoss' in C.__all__
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        crit(torch.zeros(1, 5, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))


def test_default_config_and_begin_task2_checks(C):
    cfg = C.default_config()
    assert (cfg.loss, cfg.dice_weight, cfg.dice_smooth, cfg.dice_include_background, cfg.dice_present_only, cfg.dice_per_image) == \
        ('ce', 1.0, 1e-5, True, True, False)
    plain = C.Trainer([], C.default_config(num_classes=5, conv_dim=4), device='cpu')
    assert type(plain.c_loss) is C.CrossEntropyLoss and plain.likelihood_loss is plain.c_loss
    with pytest.raises(ValueError, match="loss must be 'ce' or 'ce_dice'"):
        C.Trainer([], C.default_config(num_classes=5, conv_dim=4, loss='dice'), device='cpu')
    with pytest.raises(ValueError, match='DiceCrossEntropyLoss'):
        C.Trainer([], C.default_config(num_classes=5, conv_dim=4, loss='ce_dice', dice_weight=-1.0), device='cpu')
    tr = C.Trainer([], C.default_config(num_classes=5, conv_dim=4, loss='ce_dice', dice_weight=0.5, dice_smooth=1e-3, dice_include_background=False,
                                        dice_present_only=False, dice_per_image=True), device='cpu')
    crit = tr.c_loss
    assert isinstance(crit, C.DiceCrossEntropyLoss) and type(tr.likelihood_loss) is C.CrossEntropyLoss
    assert (crit.ce_weight, crit.dice_weight, crit.smooth, crit.include_background, crit.present_only, crit.per_image) == \
        (1.0, 0.5, 1e-3, False, False, True)
    with pytest.raises(ValueError, match='distill_lambda > 0'):
        tr.begin_task2(c_old=3)                                     # the default distill_lambda is 1
    with pytest.raises(ValueError, match='unbiased=True'):
        tr.begin_task2(c_old=3, distill_lambda=0.0, unbiased=True)
    with pytest.raises(ValueError, match='pseudo_adaptive=True'):
        tr.begin_task2(c_old=3, distill_lambda=0.0, pseudo_label=True, pseudo_adaptive=True)
    assert tr.old_model is None and tr.pseudo is None and tr.pod is None          # refused before anything was switched on
