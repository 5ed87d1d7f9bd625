"""CPU-only tests of the class-weighted / label-smoothed / focal cross-entropy's host side: tests/wce_ref.py against torch's own criterion and
against float64 autograd, loss.class_weights against hand-computed cases, the C ABI's validation before any launch, the criterion's
constructor and the trainer's configuration checks.  No kernel is launched here."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import wce_ref


@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    return C


def _inputs(B=3, K=5, H=6, W=7, seed=0, ign=-100, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, K, H, W, generator=g, dtype=torch.float64) * scale
    y = torch.randint(0, K, (B, H, W), generator=g)
    y[0, 0, :3] = ign; y[1, 2, 1:4] = ign
    return z, y


@pytest.mark.parametrize('ign', [-100, 255])
@pytest.mark.parametrize('eps', [0.0, 0.1])
@pytest.mark.parametrize('zero_class', [False, True])
def test_reference_equals_torch_cross_entropy(eps, zero_class, ign):
    """gamma = 0: loss and gradient of F.cross_entropy(weight=, label_smoothing=, ignore_index=) in float64, to 1e-12; with a class of
    weight 0 torch too divides the smoothing term by sum w_y and keeps the smoothing term of that class's pixels."""
    z, y = _inputs(ign=ign)
    w = torch.tensor([0.5, 2.0, 1.0, 3.5, 0.25], dtype=torch.float64)
    if zero_class:
        w[1] = 0.0
        assert bool((y == 1).any())
    zz = z.clone().requires_grad_()
    loss = F.cross_entropy(zz, y, weight=w, label_smoothing=eps, ignore_index=ign)
    g, = torch.autograd.grad(loss, zz)
    loss = loss.detach()
    r = wce_ref.wce(z, y, w, eps=eps, ignore_index=ign)
    assert abs(float(r.l3[0]) - float(loss)) <= 1e-12 * max(1.0, abs(float(loss)))
    assert float((r.grad - g).abs().max()) <= 1e-12
    assert float(r.l3[0]) == float(r.l3[1] + r.l3[2]) and (eps > 0 or float(r.l3[2]) == 0.0)
    assert r.nbad == 0 and r.nvalid == y.numel() - 6
    # unit weights and no smoothing: the plain criterion
    if eps == 0.0:
        r1 = wce_ref.wce(z, y, ignore_index=ign)
        assert abs(float(r1.l3[0]) - float(F.cross_entropy(z, y, ignore_index=ign))) <= 1e-12


@pytest.mark.parametrize('gamma', [0.5, 2.0])
def test_focal_closed_form_equals_autograd(gamma):
    """f = q^gamma (1 + gamma p_y t / q) times (p_k - [k = y]) is the derivative of q^gamma t.  Float64 at logit scale 3, where autograd
    through -log_softmax is itself accurate; 1e-9 of the largest gradient (its rounding, not the closed form's, sets the figure)."""
    z, y = _inputs(seed=3)
    y[2, 0, 0] = 9; y[2, 0, 1] = -3
    w = torch.tensor([0.5, 2.0, 0.0, 3.5, 0.25], dtype=torch.float64)
    loss, g = wce_ref.focal_by_autograd(z, y, w, gamma)
    r = wce_ref.wce(z, y, w, gamma=gamma)
    assert r.nbad == 2
    assert abs(float(r.l3[0]) - float(loss)) <= 1e-12 * max(1.0, abs(float(loss)))
    assert float((r.grad - g).abs().max()) <= 1e-9 * float(g.abs().max())
    # image weights multiply the pixel's term and gradient, not the denominator
    nu = torch.tensor([1.75, 0.0, 0.4], dtype=torch.float64)
    rn = wce_ref.wce(z, y, w, nu=nu, gamma=gamma)
    assert float(rn.D) == float(r.D)
    assert torch.allclose(rn.grad, r.grad * nu[:, None, None, None], rtol=1e-13, atol=0)
    assert float(rn.grad[1].abs().max()) == 0.0 and float(rn.s_px[1].max()) == 0.0


def test_reference_edge_cases():
    z, y = _inputs()
    with pytest.raises(ValueError, match='together'):
        wce_ref.wce(z, y, eps=0.1, gamma=2.0)
    # D == 0: nothing valid; every valid pixel on a class of weight 0 -- zeros where torch gives NaN
    r = wce_ref.wce(z, torch.full_like(y, -100), eps=0.1)
    assert [float(v) for v in r.l3] == [0.0, 0.0, 0.0] and float(r.grad.abs().max()) == 0.0
    w = torch.zeros(5, dtype=torch.float64); w[4] = 2.0
    y4 = y.clamp(max=3)
    r = wce_ref.wce(z, y4, w, eps=0.1)
    assert float(r.D) == 0.0 and [float(v) for v in r.l3] == [0.0, 0.0, 0.0] and float(r.grad.abs().max()) == 0.0
    assert math.isnan(float(F.cross_entropy(z, y4, weight=w, label_smoothing=0.1)))
    # a confidently right focal pixel: q = 0 in float32, f = 0, the scale's floor keeps the ratio meaningful
    zc = torch.zeros(1, 3, 1, 1, dtype=torch.float32); zc[0, 1] = 200.0
    r = wce_ref.wce(zc, torch.ones(1, 1, 1, dtype=torch.int64), gamma=2.0)
    assert float(r.grad.abs().max()) == 0.0 and float(r.s_px) == 2.0 ** -40


def test_class_weights_by_hand(C):
    # three images, K = 4; class 3 never occurs; class 2 only in image 1
    counts = torch.tensor([[60, 40, 0, 0], [10, 0, 90, 0], [100, 100, 0, 0]], dtype=torch.int32)
    # median frequency: freq_k = n_k / pixels of the images containing k = 170/400, 140/300, 90/100; median = 140/300
    w = C.loss.class_weights(counts, 'median_frequency')
    f = [170 / 400, 140 / 300, 90 / 100]
    want = [f[1] / f[0], 1.0, f[1] / f[2], 1.0]
    assert w.dtype == torch.float32 and w.shape == (4,) and w.tolist() == pytest.approx(want, rel=1e-6)
    # two classes present: the median of an even number is the middle pair's mean
    w2 = C.class_weights(torch.tensor([[30, 10, 0]]), 'median_frequency')
    assert w2.tolist() == pytest.approx([0.5 / 0.75, 0.5 / 0.25, 1.0], rel=1e-6)
    # inverse log (ENet): 1 / ln(1.02 + n_k / sum n), n = 170, 140, 90 of 400
    wl = C.loss.class_weights(counts, 'inverse_log')
    wantl = [1 / math.log(1.02 + n / 400) for n in (170, 140, 90)] + [1.0]
    assert wl.tolist() == pytest.approx(wantl, rel=1e-6)
    wn = C.loss.class_weights(counts, 'inverse_log', normalize=True)
    m = sum(wantl[:3]) / 3
    assert wn.tolist() == pytest.approx([v / m for v in wantl[:3]] + [1.0], rel=1e-6)
    assert C.loss.class_weights(torch.zeros(2, 3, dtype=torch.int64), 'median_frequency').tolist() == [1.0, 1.0, 1.0]
    with pytest.raises(ValueError, match='scheme'):
        C.loss.class_weights(counts, 'balanced')
    with pytest.raises(ValueError, match='integer'):
        C.loss.class_weights(counts.float(), 'inverse_log')
    with pytest.raises(ValueError, match='integer'):
        C.loss.class_weights(counts[0], 'inverse_log')


def test_criterion_constructs_and_validates(C):
    crit = C.CrossEntropyLoss(weight=torch.tensor([1.0, 2.0, 0.0]))          # TypeError before this feature
    assert crit.weight.dtype == torch.float32 and crit.weight.tolist() == [1.0, 2.0, 0.0] and crit.generalised
    assert 'weight' not in crit.state_dict() and crit.ignore_index == -100
    assert crit.to(torch.float32).weight is not None
    plain = C.CrossEntropyLoss()
    assert plain.weight is None and not plain.generalised and (plain.label_smoothing, plain.focal_gamma) == (0.0, 0.0)
    assert C.CrossEntropyLoss(255).ignore_index == 255
    assert C.CrossEntropyLoss(label_smoothing=0.1).generalised and C.CrossEntropyLoss(focal_gamma=2).generalised
    assert C.CrossEntropyLoss(weight=[1, 2, 3]).weight.tolist() == [1.0, 2.0, 3.0]
    with pytest.raises(TypeError):
        C.CrossEntropyLoss(-100, torch.ones(3))                              # the new arguments are keyword-only
    for kw, needle in ((dict(weight=torch.tensor([1.0, -1.0])), 'finite and >= 0'), (dict(weight=torch.tensor([1.0, float('nan')])), 'finite'),
                       (dict(weight=torch.tensor([1.0, float('inf')])), 'finite'), (dict(weight=torch.ones(2, 2)), 'vector'),
                       (dict(weight=torch.ones(0)), 'vector'), (dict(label_smoothing=1.0), r'\[0, 1\)'), (dict(label_smoothing=-0.1), r'\[0, 1\)'),
                       (dict(focal_gamma=-1.0), 'focal_gamma'), (dict(focal_gamma=float('inf')), 'focal_gamma'),
                       (dict(focal_gamma=float('nan')), 'focal_gamma'), (dict(label_smoothing=0.1, focal_gamma=2.0), 'both non-zero')):
        with pytest.raises(ValueError, match=needle):
            C.CrossEntropyLoss(**kw)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        crit(torch.zeros(1, 3, 2, 2), torch.zeros(1, 2, 2, dtype=torch.int64))
    crit.set_weight(None)
    assert crit.weight is None and not crit.generalised
    # a positive weight below 1e-30 could make D so small that grad_scale / (float)D overflows: refused; 0 and 1e-30 pass
    for bad in (1e-38, 1e-45, 9e-31):
        with pytest.raises(ValueError, match='0 or at least 1e-30'):
            C.CrossEntropyLoss(weight=[1.0, bad])
    assert C.CrossEntropyLoss(weight=[0.0, 1e-30, 2e-30]).weight.tolist()[0] == 0.0


_ARGS = ('logits', 'labels', 'class_weight', 'image_weight', 'dlogits', 'dl_nhwc', 'dl_ldc', 'dl_dtype', 'loss3', 'workspace', 'ws_bytes', 'B', 'K',
         'H', 'W', 'ignore_index', 'label_smoothing', 'focal_gamma', 'grad_scale', 'stream')


def test_abi_rejects_before_any_launch(C):
    """Every rejection returns before a launch (host addresses stand in for device pointers: nothing dereferences them), with a negative
    status and a message that names the entry point."""
    lib = C._lib.load()
    buf = ctypes.create_string_buffer(4096)
    a = (ctypes.addressof(buf) + 63) & ~63
    need = lib.clamd_ce_class_workspace_bytes()
    assert need > lib.clamd_ce_workspace_bytes() and need % 8 == 0
    base = dict(logits=a, labels=a, class_weight=a, image_weight=None, dlogits=a, dl_nhwc=None, dl_ldc=0, dl_dtype=0, loss3=a, workspace=a,
                ws_bytes=need, B=2, K=5, H=8, W=12, ignore_index=-100, label_smoothing=0.0, focal_gamma=0.0, grad_scale=1.0, stream=None)
    for kw, needle in ((dict(class_weight=None), 'class_weight'), (dict(class_weight=a + 2), 'class_weight'), (dict(image_weight=a + 2), 'image_weight'),
                       (dict(label_smoothing=1.0), 'label_smoothing'), (dict(label_smoothing=-0.5), 'label_smoothing'),
                       (dict(label_smoothing=float('nan')), 'label_smoothing'), (dict(focal_gamma=-1.0), 'focal_gamma'),
                       (dict(focal_gamma=float('inf')), 'focal_gamma'), (dict(focal_gamma=float('nan')), 'focal_gamma'),
                       (dict(label_smoothing=0.1, focal_gamma=2.0), 'both non-zero'), (dict(ws_bytes=need - 4), 'workspace'),
                       (dict(ws_bytes=lib.clamd_ce_workspace_bytes()), 'workspace'), (dict(workspace=a + 4), 'workspace'),
                       (dict(K=0), 'classes'), (dict(K=33), 'classes'), (dict(logits=None), 'null'), (dict(labels=None), 'null'),
                       (dict(dlogits=None), 'null'), (dict(loss3=None), 'null'), (dict(workspace=None), 'null'), (dict(B=0), 'empty shape'),
                       (dict(logits=a + 2), 'misaligned'), (dict(labels=a + 4), 'misaligned'), (dict(dl_nhwc=a, dl_ldc=16), 'pitch'),
                       (dict(dl_nhwc=a, dl_ldc=32, dl_dtype=7), 'dtype')):
        args = dict(base, **kw)
        with pytest.raises(RuntimeError) as e:
            C._lib.call('clamd_ce_class_fwd_bwd', *[args[k] for k in _ARGS])
        assert needle in str(e.value) and 'ce_class' in str(e.value), (kw, str(e.value))


def test_trainer_configuration(C):
    cfg = C.default_config()
    assert (cfg.class_weights, cfg.label_smoothing, cfg.focal_gamma) == (None, 0.0, 0.0)
    mk = lambda **kw: C.Trainer([], C.default_config(num_classes=5, conv_dim=4, **kw), device='cpu')
    plain = mk()
    assert type(plain.c_loss) is C.CrossEntropyLoss and plain.likelihood_loss is plain.c_loss and not plain.class_criterion_active()
    assert plain.class_weight is None
    tr = mk(class_weights=[1, 2, 0.5, 1, 3])
    assert tr.c_loss is not tr.likelihood_loss and not tr.likelihood_loss.generalised and tr.class_criterion_active()
    assert tr.class_weight.tolist() == [1.0, 2.0, 0.5, 1.0, 3.0]
    assert mk(label_smoothing=0.1).c_loss.label_smoothing == 0.1 and mk(focal_gamma=2.0).c_loss.focal_gamma == 2.0
    for kw, needle in ((dict(class_weights=[1, 2, 3]), '5 entries'), (dict(class_weights=[1, 2, 3, 4, -1]), 'finite and >= 0'),
                       (dict(label_smoothing=1.5), r'\[0, 1\)'), (dict(focal_gamma=-2), 'focal_gamma'),
                       (dict(label_smoothing=0.1, focal_gamma=1.0), 'both non-zero'),
                       (dict(loss='ce_dice', class_weights=[1, 1, 1, 1, 1]), "loss='ce_dice' with class_weights"),
                       (dict(loss='ce_dice', label_smoothing=0.1), "loss='ce_dice' with class_weights"),
                       (dict(loss='ce_dice', focal_gamma=2.0), "loss='ce_dice' with class_weights")):
        with pytest.raises(ValueError, match=needle):
            mk(**kw)
    # set_class_weights: a vector; again; off; the errors
    assert plain.set_class_weights([2, 2, 2, 2, 1]).tolist() == [2.0, 2.0, 2.0, 2.0, 1.0]
    assert plain.c_loss is not plain.likelihood_loss and plain.class_criterion_active() and not plain.likelihood_loss.generalised
    assert plain.set_class_weights(None) is None and not plain.class_criterion_active()
    with pytest.raises(ValueError, match='5 entries'):
        plain.set_class_weights([1, 2])
    with pytest.raises(ValueError, match='needs a loader'):
        plain.set_class_weights('median_frequency')
    with pytest.raises(ValueError, match="needs loss='ce'"):
        mk(loss='ce_dice').set_class_weights([1, 1, 1, 1, 1])
    # the task boundary refuses the criteria that have no class weights, before anything changes
    with pytest.raises(ValueError, match='distill_lambda > 0'):
        tr.begin_task2(2)
    with pytest.raises(ValueError, match='unbiased=True'):
        tr.begin_task2(2, distill_lambda=0.0, unbiased=True)
    assert tr.old_model is None and tr.distill is None
    # ... and in the other order: once the step runs a distillation criterion, weights would be stored and never applied
    late = mk()
    late.begin_task2(2)
    assert late.distill is not None
    with pytest.raises(ValueError, match='DistillationCrossEntropy, which has no class weights'):
        late.set_class_weights([1, 1, 1, 1, 1])
    with pytest.raises(ValueError, match='DistillationCrossEntropy, which has no class weights'):
        late.load_class_weight_state({'weight': torch.ones(5)})
    assert late.set_class_weights(None) is None and late.class_weight is None
    # a checkpoint written after grow_head carries more weights than a Trainer built with the original class count has classes
    with pytest.raises(ValueError, match='written after grow_head'):
        tr.load_class_weight_state({'weight': torch.ones(7)})
    tr.load_class_weight_state({'weight': torch.tensor([3.0, 1, 1, 1, 1])})
    assert tr.class_weight.tolist() == [3.0, 1.0, 1.0, 1.0, 1.0]
    tr.load_class_weight_state(None)
    assert tr.class_weight.tolist() == [3.0, 1.0, 1.0, 1.0, 1.0]
