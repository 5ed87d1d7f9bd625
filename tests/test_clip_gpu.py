"""GPU: clipping by the global gradient norm at the optimiser and trainer level -- UNet(4, 3, 4) at 32 x 32, batch 2, fp32, three steps,
FusedAdam and FusedSGD alike.  Measuring only (max_norm = inf) leaves the unclipped run's bits; a clipped run equals the unclipped
optimiser fed the read-back effective scale as its grad_scale, bit for bit; the norm follows grad_scale; the path integral sees the
clipped gradient; head growth, the trainer's statistics, and the replay of a captured step."""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

import clip_ref
import path_ref

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
NC, CD, SIZE, B, STEPS = 4, 4, 32, 2, 3
STAT_KEYS = {'loss', 'pixel_acc', 'class_acc', 'mean_iu', 'max_class_acc', 'lr'}


@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    C._lib.load()
    return C


def f64(t):
    return t.detach().to(torch.float64).cpu().numpy()


def _data(C, nc=NC, n=STEPS):
    return [(torch.from_numpy(C.synth.images(31, B, 3, SIZE, SIZE, first_image=B * i)).to(DEV),
             torch.from_numpy(C.synth.labels(31, B, SIZE, SIZE, nc, first_image=B * i)).to(DEV)) for i in range(n)]


def _make(C, kind, params, **kw):
    if kind == 'adam':
        return C.FusedAdam(params, lr=1e-3, betas=[0.5, 0.99], **kw)
    return C.FusedSGD(params, lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-4, **kw)


def _run(C, kind, max_norm=None, grad_scale=1.0, scales=None, path=False):
    """Three steps from seed 11.  scales: the grad_scale of every step (an unclipped run fed a clipped run's effective scales).
    -> the optimiser and, per step, dict(before, params, grads, omega0, omega and, with clipping, norm, coef, eff, flag, tensor_norms)."""
    torch.manual_seed(11)
    model = C.UNet(NC, 3, CD).to(DEV).train()
    params = list(model.parameters())
    opt = _make(C, kind, params, grad_scale=grad_scale)
    opt.set_grad_clip(max_norm)
    omega = None
    if path:
        omega = C.PathIntegral(model.named_parameters())
        opt.set_path_integral(omega.omega)
    crit = C.CrossEntropyLoss()
    log = []
    for s, (x, y) in enumerate(_data(C)):
        out = model(x)
        opt.zero_grad()
        crit(out, y).backward()
        if scales is not None:
            opt.grad_scale = scales[s]
        rec = dict(before=[p.detach().clone() for p in params], omega0=[w.clone() for w in omega.omega] if path else None)
        opt.step()
        torch.cuda.synchronize()
        rec.update(params=[p.detach().clone() for p in params], grads=[p.grad.clone() for p in params],
                   omega=[w.clone() for w in omega.omega] if path else None)
        if max_norm is not None:
            rec.update(norm=float(opt.grad_norm), coef=float(opt.clip_coef), eff=float(opt.effective_grad_scale), flag=float(opt.grad_nonfinite),
                       tensor_norms=opt.tensor_grad_norms.cpu().double().numpy())
        log.append(rec)
    return opt, log


def _same_params(a, b, what):
    for s, (ra, rb) in enumerate(zip(a, b)):
        for i, (p, q) in enumerate(zip(ra['params'], rb['params'])):
            assert torch.equal(p.view(torch.int32), q.view(torch.int32)), f'{what}: step {s}, parameter {i} differs'


_PLAIN = {}


def _plain(C, kind):
    """The unclipped run, once per optimiser."""
    if kind not in _PLAIN:
        _PLAIN[kind] = _run(C, kind)[1]
    return _PLAIN[kind]


@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_measuring_only_leaves_the_unclipped_bits(C, kind):
    """set_grad_clip(inf): parameters after every step bit-identical to the unclipped optimiser's; grad_norm and tensor_grad_norms equal the
    float64 norms of p.grad within 1e-6 relative (fp32 sums of squares in blocks of 4096 with fp64 above them: a few 1e-8)."""
    plain = _plain(C, kind)
    opt, log = _run(C, kind, max_norm=math.inf)
    _same_params(plain, log, 'max_norm = inf')
    for s, rec in enumerate(log):
        ref = clip_ref.clip([f64(g) for g in rec['grads']], math.inf)
        err = abs(rec['norm'] - ref['norm']) / ref['norm']
        terr = np.abs(rec['tensor_norms'] - ref['tensor_norms']) / np.maximum(ref['tensor_norms'], 1e-300)
        print(f'{kind} step {s}: grad_norm {rec["norm"]:.6g}, relative error {err:.2e}; per tensor at most {terr.max():.2e}')
        assert err <= 1e-6 and terr.max() <= 1e-6
        assert rec['coef'] == 1.0 and rec['eff'] == 1.0 and rec['flag'] == 0.0
    assert len(log[0]['tensor_norms']) == len(log[0]['grads'])
    assert set(opt.state_dict()) == {'state', 'param_groups'}


@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_clipped_run_is_the_unclipped_optimiser_at_the_effective_scale(C, kind):
    """max_norm = 0.1 x the first step's norm: the coefficient is below 1, and the run equals the unclipped optimiser whose grad_scale is
    set, step by step, to the read-back effective scale -- bit for bit, so the step kernel is the same and only its scale differs.  With
    grad_scale 0.5 the reported norm of the first step (same weights, same gradients) is exactly half: the factor is a power of two."""
    first = clip_ref.clip([f64(g) for g in _plain(C, kind)[0]['grads']], math.inf)['norm']
    max_norm = 0.1 * first
    _, log = _run(C, kind, max_norm=max_norm)
    for s, rec in enumerate(log):
        ref = clip_ref.clip([f64(g) for g in rec['grads']], max_norm)
        print(f'{kind} step {s}: norm {rec["norm"]:.6g} coef {rec["coef"]:.6g} (float64 {ref["coef"]:.6g})')
        assert abs(rec['coef'] - ref['coef']) <= 1e-6 * ref['coef'] and rec['flag'] == 0.0
        assert rec['eff'] == rec['coef']                                       # grad_scale 1
    assert log[0]['coef'] < 1 and abs(log[0]['coef'] - 0.1) < 1e-3
    _, fed = _run(C, kind, scales=[rec['eff'] for rec in log])
    _same_params(log, fed, 'clipped vs unclipped at the effective scale')
    assert not torch.equal(log[0]['params'][0], _plain(C, kind)[0]['params'][0])      # and clipping did change the step
    _, half = _run(C, kind, max_norm=max_norm, grad_scale=0.5)
    assert half[0]['norm'] == 0.5 * log[0]['norm']
    assert np.array_equal(half[0]['tensor_norms'], 0.5 * log[0]['tensor_norms'])
    want = clip_ref.clip([f64(g) for g in half[0]['grads']], max_norm, 0.5)
    assert abs(half[0]['coef'] - want['coef']) <= 1e-6 * want['coef'] and abs(half[0]['eff'] - want['scale']) <= 1e-6 * want['scale']
    assert half[0]['eff'] == float(np.float32(0.5) * np.float32(half[0]['coef']))


@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_path_integral_sees_the_clipped_gradient(C, kind):
    """set_path_integral with clipping: per step and element omega against path_ref.omega_from_kernel_values with the effective scale
    (the gradient the step consumed), on the kernel's own parameters before and after."""
    first = clip_ref.clip([f64(g) for g in _plain(C, kind)[0]['grads']], math.inf)['norm']
    _, log = _run(C, kind, max_norm=0.1 * first, path=True)
    worst, apart, tensors = 0.0, 0, 0
    for s, rec in enumerate(log):
        assert rec['coef'] < 1
        for i, (w0, w1, g, p0, p1) in enumerate(zip(rec['omega0'], rec['omega'], rec['grads'], rec['before'], rec['params'])):
            want, bound = path_ref.omega_from_kernel_values(f64(w0), f64(g), rec['eff'], f64(p0), f64(p1))
            r = float((np.abs(f64(w1) - want) / bound).max())
            worst = max(worst, r)
            assert r <= 1.0, (kind, s, i, r)
            # the unclipped gradient would be ten times as large: the bound tells them apart wherever a gradient is not zero
            far, _ = path_ref.omega_from_kernel_values(f64(w0), f64(g), 1.0, f64(p0), f64(p1))
            apart += float((np.abs(f64(w1) - far) / bound).max()) > 1.0
            tensors += 1
    assert apart > tensors // 2, (apart, tensors)
    print(f'{kind}: omega with clipping, worst error / bound {worst:.3f}')
    assert any(bool(w.any()) for w in log[-1]['omega'])


def _launched(C, monkeypatch):
    names = []
    real = C.unet._hbm
    monkeypatch.setattr(C.unet, '_hbm', lambda family, nbytes, name, *args: (names.append((name, nbytes)), real(family, nbytes, name, *args))[1])
    return names


@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_trainer_statistics_and_head_growth(C, monkeypatch, kind):
    """Trainer(max_grad_norm=1.0, stats_every=1) reports grad_norm and clipped and launches the norm pass once per step; with None the
    statistics' keys and the optimiser launches are what they were.  After grow_head(1) the next clipped step runs and tensor_grad_norms
    has the grown head's rows.  A non-finite norm raises a ValueError that names the iteration."""
    data = _data(C)
    names = _launched(C, monkeypatch)
    cfg = lambda **kw: C.default_config(n_iters=10, lr=1e-3, num_classes=NC, conv_dim=CD, compute_dtype='fp32', stats_every=1, optimizer=kind, **kw)
    torch.manual_seed(2)
    off = C.Trainer(data, cfg())
    stats = off.train_epoch(0)
    assert set(stats) == STAT_KEYS
    numel = sum(p.numel() for p in off.model.parameters())
    opt_launches = [n for n in names if n[0].startswith(('clamd_adam', 'clamd_sgd', 'clamd_grad'))]
    assert opt_launches == [(f'clamd_{kind}_step', (28 if kind == 'adam' else 20) * numel)] * STEPS, opt_launches
    assert off.optim._clip_out is None and off.optim._hyper_eff is None
    del names[:]
    torch.manual_seed(2)
    tr = C.Trainer(data, cfg(max_grad_norm=1.0))
    stats = tr.train_epoch(0)
    assert set(stats) == STAT_KEYS | {'grad_norm', 'clipped'}
    assert math.isfinite(stats['grad_norm']) and stats['grad_norm'] > 0 and 0.0 <= stats['clipped'] <= 1.0
    opt_launches = [n for n in names if n[0].startswith(('clamd_adam', 'clamd_sgd', 'clamd_grad'))]
    assert opt_launches == [('clamd_grad_norm_clip', 4 * numel), (f'clamd_{kind}_step', (28 if kind == 'adam' else 20) * numel)] * STEPS, opt_launches
    # head growth
    nparams = len(list(tr.model.parameters()))
    tr.grow_head(1)
    x, _ = data[0]
    y = torch.from_numpy(C.synth.labels(32, B, SIZE, SIZE, NC + 1)).to(DEV)
    _, loss = tr.train_step(x, y)
    torch.cuda.synchronize()
    assert math.isfinite(float(loss.detach())) and float(tr.optim.grad_nonfinite) == 0.0
    params = list(tr.model.parameters())
    tn = tr.optim.tensor_grad_norms.cpu().double().numpy()
    assert len(tn) == nparams == len(params) and params[-2].shape[0] == NC + 1 and params[-1].shape == (NC + 1,)
    ref = clip_ref.clip([f64(p.grad) for p in params], 1.0)
    assert np.all(np.abs(tn - ref['tensor_norms']) <= 1e-6 * ref['tensor_norms']) and tn[-1] > 0 and tn[-2] > 0
    assert abs(float(tr.optim.grad_norm) - ref['norm']) <= 1e-6 * ref['norm']
    assert abs(float(tr.optim.clip_coef) - ref['coef']) <= 1e-6 * ref['coef']
    # a non-finite gradient in the last iteration (planted in front of the step, where ddp.GradSync.wait runs)
    torch.manual_seed(2)
    bad = C.Trainer(data, cfg(max_grad_norm=1.0))
    calls = []

    def plant():
        calls.append(1)
        if len(calls) == STEPS:
            next(iter(bad.model.parameters())).grad.view(-1)[0] = math.nan
    bad.optim.pre_step_hooks.append(plant)
    with pytest.raises(ValueError, match=f'iteration {STEPS - 1}'):
        bad.train_epoch(0)


def test_captured_step_replays_with_a_new_coefficient(C):
    """One eager step, then FusedSGD.step() alone in a torch.cuda.graph (a linear chain: norm pass, finalize, step).  Replayed after the
    gradient contents were doubled in place, the norm doubles exactly and the coefficient halves (to the 1e-6 of its denominator), with no
    host work in between: nothing of the clipping lives on the host."""
    rng = np.random.default_rng(5)
    shapes = [(5000,), (33, 125), (4097,), (3,)]
    ps = [nn.Parameter(torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(DEV)) for s in shapes]
    for p in ps:
        p.grad = torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(np.float32)).to(DEV)
    norm0 = clip_ref.clip([f64(p.grad) for p in ps], math.inf)['norm']
    opt = C.FusedSGD(ps, lr=0.01, momentum=0.9, nesterov=True)
    opt.set_grad_clip(0.25 * norm0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()                                                             # eager: builds the tables, uploads the hyper-parameters
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = (float(opt.grad_norm), float(opt.clip_coef))
    assert abs(eager[0] - norm0) <= 1e-6 * norm0 and abs(eager[1] - 0.25) <= 1e-6
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    graph.replay()
    torch.cuda.synchronize()
    assert (float(opt.grad_norm), float(opt.clip_coef)) == eager
    before = [p.detach().clone() for p in ps]
    for p in ps:
        p.grad.mul_(2.0)
    graph.replay()
    torch.cuda.synchronize()
    assert float(opt.grad_norm) == 2.0 * eager[0]
    assert abs(float(opt.clip_coef) - 0.5 * eager[1]) <= 1e-6 * eager[1] and float(opt.clip_coef) < 0.2
    assert all(not torch.equal(p.detach(), b) for p, b in zip(ps, before))
