"""GPU: Synaptic Intelligence at the optimiser and trainer level (build-defined: the reference has no continual-learning code).

    per step    omega += -g * (theta(t+1) - theta(t)),  g = the task-loss gradient the optimiser is handed, inside its kernel
    boundary    Omega <- Omega + max(0, omega) / ((theta - theta_start)^2 + xi);  theta* <- theta;  omega <- 0;  theta_start <- theta
    penalty     c * sum Omega (theta - theta*)^2 = the consolidation term with lambda = 2 c

FusedAdam / FusedSGD with a PathIntegral against the float64 accumulation from their own parameter snapshots; task 1 with tracking on and
off; two tasks against the same procedure composed from stock torch on the same device; a third boundary; head growth; checkpoints."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import path_ref
from conftest import rel_l2
from oracle import torch_cpu as TC
from test_ewc_gpu import _batches, _bns, _check_importance

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
EPS, QUANTUM = 2.0 ** -24, 2.0 ** -149


@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    C._lib.load()
    return C


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(torch.float32).to(DEV)


def f64(t):
    return t.detach().to(torch.float64).cpu().numpy()


def sync():
    torch.cuda.synchronize()


class Accum:
    """The float64 accumulation of omega from a run's own parameter snapshots and gradients, and the bound on the fp32 result: per step five
    roundings of 2^-24 on |omega| + |g * delta| (path_ref.omega_from_kernel_values), |omega| itself at most the sum of the terms so far --
    steps * 5 * 2^-24 * sum |g * delta| -- plus the denormal quantum per step."""

    def __init__(self, params):
        self.omega = [np.zeros(tuple(p.shape)) for p in params]
        self.mag = [np.zeros(tuple(p.shape)) for p in params]
        self.steps = 0

    def add(self, grads, before, after):
        for w, a, g, b, p in zip(self.omega, self.mag, grads, before, after):
            t = f64(g) * (f64(p) - f64(b))
            w -= t
            a += np.abs(t)
        self.steps += 1

    def check(self, omega, what):
        worst = 0.0
        for i, (w, a, got) in enumerate(zip(self.omega, self.mag, omega)):
            bound = self.steps * 5 * EPS * a + self.steps * 4 * QUANTUM
            r = float((np.abs(f64(got) - w) / bound).max())
            worst = max(worst, r)
            assert r <= 1.0, f'{what}: omega[{i}]: error / bound {r:.3f}'
        print(f'{what}: omega vs float64 accumulation over {self.steps} steps: worst error / bound {worst:.3f}')


# ------------------------------------------------------------------------------------------------------------------ optimiser level

@pytest.mark.parametrize('kind', ['adam', 'sgd_momentum', 'sgd_plain'])
def test_fused_optimizers_accumulate_the_path_integral(C, kind):
    """Three tensors (lengths off the chunk and off 4) and three steps: omega after each step against the float64 accumulation.  Plain SGD
    (no momentum, weight decay or anchors): omega == lr * sum g^2, the identity -g * (-lr g) -- a wrong sign or a wrong gradient shows."""
    rng = np.random.default_rng(41)
    shapes = [(5000,), (33, 125), (4097,)]
    lr = 0.1 if kind != 'adam' else 1e-2
    p0 = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    grads = [[rng.standard_normal(s).astype(np.float32) for s in shapes] for _ in range(3)]
    ps = [nn.Parameter(dev(a)) for a in p0]
    if kind == 'adam':
        opt = C.FusedAdam(ps, lr=lr, betas=[0.5, 0.99])
    elif kind == 'sgd_momentum':
        opt = C.FusedSGD(ps, lr=lr, momentum=0.9, nesterov=True, weight_decay=0.05)
    else:
        opt = C.FusedSGD(ps, lr=lr)
    path = C.PathIntegral([(f't{i}', p) for i, p in enumerate(ps)])
    opt.set_path_integral(path.omega)
    acc = Accum(ps)
    for s in range(3):
        before = [p.detach().clone() for p in ps]
        for p, g in zip(ps, grads[s]):
            p.grad = dev(g)
        opt.step()
        sync()
        acc.add([p.grad for p in ps], before, ps)
        acc.check(path.omega, f'{kind} step {s}')
        assert all(not torch.equal(p.detach(), b) for p, b in zip(ps, before))
    if kind == 'sgd_plain':
        for i, w in enumerate(path.omega):
            want = float(np.float32(lr)) * sum(g[i].astype(np.float64) ** 2 for g in grads)
            e = rel_l2(f64(w), want)
            print(f'plain SGD omega[{i}] vs lr * sum g^2: rel_l2 {e:.2e}')
            assert e < 1e-6, (i, e)
    assert set(opt.state_dict()) == {'state', 'param_groups'}
    if kind == 'adam':
        assert set(opt.state_dict()['state'][0]) == {'step', 'exp_avg', 'exp_avg_sq'}          # omega is not optimiser state


# ------------------------------------------------------------------------------------------------------------------ task 1, on / off

def _launched(C, monkeypatch):
    """Records the entry point of every HBM-bound launch."""
    names = []
    real = C.unet._hbm
    monkeypatch.setattr(C.unet, '_hbm', lambda family, nbytes, name, *args: (names.append((name, nbytes)), real(family, nbytes, name, *args))[1])
    return names


@pytest.mark.parametrize('kind,kw,exact', [('adam', {}, True), ('sgd', {'weight_decay': 0.0}, True), ('sgd', {}, False)],
                         ids=['adam', 'sgd_no_decay', 'sgd_default_decay'])
def test_task1_is_the_same_with_tracking_on_or_off(C, monkeypatch, kind, kw, exact):
    """UNet(21, 3, 8), 64 x 64, batch 4, three steps from the same seed with path_integral on and off: parameters and the optimiser's state
    bit-identical (Adam; SGD without weight decay) or within rel_l2 < 1e-6 (SGD with the default weight decay 1e-4, where nothing obliges
    grad * scale + wd * p to contract alike in the two instantiations).  omega is non-zero with tracking on; without it the step launches
    the untracked entry point."""
    nc, cd, B, size = 21, 8, 4, 64
    data = [(x.to(DEV), y.to(DEV)) for x, y in _batches(C, 9, 3, B, size, nc)]
    names = _launched(C, monkeypatch)
    runs = {}
    for on in (False, True):
        cfg = C.default_config(n_iters=100, lr=1e-3 if kind == 'adam' else 1e-2, num_classes=nc, conv_dim=cd, compute_dtype='fp32', stats_every=1,
                               optimizer=kind, path_integral=on, **kw)
        torch.manual_seed(6)
        tr = C.Trainer(data, cfg)
        del names[:]
        for x, y in data:
            tr.train_step(x, y)
        sync()
        steps = [(n, b) for n, b in names if n.startswith(('clamd_adam_step', 'clamd_sgd_step'))]
        numel = sum(p.numel() for p in tr.model.parameters())
        plain = 28 if kind == 'adam' else 20
        assert steps == [(f'clamd_{kind}_step' + ('_tracked' if on else ''), (plain + (8 if on else 0)) * numel)] * 3, steps
        assert (tr.path is not None) == on and (tr.optim._path is not None) == on
        runs[on] = tr
    off, on = runs[False], runs[True]
    keys = ('exp_avg', 'exp_avg_sq') if kind == 'adam' else ('momentum_buffer',)
    for (n, a), b in zip(off.model.named_parameters(), on.model.parameters()):
        pairs = [(a.detach(), b.detach())] + [(off.optim.state[a][k], on.optim.state[b][k]) for k in keys]
        for u, v in pairs:
            if exact:
                assert torch.equal(u.view(torch.int32), v.view(torch.int32)), n
            else:
                assert rel_l2(f64(v), f64(u)) < 1e-6, n
    assert all(bool(w.any()) for w in on.path.omega)
    assert torch.equal(on.path.flat, torch.cat([w.reshape(-1) for w in on.path.omega]))


# ------------------------------------------------------------------------------------------------------------------ two tasks

def _torch_si_two_task(ref, task1, task2, c, lr, xi):
    """The procedure composed from stock torch, on the model's own device and dtype: task 1 (plain hot loop, torch.optim.Adam) with omega
    accumulated by hand from parameter clones; at the boundary Omega = max(0, omega) / ((theta - theta_start)^2 + xi) and theta* = theta; task
    2 with every BatchNorm in eval mode and loss = CE + c * sum Omega (theta - theta*)^2 by autograd (c None: the pilot, no term).
    Returns the task-1 losses, per task-2 step (CE, penalty), Omega, the anchor, and the last raw gradient."""
    crit = nn.CrossEntropyLoss()
    opt = TC.make_optimizer(ref, lr=lr)
    ref.train()
    params = list(ref.parameters())
    start = [p.detach().clone() for p in params]
    omega = [torch.zeros_like(p) for p in params]
    losses1 = []
    for x, y in task1:
        before = [p.detach().clone() for p in params]
        losses1.append(float(TC.train_step(ref, opt, crit, x, y)[1].detach()))
        for w, p, b in zip(omega, params, before):
            w -= p.grad * (p.detach() - b)
    Om = [w.clamp_min(0) / ((p.detach() - s) ** 2 + xi) for w, p, s in zip(omega, params, start)]
    anchor = [p.detach().clone() for p in params]
    for mod in ref.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.eval()
    out, raw = [], None
    for x, y in task2:
        logits = ref(x)
        opt.zero_grad()
        ce = crit(logits, y)
        raw = torch.autograd.grad(ce, params, retain_graph=c is not None)
        if c is None:
            for p, g in zip(params, raw):
                p.grad = g
            pen = torch.zeros(())
        else:
            pen = c * sum((w * (p - a) ** 2).sum() for w, p, a in zip(Om, params, anchor))
            (ce + pen).backward()
        opt.step()
        out.append((float(ce.detach()), float(pen.detach())))
    return losses1, out, Om, anchor, raw


def _weighted_dist(params, importance, anchor):
    """sum Omega (theta - theta*)^2 in float64."""
    return sum(float((w.double() * (p.detach().double() - a.double()) ** 2).sum()) for p, w, a in zip(params, importance, anchor))


SPLIT = dict(nc=21, cd=8, B=4, size=64, n1=6, n2=6, lr=1e-3, c_old=11, xi=0.1)


def _split_tasks(C, device):
    s = SPLIT
    mk = lambda lo, hi, n: [(x.to(device), y.to(device)) for x, y in _batches(C, 9, n, s['B'], s['size'], s['nc'], class_lo=lo, class_hi=hi)]
    return mk(0, 11, s['n1']), mk(11, 21, s['n2'])


def test_si_two_task_split(C):
    """The synthetic split of test_ewc_two_task_split at its small shape, fp32: task 1 on classes 0-10 with tracking on,
    begin_task2(c_old=11, distill_lambda=0, si_lambda=c, freeze_bn=True), task 2 on classes 11-20 -- against the same procedure composed
    from stock torch on the same device.  omega after task 1 against the float64 accumulation from this path's own gradients and snapshots;
    the boundary against the float64 formula on those values; per task-2 step the penalty against the float64 sum over the weights before
    the update at rel=1e-4, and the loss within that test's tol_l = 2e-3.  On the CPU the stock-torch procedure in fp32 stays within
    TORCH_FP32_VS_FP64 of itself in float64 on every one of the twelve losses (measured there before this bound was applied), so tol_l
    measures the kernels and not the procedure.
    c is not tuned: a pilot task 2 without the term (same start) gives the last raw gradient g and the drift d; c = ||g|| / (2 ||Omega d||)
    makes the penalty gradient at that point as large as the loss gradient.  With it, sum Omega (theta - theta*)^2 after task 2 must be
    strictly smaller than in the pilot run."""
    s = SPLIT
    lr, xi, tol_l = s['lr'], s['xi'], 2e-3
    assert TORCH_FP32_VS_FP64 < tol_l
    task1, task2 = _split_tasks(C, DEV)
    torch.manual_seed(5)
    ref = TC.build_unet(s['nc'], 3, s['cd']).to(DEV)
    cfg = lambda **kw: C.default_config(n_iters=100, lr=lr, num_classes=s['nc'], conv_dim=s['cd'], compute_dtype='fp32', stats_every=1, **kw)
    tr = C.Trainer(task1, cfg(path_integral=True, si_xi=xi))
    tr.model.load_state_dict(ref.state_dict())
    params = list(tr.model.parameters())
    tr.path.restart(params)                                               # the weights were replaced: the task starts here
    start0 = [p.detach().clone() for p in params]
    acc = Accum(params)
    losses1 = []
    for x, y in task1:
        before = [p.detach().clone() for p in params]
        losses1.append(float(tr.train_step(x, y)[1].detach()))
        acc.add([p.grad for p in params], before, params)
    sync()
    acc.check(tr.path.omega, 'task 1')
    for a, b in zip(tr.path.start, start0):
        assert torch.equal(a, b)
    omega1 = [w.clone() for w in tr.path.omega]
    # ---- pilot: task 2 without the term, from a copy of the state after task 1; Omega from the path integral, which consolidate() leaves alone
    cons0 = tr.path.consolidate(tr.model.named_parameters())
    sync()
    assert all(torch.equal(a, b) for a, b in zip(tr.path.omega, omega1))
    pilot = C.Trainer(task1, cfg())
    pilot.model.load_state_dict({k: v.clone() for k, v in tr.model.state_dict().items()})
    pilot.optim.load_state_dict({'param_groups': tr.optim.state_dict()['param_groups'],
                                 'state': {i: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()}
                                           for i, st in tr.optim.state_dict()['state'].items()}})
    pilot.begin_task2(c_old=s['c_old'], distill_lambda=0, freeze_bn=True)
    assert pilot.consolidation is None and pilot.path is None
    for x, y in task2:
        pilot.train_step(x, y)
    sync()
    pp = list(pilot.model.parameters())
    g_norm = float(torch.cat([p.grad.reshape(-1) for p in pp]).double().norm())
    od_norm = float(torch.cat([(w * (p.detach() - a)).reshape(-1) for p, w, a in zip(pp, cons0.importance, cons0.anchor)]).double().norm())
    dist0 = _weighted_dist(pp, cons0.importance, cons0.anchor)
    assert od_norm > 0 and dist0 > 0
    c = g_norm / (2 * od_norm)
    print(f'si two-task: c = ||g|| / (2 ||Omega d||) = {g_norm:.3e} / (2 * {od_norm:.3e}) = {c:.3e}')
    del pilot
    # ---- the run with the term ----
    R1, R2, _, _, _ = _torch_si_two_task(ref, task1, task2, c, lr, xi)
    assert losses1 == pytest.approx(R1, rel=tol_l)
    want_imp = [path_ref.path_importance(np.zeros(tuple(p.shape)), f64(w), f64(p), f64(st), decay=1.0, xi=float(np.float32(xi)))
                for w, p, st in zip(omega1, params, start0)]
    tr.begin_task2(c_old=s['c_old'], distill_lambda=0, si_lambda=c, freeze_bn=True)
    sync()
    cons = tr.consolidation
    assert tr.distill is None and tr.ewc_lambda == 2 * c and cons.finished
    assert tr.model.training and all(not bn.training for bn in _bns(tr.model))
    for n, w, want in zip(cons.names, cons.importance, want_imp):
        _check_importance(f64(w), want, f'importance of {n}')
    for w0, w in zip(cons0.importance, cons.importance):
        assert torch.equal(w0, w)                                          # the same launch on the same values
    for a, st, p in zip(cons.anchor, tr.path.start, params):
        assert torch.equal(a, p.detach()) and torch.equal(st, p.detach())
    assert not tr.path.flat.any()
    assert tr.optim._importance[0].data_ptr() == cons.importance[0].data_ptr() and tr.optim._path[0].data_ptr() == tr.path.omega[0].data_ptr()
    acc2 = Accum(params)
    for i, (x, y) in enumerate(task2):
        before = [p.detach().clone() for p in params]
        _, loss = tr.train_step(x, y)
        acc2.add([p.grad for p in params], before, params)
        ce, rpen = R2[i]
        pen = float(tr.optim.consolidation_penalty())
        print(f'    task-2 step {i}: loss {float(loss.detach()):.6f} (torch {ce:.6f}), penalty {pen:.4e} (torch {rpen:.4e})')
        assert float(loss.detach()) == pytest.approx(ce, rel=tol_l), (i, float(loss.detach()), ce)
        want = c * sum(float((w.double() * (b.double() - a.double()) ** 2).sum()) for b, w, a in zip(before, cons.importance, cons.anchor))
        assert pen == pytest.approx(want, rel=1e-4, abs=1e-12), (i, pen, want)
        if i == 0:
            assert pen == 0.0
    sync()
    acc2.check(tr.path.omega, 'task 2')                                    # the gradient handed over, not the one with the pull added
    assert all(bool(w.any()) for w in tr.path.omega)
    dist1 = _weighted_dist(params, cons.importance, cons.anchor)
    print(f'    sum Omega (theta - theta*)^2 after task 2: {dist1:.4e} with the term, {dist0:.4e} without')
    assert dist1 < dist0, (dist1, dist0)


TORCH_FP32_VS_FP64 = 3.8e-5    # largest relative distance over the twelve losses, CPU, c from the float64 pilot (see test_si_two_task_split)


def _small_run(C, n1=3, n2=2, seed=3, **kw):
    """Task 1 on the small shape with tracking on."""
    s = SPLIT
    mk = lambda lo, hi, n, nc=s['nc']: [(x.to(DEV), y.to(DEV)) for x, y in _batches(C, 9, n, s['B'], s['size'], nc, class_lo=lo, class_hi=hi)]
    task1, task2 = mk(0, 11, n1), mk(11, 21, n2)
    cfg = C.default_config(n_iters=100, lr=1e-3, num_classes=s['nc'], conv_dim=s['cd'], compute_dtype='fp32', stats_every=1, path_integral=True, **kw)
    torch.manual_seed(seed)
    tr = C.Trainer(task1, cfg)
    for x, y in task1:
        tr.train_step(x, y)
    return tr, cfg, task1, task2, mk


def test_si_third_boundary_adds_to_the_previous_importance(C):
    """begin_task2 a second time (task 3): importance = previous + the new term (float64 formula, _check_importance), a new anchor, omega
    and start restarted; the first step from it reports a penalty of 0."""
    tr, _, _, task2, _ = _small_run(C)
    c = 50.0
    tr.begin_task2(c_old=11, distill_lambda=0, si_lambda=c, freeze_bn=True)
    first = tr.consolidation
    params = list(tr.model.parameters())
    for x, y in task2:
        tr.train_step(x, y)
    sync()
    assert float(tr.optim.consolidation_penalty()) > 0
    omega2, start2 = [w.clone() for w in tr.path.omega], [st.clone() for st in tr.path.start]
    prev = [w.clone() for w in first.importance]
    tr.begin_task2(c_old=21, distill_lambda=0, si_lambda=c)
    sync()
    merged = tr.consolidation
    assert merged is not first and tr.ewc_lambda == 2 * c
    added = False
    for n, w, w0, om, p, st in zip(merged.names, merged.importance, prev, omega2, params, start2):
        want = path_ref.path_importance(f64(w0), f64(om), f64(p), f64(st), decay=1.0, xi=float(np.float32(0.1)))
        _check_importance(f64(w), want, f'merged importance of {n}')
        added = added or bool((w > w0).any())
    assert added
    for a, st, p in zip(merged.anchor, tr.path.start, params):
        assert torch.equal(a, p.detach()) and torch.equal(st, p.detach())
    assert not tr.path.flat.any()
    assert tr.optim._importance[0].data_ptr() == merged.importance[0].data_ptr()
    tr.train_step(*task2[0])
    assert float(tr.optim.consolidation_penalty()) == 0.0                  # first step from the new anchor
    assert tr.path.flat.any()


@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_si_head_growth(C, kind):
    """begin_task2(c_old=11, si_lambda=c, new_classes=2): the head's omega and start have the grown shape, old rows keep their state (zeroed at
    the boundary), new rows have omega 0 and importance 0 and their initial value as start, and start follows the row that the head's
    initialisation rewrites; a train step runs and moves the new rows' omega."""
    tr, _, _, _, mk = _small_run(C, optimizer=kind)
    names = [n for n, _ in tr.model.named_parameters()]
    boundary = {n: p.detach().clone() for n, p in list(tr.model.named_parameters())[-2:]}
    tr.begin_task2(c_old=11, si_lambda=5.0, new_classes=2)
    sync()
    assert tr.cfg.num_classes == 23 and tr.path.names == names
    head = list(tr.model.named_parameters())[-2:]
    for n, p in head:
        i = names.index(n)
        w, st, imp = tr.path.omega[i], tr.path.start[i], tr.consolidation.importance[i]
        assert p.shape[0] == 23 and w.shape == p.shape and st.shape == p.shape and imp.shape == p.shape
        # head_init='background' moves the background row itself.  That is no step of the path: start follows it (by the same fp32
        # difference, an exact zero on the rows the growth left alone), the anchor stays at the boundary's weights
        moved = p.detach()[:21] - boundary[n]
        assert (bool(moved.any()) or p.dim() > 1) and not bool(moved[1:].any())      # the bias of the background row, nothing else
        assert not w.any() and torch.equal(st[:21], boundary[n] + moved) and torch.equal(st[21:], p.detach()[21:]) and not imp[21:].any()
        assert float((st - p.detach()).abs().max()) <= 2.0 ** -23 * float(p.detach().abs().max())
        assert torch.equal(tr.consolidation.anchor[i][:21], boundary[n]) and torch.equal(tr.consolidation.anchor[i][21:], p.detach()[21:])
        assert tr.optim._path[i].data_ptr() == w.data_ptr() and tr.optim._importance[i].data_ptr() == imp.data_ptr()
    assert sum(w.numel() for w in tr.path.omega) == tr.path.flat.numel() == sum(p.numel() for p in tr.model.parameters())
    assert any(bool(w.any()) for w in tr.consolidation.importance)
    x, y = mk(11, 23, 1, 23)[0]
    _, loss = tr.train_step(x, y)
    sync()
    assert np.isfinite(float(loss.detach()))
    for n, _ in head:
        w = tr.path.omega[names.index(n)]
        assert bool(w[21:].any()), f'{n}: the new rows were not tracked'
    assert np.isfinite(float(tr.optim.consolidation_penalty()))


def test_si_checkpoint_resumes_bit_identically(C, tmp_path):
    """save_network mid task 2 -> fresh Trainer(path_integral=True) -> load_network -> the next step's loss, parameters, penalty and omega
    are bit-identical to the uninterrupted run; the file's keys are the reference's four plus consolidation_state and path_state."""
    tr, cfg, task1, task2, _ = _small_run(C, seed=4, si_xi=0.05)
    tr.begin_task2(c_old=11, distill_lambda=0, si_lambda=40.0, freeze_bn=True)
    tr.train_step(*task2[0])
    path = tr.save_network('G', 7, 7, str(tmp_path))
    ck = torch.load(path, map_location='cpu', weights_only=False)
    assert set(ck) == {'epoch', 'model_state', 'optimizer_state', 'scheduler_state', 'consolidation_state', 'path_state'}
    assert set(ck['path_state']) == {'omega', 'start', 'xi'} and ck['path_state']['xi'] == 0.05 and ck['consolidation_state']['lambda'] == 80.0
    assert list(ck['path_state']['omega']) == [n for n, _ in tr.model.named_parameters()]
    ref = TC.build_unet(21, 3, SPLIT['cd'])
    ref.load_state_dict(ck['model_state'])                                 # as the reference's load_network does
    TC.make_optimizer(ref).load_state_dict(ck['optimizer_state'])
    _, loss_a = tr.train_step(*task2[1])
    sync()
    cfg2 = C.default_config(**{**vars(cfg), 'si_xi': 0.1})
    tr2 = C.Trainer(task1, cfg2)
    assert tr2.load_network('G', 7, str(tmp_path)) and tr2.ewc_lambda == 80.0 and tr2.path.xi == 0.05
    for bn in _bns(tr2.model):                                             # module modes are not checkpoint state
        bn.eval()
    _, loss_b = tr2.train_step(*task2[1])
    sync()
    assert float(loss_a.detach()) == float(loss_b.detach())
    assert torch.equal(tr.optim.consolidation_penalty(), tr2.optim.consolidation_penalty()) and float(tr.optim.consolidation_penalty()) > 0
    for (n, a), b in zip(tr.model.named_parameters(), tr2.model.parameters()):
        assert torch.equal(a.detach(), b.detach()), n
    assert torch.equal(tr.path.flat.view(torch.int32), tr2.path.flat.view(torch.int32)) and tr.path.flat.any()
    for a, b in zip(tr.path.start, tr2.path.start):
        assert torch.equal(a, b)
