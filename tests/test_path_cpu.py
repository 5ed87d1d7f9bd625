"""CPU-only tests of Synaptic Intelligence's host side: the float64 restatement (tests/path_ref.py) pinned against stock torch, the new
entry points validate before any launch, set_path_integral validates its arguments, PathIntegral.state_dict round-trips by parameter
name, and the trainer's si_lambda and 'path_state' handling.  No kernel is launched here."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import path_ref


@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    return C


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_restatement_matches_stock_torch_and_telescopes(kind):
    """Three steps of torch.optim.Adam / torch.optim.SGD (momentum, Nesterov, weight decay) on tiny float64 tensors, omega accumulated by
    hand from parameter clones: path_ref agrees to 1e-12 relative, and the per-step differences sum to theta_end - theta_start."""
    g = torch.Generator().manual_seed(3)
    shapes = [(7,), (3, 4)]
    ps = [torch.nn.Parameter(torch.randn(s, generator=g, dtype=torch.float64)) for s in shapes]
    grads = [[torch.randn(s, generator=g, dtype=torch.float64) for s in shapes] for _ in range(3)]
    if kind == 'adam':
        opt = torch.optim.Adam(ps, lr=1e-2, betas=(0.5, 0.99), eps=1e-8)
    else:
        opt = torch.optim.SGD(ps, lr=0.05, momentum=0.9, nesterov=True, weight_decay=0.05)
    start = [p.detach().clone() for p in ps]
    omega = [torch.zeros(s, dtype=torch.float64) for s in shapes]
    moved = [torch.zeros(s, dtype=torch.float64) for s in shapes]
    rp = [p.detach().numpy().copy() for p in ps]
    rm = [np.zeros(s) for s in shapes]
    rv = [np.zeros(s) for s in shapes]
    rb = [np.zeros(s) for s in shapes]
    ro = [np.zeros(s) for s in shapes]
    for s, gs in enumerate(grads, 1):
        before = [p.detach().clone() for p in ps]
        for p, x in zip(ps, gs):
            p.grad = x.clone()
        opt.step()
        for i, (p, b, x) in enumerate(zip(ps, before, gs)):
            omega[i] -= x * (p.detach() - b)
            moved[i] += p.detach() - b
            if kind == 'adam':
                r = path_ref.adam_step_tracked(rp[i], x.numpy(), rm[i], rv[i], ro[i], s, lr=1e-2, beta1=0.5, beta2=0.99, eps=1e-8)
                rp[i], rm[i], rv[i], ro[i] = r['p'], r['m'], r['v'], r['omega']
            else:
                r = path_ref.sgd_step_tracked(rp[i], x.numpy(), rb[i], ro[i], lr=0.05, momentum=0.9, nesterov=True, weight_decay=0.05)
                rp[i], rb[i], ro[i] = r['p'], r['buf'], r['omega']
            assert _rel(rp[i], p.detach().numpy()) <= 1e-12, (kind, s, i)
            assert _rel(ro[i], omega[i].numpy()) <= 1e-12, (kind, s, i)
    for i, p in enumerate(ps):
        assert _rel(moved[i].numpy(), (p.detach() - start[i]).numpy()) <= 1e-12          # the telescoping identity
        assert np.abs(ro[i]).max() > 0
        if kind == 'adam':
            assert _rel(rm[i], opt.state[p]['exp_avg'].numpy()) <= 1e-12 and _rel(rv[i], opt.state[p]['exp_avg_sq'].numpy()) <= 1e-12
        else:
            assert _rel(rb[i], opt.state[p]['momentum_buffer'].numpy()) <= 1e-12


def test_restatement_takes_the_gradient_before_the_pulls_and_the_boundary_formula():
    """The pulls and the gradient scale by hand on one element; the boundary formula on its four kinds of element."""
    r = path_ref.sgd_step_tracked([1.0], [2.0], None, [0.5], [0.0], [3.0], lr=0.1, grad_scale=0.5, weight_decay=0.2, l2_lambda=0.25,
                                  ewc_lambda=2.0)
    u = 0.5 * 2.0 + 0.2 * 1.0 + 2 * 0.25 * 1.0 + 2.0 * 3.0 * 1.0
    assert r['p'][0] == pytest.approx(1.0 - 0.1 * u, rel=1e-15)
    assert r['omega'][0] == pytest.approx(0.5 + (0.5 * 2.0) * (0.1 * u), rel=1e-15)       # g_task = 1.0, not u
    got = path_ref.path_importance([1.0, 1.0, 0.0, 2.0], [-3.0, 0.0, 4.0, 1.0], [1.0, 2.0, 3.0, 5.0], [0.0, 2.0, 1.0, 5.0], decay=0.5, xi=0.1)
    np.testing.assert_allclose(got, [0.5, 0.5, 4.0 / 4.1, 1.0 + 1.0 / 0.1], rtol=1e-15)


def test_path_entry_points_reject_bad_arguments_before_any_launch(C):
    """Style of test_ewc_entry_points_reject_bad_arguments_before_any_launch: every call fails validation on the host (the non-null
    pointers are host memory that nothing dereferences), returns a negative status, and clamd_last_error() names the problem."""
    lib = C._lib.load()
    call = C._lib.call
    buf = ctypes.create_string_buffer(256)
    a = ctypes.addressof(buf)
    assert lib.clamd_sizeof_path_tensor() == 40 and lib.clamd_sizeof_adam_tensor() == 48 and lib.clamd_sizeof_sgd_tensor() == 48
    adam, sgd, imp = 'clamd_adam_step_tracked', 'clamd_sgd_step_tracked', 'clamd_path_importance'
    cases = [
        ('no chunks', adam, (a, None, a, a, 0, a, a, a, None, None, None)),
        ('no chunks', adam, (a, None, a, a, -2, a, a, a, None, None, None)),
        ('null tensor or chunk table', adam, (None, None, a, a, 4, a, a, a, None, None, None)),
        ('null tensor or chunk table', adam, (a, None, a, None, 4, a, a, a, None, None, None)),
        ('null path table', adam, (a, None, None, a, 4, a, a, a, None, None, None)),
        ('null path table', adam, (a, a, None, a, 4, a, a, a, a, None, None)),
        ('null hyper / step / derived', adam, (a, None, a, a, 4, None, a, a, None, None, None)),
        ('null hyper / step / derived', adam, (a, None, a, a, 4, a, None, a, None, None, None)),
        ('null hyper / step / derived', adam, (a, None, a, a, 4, a, a, None, None, None, None)),
        ('an importance table needs a penalty buffer', adam, (a, a, a, a, 4, a, a, a, None, None, None)),
        ('a consolidation penalty buffer without an importance table', adam, (a, None, a, a, 4, a, a, a, a, None, None)),
        ('no chunks', sgd, (a, None, a, a, 0, a, None, None, None)),
        ('null tensor or chunk table', sgd, (None, None, a, a, 4, a, None, None, None)),
        ('null tensor or chunk table', sgd, (a, None, a, None, 4, a, None, None, None)),
        ('null path table', sgd, (a, None, None, a, 4, a, None, None, None)),
        ('null hyper buffer', sgd, (a, None, a, a, 4, None, None, None, None)),
        ('an importance table needs a penalty buffer', sgd, (a, a, a, a, 4, a, None, None, None)),
        ('a consolidation penalty buffer without an importance table', sgd, (a, None, a, a, 4, a, a, None, None)),
        ('no chunks', imp, (a, a, 0, 1.0, 0.1, None)),
        ('null tensor or chunk table', imp, (None, a, 4, 1.0, 0.1, None)),
        ('null tensor or chunk table', imp, (a, None, 4, 1.0, 0.1, None)),
        ('xi must be finite and > 0', imp, (a, a, 4, 1.0, 0.0, None)),
        ('xi must be finite and > 0', imp, (a, a, 4, 1.0, -0.1, None)),
        ('xi must be finite and > 0', imp, (a, a, 4, 1.0, math.nan, None)),
        ('xi must be finite and > 0', imp, (a, a, 4, 1.0, math.inf, None)),
        ('xi must be finite and > 0', imp, (a, a, 4, 1.0, 1e-60, None)),            # zero as fp32
        ('decay must be finite and >= 0', imp, (a, a, 4, -0.5, 0.1, None)),
        ('decay must be finite and >= 0', imp, (a, a, 4, math.nan, 0.1, None)),
        ('decay must be finite and >= 0', imp, (a, a, 4, math.inf, 0.1, None)),
    ]
    for needle, name, args in cases:
        with pytest.raises(RuntimeError) as e:
            call(name, *args)
        assert needle in str(e.value), (name, str(e.value))
        assert needle in lib.clamd_last_error().decode()
        assert name[len('clamd_'):] in str(e.value)
    assert bytes(buf) == bytes(256)                    # untouched


def _params(dev, shapes=((3, 2), (5,))):
    return [torch.nn.Parameter(torch.zeros(*s, device=dev)) for s in shapes]


@pytest.mark.parametrize('opt_name', ['FusedAdam', 'FusedSGD'])
def test_set_path_integral_validates_count_shape_dtype_and_device(C, opt_name):
    # 'meta' stands in for the GPU: a device that is not the CPU, without needing one
    make = (lambda ps: C.FusedAdam(ps, lr=1e-3, betas=[0.5, 0.99])) if opt_name == 'FusedAdam' else (lambda ps: C.FusedSGD(ps, lr=1e-3, momentum=0.9))
    ps = _params('meta')
    opt = make(ps)
    like = lambda dev: [torch.zeros(p.shape, device=dev) for p in ps]
    assert opt._path is None
    with pytest.raises(ValueError, match='2 parameters, 1 path tensors'):
        opt.set_path_integral(like('meta')[:1])
    bad = like('meta'); bad[1] = torch.zeros(4, device='meta')
    with pytest.raises(ValueError, match='shape'):
        opt.set_path_integral(bad)
    half = like('meta'); half[0] = half[0].half()
    with pytest.raises(ValueError, match='fp32'):
        opt.set_path_integral(half)
    strided = like('meta'); strided[0] = torch.zeros(2, 3, device='meta').t()
    with pytest.raises(ValueError, match='contiguous'):
        opt.set_path_integral(strided)
    cpu_one = like('meta'); cpu_one[0] = torch.zeros(ps[0].shape)
    with pytest.raises(ValueError, match='path on cpu'):
        opt.set_path_integral(cpu_one)
    assert opt._path is None                                               # nothing was installed by the failed calls
    opt.set_path_integral(like('meta'))
    assert len(opt._path) == 2
    opt.set_path_integral(None)
    assert opt._path is None
    # composes with both anchor terms in any order; omega is not optimiser state
    ps = _params('cpu')
    opt = make(ps)
    snap = [torch.full(p.shape, 1.0) for p in ps]
    imp = [torch.ones(p.shape) for p in ps]
    om = [torch.zeros(p.shape) for p in ps]
    opt.set_path_integral(om)
    opt.set_consolidation(snap, imp, 0.5)
    opt.set_l2_anchor(snap, 0.1)
    assert opt._path[0].data_ptr() == om[0].data_ptr() and opt._importance is not None and opt._l2_on
    opt.set_consolidation(None, None, 0.0)
    opt.set_l2_anchor(None, 0.0)
    assert opt._path is not None and opt._anchor is None
    plain = make(_params('cpu'))
    assert opt.state_dict() == plain.state_dict() and set(opt.state_dict()) == {'state', 'param_groups'}
    # head growth: replace_params grows the omega entries as it grows the importance -- old rows kept, new rows zero
    om[0].fill_(2.0)
    grown = torch.nn.Parameter(torch.ones(5, 2))
    opt.replace_params({ps[0]: grown})
    assert opt._path[0].shape == (5, 2) and torch.equal(opt._path[0][:3], torch.full((3, 2), 2.0)) and not opt._path[0][3:].any()
    assert opt._path[1].data_ptr() == om[1].data_ptr()
    ps[0] = grown
    om[0].zero_()
    for p in ps:
        p.grad = torch.zeros_like(p)
    with pytest.raises(RuntimeError):
        opt.step()                                                         # CPU parameters: fails loudly, no fallback
    assert not any(w.any() for w in om)


def test_path_integral_state_dict_round_trips_by_name(C):
    g = torch.Generator().manual_seed(0)
    named = [('b.weight', torch.randn(3, 2, generator=g)), ('a.bias', torch.randn(5, generator=g))]
    c = C.PathIntegral(named, xi=0.25)
    assert [tuple(w.shape) for w in c.omega] == [(3, 2), (5,)] and c.flat.numel() == 11 and not c.flat.any()
    assert all(w.data_ptr() == c.flat.data_ptr() + 4 * o for w, o in zip(c.omega, (0, 6)))            # views of ONE flat buffer
    assert all(torch.equal(a, p) and a.data_ptr() != p.data_ptr() for a, (_, p) in zip(c.start, named))
    c.flat.copy_(torch.randn(11, generator=g))
    sd = c.state_dict()
    assert set(sd) == {'omega', 'start', 'xi'} and list(sd['omega']) == ['b.weight', 'a.bias'] and sd['xi'] == 0.25
    saved = {'omega': {k: v.clone() for k, v in reversed(list(sd['omega'].items()))},                 # another key order
             'start': {k: v.clone() for k, v in reversed(list(sd['start'].items()))}, 'xi': 0.25}
    d = C.PathIntegral([(n, torch.zeros_like(p)) for n, p in named])
    assert d.xi == 0.1
    d.load_state_dict(saved)
    assert d.xi == 0.25
    for a, b in zip(c.omega + c.start, d.omega + d.start):
        assert torch.equal(a, b)
    with pytest.raises(KeyError, match='missing'):
        d.load_state_dict({**saved, 'omega': {'b.weight': saved['omega']['b.weight']}})
    with pytest.raises(ValueError, match='shape'):
        d.load_state_dict({**saved, 'start': {'b.weight': torch.zeros(2, 3), 'a.bias': torch.zeros(5)}})
    for a, b in zip(c.omega + c.start, d.omega + d.start):
        assert torch.equal(a, b)                                                                       # the failed loads changed nothing
    for xi in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match='xi'):
            C.PathIntegral(named, xi=xi)
    # restart and head growth on the host
    d.restart([p + 1 for _, p in named])
    assert not d.flat.any() and torch.equal(d.start[0], named[0][1] + 1)
    d.flat.fill_(2.0)
    new = torch.full((5, 2), 7.0)
    d.grow('b.weight', new)
    assert d.shapes[0] == (5, 2) and d.flat.numel() == 15 and torch.equal(d.omega[0][:3], torch.full((3, 2), 2.0)) and not d.omega[0][3:].any()
    assert torch.equal(d.start[0][:3], named[0][1] + 1) and torch.equal(d.start[0][3:], new[3:]) and torch.equal(d.omega[1], torch.full((5,), 2.0))
    # with the old parameter: start follows what the growth did to an old row; a 0-dim tensor beside the grown one is laid out again too
    e = C.PathIntegral([('w', torch.tensor([1.0, 2.0])), ('s', torch.tensor(3.0))])
    e.flat.copy_(torch.tensor([0.5, 0.25, 0.125]))
    e.grow('w', torch.tensor([1.5, 2.0, 9.0]), torch.tensor([1.0, 2.0]))
    assert torch.equal(e.start[0], torch.tensor([1.5, 2.0, 9.0])) and torch.equal(e.flat, torch.tensor([0.5, 0.25, 0.0, 0.125]))
    assert e.omega[1].shape == () and float(e.omega[1]) == 0.125 and float(e.start[1]) == 3.0
    with pytest.raises(ValueError, match='old_param'):
        e.grow('w', torch.zeros(4), torch.zeros(2))
    k = C.Consolidation([('w', torch.tensor([1.0, 2.0])), ('s', torch.tensor(3.0))])
    k.flat.copy_(torch.tensor([0.5, 0.25, 0.125]))
    k.grow('w', torch.tensor([1.5, 2.0, 9.0]))
    assert torch.equal(k.flat, torch.tensor([0.5, 0.25, 0.0, 0.125])) and torch.equal(k.anchor[0], torch.tensor([1.0, 2.0, 9.0]))
    with pytest.raises(ValueError, match='growth'):
        d.grow('a.bias', torch.zeros(5))
    with pytest.raises(KeyError):
        d.grow('nope', torch.zeros(9))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        C.PathIntegral(named).consolidate(named)


def test_trainer_si_lambda_checks_and_checkpoints(C, tmp_path):
    """si_lambda needs cfg.path_integral and is refused with ewc_lambda, both before anything is changed; a checkpoint with the reference's
    four keys only still loads and leaves self.path as built; one with 'path_state' restores omega, start and xi by name."""
    cfg = C.default_config(n_iters=10, num_classes=3, conv_dim=4)
    assert cfg.path_integral is False and cfg.si_xi == 0.1
    tr = C.Trainer([], cfg, device='cpu')
    assert tr.path is None and tr.optim._path is None
    with pytest.raises(ValueError, match='path_integral'):
        tr.begin_task2(2, si_lambda=1.0)
    assert tr.old_model is None and tr.consolidation is None and tr.ewc_lambda == 0.0
    for kind in ('adam', 'sgd'):
        cfg_si = C.default_config(n_iters=10, num_classes=3, conv_dim=4, path_integral=True, si_xi=0.5, optimizer=kind)
        ts = C.Trainer([], cfg_si, device='cpu')
        names = [n for n, _ in ts.model.named_parameters()]
        assert isinstance(ts.path, C.PathIntegral) and ts.path.xi == 0.5 and ts.path.names == names
        assert all(w.data_ptr() == v.data_ptr() for w, v in zip(ts.optim._path, ts.path.omega))
        assert all(torch.equal(s, p.detach()) for s, p in zip(ts.path.start, ts.model.parameters()))
        with pytest.raises(ValueError, match='Riemannian Walk'):
            ts.begin_task2(2, si_lambda=1.0, ewc_lambda=1.0)
        with pytest.raises(ValueError, match='si_lambda'):
            ts.begin_task2(2, si_lambda=-1.0)
        assert ts.old_model is None and ts.consolidation is None and ts.ewc_lambda == 0.0
    ck = {'epoch': 4, 'model_state': tr.model.state_dict(), 'optimizer_state': tr.optim.state_dict(),
          'scheduler_state': tr.scheduler.state_dict()}
    torch.save(ck, os.path.join(tmp_path, '3_net_G.pth'))
    cfg_si = C.default_config(n_iters=10, num_classes=3, conv_dim=4, path_integral=True)
    tr2 = C.Trainer([], cfg_si, device='cpu')
    built = tr2.path
    built.flat.fill_(3.0)
    assert tr2.load_network('G', 3, str(tmp_path)) is True
    assert tr2.path is built and bool((built.flat == 3.0).all()) and tr2.optim._path[0].data_ptr() == built.omega[0].data_ptr()
    tr3 = C.Trainer([], cfg, device='cpu')
    assert tr3.load_network('G', 3, str(tmp_path)) is True and tr3.path is None and tr3.optim._path is None
    g = torch.Generator().manual_seed(1)
    ck['path_state'] = {'omega': {n: torch.randn(p.shape, generator=g) for n, p in tr.model.named_parameters()},
                        'start': {n: torch.randn(p.shape, generator=g) for n, p in tr.model.named_parameters()}, 'xi': 0.3}
    torch.save(ck, os.path.join(tmp_path, '4_net_G.pth'))
    for t in (tr2, tr3):                               # a trainer with a path integral, and one without: it starts tracking
        assert t.load_network('G', 4, str(tmp_path)) is True
        assert t.path.xi == 0.3
        for n, w, s in zip(t.path.names, t.path.omega, t.path.start):
            assert torch.equal(w, ck['path_state']['omega'][n]) and torch.equal(s, ck['path_state']['start'][n])
        assert all(w.data_ptr() == v.data_ptr() for w, v in zip(t.optim._path, t.path.omega))
