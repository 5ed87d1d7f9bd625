"""CPU-only tests of the fused SGD optimiser's host side: the float64 restatement against torch.optim.SGD, the C ABI's validation before any
launch, FusedSGD's constructor, state layout, checkpoint interchange, head growth and anchor checks, the trainer's two learning-rate
schedules and the cross-optimiser checkpoint check.  No kernel is launched here."""
import ctypes
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import sgd_ref


@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    return C


@pytest.mark.parametrize('mu,nesterov', [(0.0, False), (0.9, False), (0.9, True)])
@pytest.mark.parametrize('wd', [0.0, 0.05])
def test_restatement_equals_torch_sgd_in_float64(mu, nesterov, wd):
    rng = np.random.default_rng(3)
    p0 = rng.standard_normal(301)
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.SGD([p], lr=0.07, momentum=mu, nesterov=nesterov, weight_decay=wd)
    rp, rbuf = p0.copy(), (np.zeros_like(p0) if mu > 0 else None)
    for _ in range(4):
        g = rng.standard_normal(301)
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        r = sgd_ref.sgd_step(rp, g, rbuf, lr=0.07, momentum=mu, weight_decay=wd, nesterov=nesterov)
        rp, rbuf = r['p'], r['buf']
        np.testing.assert_allclose(rp, p.detach().numpy(), rtol=1e-12, atol=0)
        if mu > 0:
            np.testing.assert_allclose(rbuf, opt.state[p]['momentum_buffer'].numpy(), rtol=1e-12, atol=0)


def test_restatement_anchor_terms_are_the_gradient_of_the_penalties():
    """Torch defines no anchor terms; the formula does: the pulls are the gradients of l2 * sum d^2 and (ewc / 2) * sum omega d^2."""
    rng = np.random.default_rng(4)
    p, old, om, g = rng.standard_normal(50), rng.standard_normal(50), rng.random(50) * 2, rng.standard_normal(50)
    r = sgd_ref.sgd_step(p, g, None, old, om, lr=1.0, l2_lambda=0.3, ewc_lambda=0.7)
    np.testing.assert_allclose(p - r['p'], g + 2 * 0.3 * (p - old) + 0.7 * om * (p - old), rtol=1e-13)
    assert r['l2'] == pytest.approx(((p - old) ** 2).sum()) and r['ewc'] == pytest.approx((om * (p - old) ** 2).sum())


def test_sgd_entry_point_rejects_bad_arguments_before_any_launch(C):
    """Pattern of test_ewc_cpu.py: every call fails validation on the host (the non-null pointers are host memory that nothing
    dereferences), returns a negative status, and clamd_last_error() names the problem."""
    lib = C._lib.load()
    call = C._lib.call
    buf = ctypes.create_string_buffer(256)
    a = ctypes.addressof(buf)
    assert lib.clamd_sizeof_sgd_tensor() == 48
    cases = [
        ('no chunks', (a, None, a, 0, a, None, None, None)),
        ('no chunks', (a, None, a, -2, a, None, None, None)),
        ('null tensor or chunk table', (None, None, a, 4, a, None, None, None)),
        ('null tensor or chunk table', (a, None, None, 4, a, None, None, None)),
        ('null hyper', (a, None, a, 4, None, None, None, None)),
        ('importance table needs a penalty buffer', (a, a, a, 4, a, None, None, None)),
        ('importance table needs a penalty buffer', (a, a, a, 4, a, None, a, None)),
        ('penalty buffer without an importance table', (a, None, a, 4, a, a, None, None)),
    ]
    for needle, args in cases:
        with pytest.raises(RuntimeError) as e:
            call('clamd_sgd_step', *args)
        assert needle in str(e.value), str(e.value)
        assert needle in lib.clamd_last_error().decode()
    assert bytes(buf) == bytes(256)                    # untouched


def _params(dev, shapes=((3, 2), (5,))):
    return [torch.nn.Parameter(torch.zeros(*s, device=dev)) for s in shapes]


def test_constructor_errors(C):
    for dev in ('meta', 'cpu'):
        ps = _params(dev)
        for kw in (dict(dampening=0.1), dict(nesterov=True), dict(nesterov=True, momentum=0.0), dict(lr=-1.0), dict(momentum=-0.1),
                   dict(weight_decay=-1e-4)):
            with pytest.raises(ValueError):
                C.FusedSGD(ps, **{'lr': 0.1, **kw})
        with pytest.raises(ValueError, match='single parameter group'):
            C.FusedSGD([{'params': ps[:1]}, {'params': ps[1:]}], lr=0.1)
        with pytest.raises(ValueError, match='no_decay'):
            C.FusedSGD(ps, lr=0.1, no_decay=[torch.nn.Parameter(torch.zeros(2, device=dev))])
        opt = C.FusedSGD(ps, lr=0.1, momentum=0.9, nesterov=True, weight_decay=1e-4, no_decay=ps[1:])
        assert opt._no_decay == {id(ps[1])}
    assert 'FusedSGD' in C.__all__


def test_state_layout_is_torch_sgds(C):
    ps = _params('cpu')
    for kw in (dict(momentum=0.9, nesterov=True, weight_decay=1e-4), dict()):
        ours = C.FusedSGD(ps, lr=0.1, **kw)
        theirs = torch.optim.SGD(ps, lr=0.1, **kw)
        a, b = ours.state_dict(), theirs.state_dict()
        assert set(a) == set(b) == {'state', 'param_groups'}
        assert set(a['param_groups'][0]) == set(b['param_groups'][0])
        assert set(ours.defaults) == set(theirs.defaults)
        assert a['param_groups'][0]['params'] == b['param_groups'][0]['params']
        assert a['state'] == {} == b['state']                          # before the first step
    # after a step torch holds one 'momentum_buffer' per parameter; FusedSGD's state has the same keys once its buffers exist
    theirs = torch.optim.SGD(ps, lr=0.1, momentum=0.9)
    for p in ps:
        p.grad = torch.ones_like(p)
    theirs.step()
    ours = C.FusedSGD(ps, lr=0.1, momentum=0.9)
    ours.load_state_dict(theirs.state_dict())
    a, b = ours.state_dict(), theirs.state_dict()
    assert {k: set(v) for k, v in a['state'].items()} == {k: set(v) for k, v in b['state'].items()} == {0: {'momentum_buffer'}, 1: {'momentum_buffer'}}


def test_load_state_dict_round_trips_with_torch_sgd(C):
    ps = _params('cpu')
    theirs = torch.optim.SGD(ps, lr=0.05, momentum=0.8, nesterov=True, weight_decay=0.01)
    for p in ps:
        p.grad = torch.arange(p.numel(), dtype=torch.float32).view_as(p)
    theirs.step()
    sd = theirs.state_dict()
    ours = C.FusedSGD(_params('cpu'), lr=0.1, momentum=0.9)
    ours._table, ours._hyper_host = ['stale'], ('stale',)
    ours.load_state_dict(sd)
    assert ours._table is None and ours._hyper_host is None             # device tables and hyper-parameters are rebuilt at the next step
    g = ours.param_groups[0]
    assert (g['lr'], g['momentum'], g['nesterov'], g['weight_decay']) == (0.05, 0.8, True, 0.01)
    back = ours.state_dict()
    for i in (0, 1):
        assert torch.equal(back['state'][i]['momentum_buffer'], sd['state'][i]['momentum_buffer'])
    again = torch.optim.SGD(_params('cpu'), lr=1.0)
    again.load_state_dict(back)                                        # and back into torch
    assert torch.equal(again.state[again.param_groups[0]['params'][1]]['momentum_buffer'], sd['state'][1]['momentum_buffer'])
    assert again.param_groups[0]['momentum'] == 0.8
    # torch before its first step: an empty state loads and the buffers start at zero at the next step
    fresh = C.FusedSGD(_params('cpu'), lr=0.1, momentum=0.9)
    fresh.load_state_dict(torch.optim.SGD(_params('cpu'), lr=0.1, momentum=0.9).state_dict())
    assert fresh.state_dict()['state'] == {}
    for p in fresh.param_groups[0]['params']:
        p.grad = torch.zeros_like(p)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fresh.step()
    for p in fresh.param_groups[0]['params']:
        p.grad = None
    with pytest.raises(RuntimeError, match='must have a gradient'):
        fresh.step()


def test_replace_params_keeps_rows_zeroes_new_ones_and_carries_no_decay(C):
    w, b = torch.nn.Parameter(torch.randn(3, 2)), torch.nn.Parameter(torch.randn(3))
    other = torch.nn.Parameter(torch.randn(4))
    opt = C.FusedSGD([w, b, other], lr=0.1, momentum=0.9, weight_decay=1e-4, no_decay=[b])
    mw, mb = torch.randn(3, 2), torch.randn(3)
    opt.state[w], opt.state[b] = {'momentum_buffer': mw.clone()}, {'momentum_buffer': mb.clone()}
    snap = [p.detach().clone() for p in (w, b, other)]
    opt.set_consolidation(snap, [torch.ones_like(p) for p in snap], 0.5)
    opt.set_l2_anchor(snap, 0.1)
    nw, nb = torch.nn.Parameter(torch.randn(5, 2)), torch.nn.Parameter(torch.randn(5))
    opt._table = ['stale']
    opt.replace_params({w: nw, b: nb})
    ps = opt.param_groups[0]['params']
    assert ps[0] is nw and ps[1] is nb and ps[2] is other and opt._table is None
    assert w not in opt.state and b not in opt.state
    assert torch.equal(opt.state[nw]['momentum_buffer'][:3], mw) and not opt.state[nw]['momentum_buffer'][3:].any()
    assert torch.equal(opt.state[nb]['momentum_buffer'][:3], mb) and not opt.state[nb]['momentum_buffer'][3:].any()
    assert opt._no_decay == {id(nb)}
    assert torch.equal(opt._anchor[0][:3], snap[0]) and torch.equal(opt._anchor[0][3:], nw.detach()[3:])
    assert torch.equal(opt._importance[1][:3], torch.ones(3)) and not opt._importance[1][3:].any()
    # what FusedAdam.replace_params rejects
    with pytest.raises(ValueError, match='not a parameter of this optimiser'):
        opt.replace_params({w: nw})
    with pytest.raises(ValueError, match='not growth along dim 0'):
        opt.replace_params({nw: torch.nn.Parameter(torch.randn(5, 2))})
    with pytest.raises(ValueError, match='not growth along dim 0'):
        opt.replace_params({nw: torch.nn.Parameter(torch.randn(6, 3))})
    with pytest.raises(ValueError, match='device and dtype'):
        opt.replace_params({nw: torch.nn.Parameter(torch.randn(6, 2).double())})
    # before the first step there is no state to carry
    opt2 = C.FusedSGD([w], lr=0.1, momentum=0.9)
    opt2.replace_params({w: nw})
    assert opt2.state_dict()['state'] == {}


def test_set_consolidation_and_l2_anchor_make_fused_adams_checks(C):
    """The checks of test_ewc_cpu.test_set_consolidation_validates_count_shape_device_and_anchor, on FusedSGD."""
    ps = _params('meta')
    opt = C.FusedSGD(ps, lr=0.1, momentum=0.9)
    like = lambda dev: [torch.zeros(p.shape, device=dev) for p in ps]
    opt.set_consolidation(like('meta'), like('meta'), 0.5)
    assert opt._ewc_lambda == 0.5 and len(opt._importance) == 2
    opt.set_consolidation(None, None, 0.0)
    assert opt._importance is None and opt._anchor is None and opt._ewc_lambda == 0.0
    with pytest.raises(ValueError, match='2 parameters, 1 anchors'):
        opt.set_consolidation(like('meta')[:1], like('meta'), 0.5)
    with pytest.raises(ValueError, match='3 importance tensors'):
        opt.set_consolidation(like('meta'), like('meta') + like('meta')[:1], 0.5)
    bad = like('meta'); bad[1] = torch.zeros(4, device='meta')
    with pytest.raises(ValueError, match='shape'):
        opt.set_consolidation(like('meta'), bad, 0.5)
    with pytest.raises(ValueError, match='shape'):
        opt.set_consolidation(bad, like('meta'), 0.5)
    cpu_one = like('meta'); cpu_one[0] = torch.zeros(ps[0].shape)
    with pytest.raises(ValueError, match='importance on cpu'):
        opt.set_consolidation(like('meta'), cpu_one, 0.5)
    with pytest.raises(ValueError, match='anchor on cpu'):
        opt.set_consolidation(cpu_one, like('meta'), 0.5)
    half = like('meta'); half[0] = half[0].half()
    with pytest.raises(ValueError, match='fp32'):
        opt.set_consolidation(like('meta'), half, 0.5)
    with pytest.raises(ValueError, match='FusedSGD.set_consolidation: lam'):
        opt.set_consolidation(like('meta'), like('meta'), -1.0)
    assert opt._importance is None
    ps = _params('cpu')
    opt = C.FusedSGD(ps, lr=0.1, momentum=0.9)
    snap = [torch.full(p.shape, 1.0) for p in ps]
    other = [torch.full(p.shape, 2.0) for p in ps]
    imp = [torch.ones(p.shape) for p in ps]
    opt.set_l2_anchor(snap, 0.1)
    assert opt.l2_lambda == 0.1
    with pytest.raises(ValueError, match='same snapshot'):
        opt.set_consolidation(other, imp, 0.5)
    assert opt._importance is None
    l2_ptr = opt._anchor[0].data_ptr()
    opt.set_consolidation([s.clone() for s in snap], imp, 0.5)
    assert opt._anchor[0].data_ptr() == l2_ptr and opt._l2_on and opt._l2_lambda == 0.1
    with pytest.raises(ValueError, match='same snapshot'):
        opt.set_l2_anchor(other, 0.1)
    opt.set_l2_anchor(None, 0.0)
    assert opt._anchor is not None and not opt._l2_on and opt.l2_lambda == 0.0
    with pytest.raises(RuntimeError, match='FusedSGD.consolidation_penalty'):
        opt.consolidation_penalty()
    opt.set_consolidation(None, None, 0.0)
    assert opt._anchor is None
    opt.set_consolidation(snap, imp, 0.5)
    plain = C.FusedSGD(_params('cpu'), lr=0.1, momentum=0.9)
    assert opt.state_dict() == plain.state_dict()                      # consolidation is not optimiser state


def test_iteration_schedule_and_unchanged_epoch_schedule(C):
    from continual_learning_amd.trainer import make_scheduler
    N, lr = 7, 0.02
    p = torch.nn.Parameter(torch.zeros(3))
    cfg = C.default_config(lr=lr, n_iters=99, lr_schedule='iteration', max_iters=N)
    assert (cfg.optimizer, cfg.momentum, cfg.nesterov, cfg.weight_decay, cfg.decay_norm_and_bias) == ('adam', 0.9, True, 1e-4, True)
    opt = torch.optim.SGD([p], lr=lr)
    sch = make_scheduler(opt, cfg)
    seen = []
    for n in range(N + 3):
        seen.append(opt.param_groups[0]['lr'])
        opt.step()
        sch.step()
    want = [lr * max(0.0, 1 - n / N) ** 0.9 for n in range(N + 3)]
    np.testing.assert_allclose(seen, want, rtol=1e-15, atol=0)
    assert seen[0] == lr and seen[N] == 0.0 and seen[N + 2] == 0.0
    # max_iters None: n_iters epochs of the loader's length
    cfg = C.default_config(lr=lr, n_iters=3, lr_schedule='iteration')
    opt = torch.optim.SGD([p], lr=lr)
    sch = make_scheduler(opt, cfg, iters_per_epoch=4)
    for _ in range(6):
        opt.step()
        sch.step()
    assert opt.param_groups[0]['lr'] == pytest.approx(lr * 0.5 ** 0.9, rel=1e-15)
    with pytest.raises(ValueError, match='max_iters'):
        make_scheduler(opt, cfg)
    with pytest.raises(ValueError, match='lr_schedule'):
        make_scheduler(opt, C.default_config(lr_schedule='step'))
    # the epoch schedule is the reference's: (1 - n/n_iters) ** lr_exp, as the trainer has always built it
    cfg = C.default_config(lr=lr, n_iters=5)
    assert cfg.lr_schedule == 'epoch' and cfg.max_iters is None
    opt = torch.optim.SGD([p], lr=lr)
    sch = make_scheduler(opt, cfg)
    ref_opt = torch.optim.SGD([p], lr=lr)
    ref = torch.optim.lr_scheduler.LambdaLR(ref_opt, lr_lambda=lambda n: (1 - n / cfg.n_iters) ** cfg.lr_exp)
    for _ in range(5):
        assert opt.param_groups[0]['lr'] == ref_opt.param_groups[0]['lr']
        opt.step(); sch.step(); ref_opt.step(); ref.step()
    assert sch.state_dict().keys() == ref.state_dict().keys()


def test_cross_optimiser_checkpoint_is_refused_by_name(C):
    from continual_learning_amd.trainer import check_optimizer_state, optimizer_kind
    ps = _params('cpu')
    for p in ps:
        p.grad = torch.ones_like(p)
    adam = torch.optim.Adam(ps, lr=1e-3); adam.step()
    sgd = torch.optim.SGD(ps, lr=1e-3, momentum=0.9); sgd.step()
    assert optimizer_kind(adam.state_dict()) == 'adam' and optimizer_kind(sgd.state_dict()) == 'sgd'
    assert optimizer_kind(torch.optim.SGD(ps, lr=1e-3).state_dict()) is None
    check_optimizer_state(adam.state_dict(), 'adam')
    check_optimizer_state(sgd.state_dict(), 'sgd')
    for kind in ('adam', 'sgd'):
        check_optimizer_state({'state': {}, 'param_groups': []}, kind)         # an empty state loads into either
    with pytest.raises(ValueError, match="'adam'.*'sgd'"):
        check_optimizer_state(adam.state_dict(), 'sgd')
    with pytest.raises(ValueError, match="'sgd'.*'adam'"):
        check_optimizer_state(sgd.state_dict(), 'adam')
