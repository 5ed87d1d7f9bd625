"""CPU-only tests of elastic weight consolidation's host side: the entry points validate before any launch, FusedAdam.set_consolidation
validates its arguments, Consolidation.state_dict round-trips by parameter name, and checkpoints with and without the optional
'consolidation_state' key load.  No kernel is launched here."""
import ctypes
import math
import os

import pytest
import torch


@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    return C


def test_ewc_entry_points_reject_bad_arguments_before_any_launch(C):
    """Style of test_abi_rejects_bad_arguments_before_any_launch: every call fails validation on the host (the non-null pointers are host
    memory that nothing dereferences), returns a negative status, and clamd_last_error() names the problem."""
    lib = C._lib.load()
    call = C._lib.call
    buf = ctypes.create_string_buffer(256)
    a = ctypes.addressof(buf)
    assert lib.clamd_sizeof_importance_tensor() == 24 and lib.clamd_sizeof_adam_tensor() == 48
    cases = [
        ('no chunks', 'clamd_importance_accum', (a, a, 0, 1.0, 1.0, 2, None)),
        ('no chunks', 'clamd_importance_accum', (a, a, -3, 1.0, 1.0, 2, None)),
        ('null tensor or chunk table', 'clamd_importance_accum', (None, a, 4, 1.0, 1.0, 2, None)),
        ('null tensor or chunk table', 'clamd_importance_accum', (a, None, 4, 1.0, 1.0, 2, None)),
        ('power must be 1 or 2', 'clamd_importance_accum', (a, a, 4, 1.0, 1.0, 3, None)),
        ('power must be 1 or 2', 'clamd_importance_accum', (a, a, 4, 1.0, 1.0, 0, None)),
        ('decay must be finite and >= 0', 'clamd_importance_accum', (a, a, 4, -0.5, 1.0, 2, None)),
        ('decay must be finite and >= 0', 'clamd_importance_accum', (a, a, 4, math.nan, 1.0, 2, None)),
        ('decay must be finite and >= 0', 'clamd_importance_accum', (a, a, 4, math.inf, 1.0, 2, None)),
        ('scale must be finite and >= 0', 'clamd_importance_accum', (a, a, 4, 1.0, -1.0, 1, None)),
        ('scale must be finite and >= 0', 'clamd_importance_accum', (a, a, 4, 1.0, math.inf, 1, None)),
        ('scale must be finite and >= 0', 'clamd_importance_accum', (a, a, 4, 1.0, math.nan, 1, None)),
        ('no chunks', 'clamd_adam_step_consolidated', (a, a, a, 0, a, a, a, a, None, None)),
        ('null tensor or chunk table', 'clamd_adam_step_consolidated', (None, a, a, 4, a, a, a, a, None, None)),
        ('null tensor or chunk table', 'clamd_adam_step_consolidated', (a, a, None, 4, a, a, a, a, None, None)),
        ('null importance table', 'clamd_adam_step_consolidated', (a, None, a, 4, a, a, a, a, None, None)),
        ('null hyper / step / derived', 'clamd_adam_step_consolidated', (a, a, a, 4, None, a, a, a, None, None)),
        ('null hyper / step / derived', 'clamd_adam_step_consolidated', (a, a, a, 4, a, None, a, a, None, None)),
        ('null hyper / step / derived', 'clamd_adam_step_consolidated', (a, a, a, 4, a, a, None, a, None, None)),
        ('null penalty buffer', 'clamd_adam_step_consolidated', (a, a, a, 4, a, a, a, None, None, None)),
        ('no chunks', 'clamd_adam_step', (a, a, 0, a, a, a, None, None)),
        ('no chunks', 'clamd_adam_step', (a, a, -1, a, a, a, None, None)),
        ('null tensor or chunk table', 'clamd_adam_step', (None, a, 4, a, a, a, None, None)),
        ('null tensor or chunk table', 'clamd_adam_step', (a, None, 4, a, a, a, None, None)),
        ('null hyper / step / derived', 'clamd_adam_step', (a, a, 4, None, a, a, None, None)),
        ('null hyper / step / derived', 'clamd_adam_step', (a, a, 4, a, None, a, None, None)),
        ('null hyper / step / derived', 'clamd_adam_step', (a, a, 4, a, a, None, None, None)),
    ]
    for needle, name, args in cases:
        with pytest.raises(RuntimeError) as e:
            call(name, *args)
        assert needle in str(e.value), (name, str(e.value))
        assert needle in lib.clamd_last_error().decode()
    assert bytes(buf) == bytes(256)                    # untouched


def _params(dev, shapes=((3, 2), (5,))):
    return [torch.nn.Parameter(torch.zeros(*s, device=dev)) for s in shapes]


def test_set_consolidation_validates_count_shape_device_and_anchor(C):
    # 'meta' stands in for the GPU: a device that is not the CPU, without needing one
    ps = _params('meta')
    opt = C.FusedAdam(ps, lr=1e-3, betas=[0.5, 0.99])
    like = lambda dev: [torch.zeros(p.shape, device=dev) for p in ps]
    opt.set_consolidation(like('meta'), like('meta'), 0.5)
    assert opt._ewc_lambda == 0.5 and len(opt._importance) == 2
    opt.set_consolidation(None, None, 0.0)
    assert opt._importance is None and opt._anchor is None and opt._ewc_lambda == 0.0
    with pytest.raises(ValueError, match='2 parameters, 1 anchors'):
        opt.set_consolidation(like('meta')[:1], like('meta'), 0.5)
    with pytest.raises(ValueError, match='2 importance tensors|3 importance tensors'):
        opt.set_consolidation(like('meta'), like('meta') + like('meta')[:1], 0.5)
    bad = like('meta'); bad[1] = torch.zeros(4, device='meta')
    with pytest.raises(ValueError, match='shape'):
        opt.set_consolidation(like('meta'), bad, 0.5)
    with pytest.raises(ValueError, match='shape'):
        opt.set_consolidation(bad, like('meta'), 0.5)
    cpu_one = like('meta'); cpu_one[0] = torch.zeros(ps[0].shape)          # a CPU tensor among the device ones
    with pytest.raises(ValueError, match='importance on cpu'):
        opt.set_consolidation(like('meta'), cpu_one, 0.5)
    with pytest.raises(ValueError, match='anchor on cpu'):
        opt.set_consolidation(cpu_one, like('meta'), 0.5)
    half = like('meta'); half[0] = half[0].half()
    with pytest.raises(ValueError, match='fp32'):
        opt.set_consolidation(like('meta'), half, 0.5)
    with pytest.raises(ValueError, match='lam'):
        opt.set_consolidation(like('meta'), like('meta'), -1.0)
    assert opt._importance is None                                         # nothing was installed by the failed calls
    # one anchor pointer per tensor: an L2 anchor and a consolidation anchor must be the same snapshot
    ps = _params('cpu')
    opt = C.FusedAdam(ps, lr=1e-3, betas=[0.5, 0.99])
    snap = [torch.full(p.shape, 1.0) for p in ps]
    other = [torch.full(p.shape, 2.0) for p in ps]
    imp = [torch.ones(p.shape) for p in ps]
    opt.set_l2_anchor(snap, 0.1)
    with pytest.raises(ValueError, match='same snapshot'):
        opt.set_consolidation(other, imp, 0.5)
    assert opt._importance is None
    l2_ptr = opt._anchor[0].data_ptr()
    opt.set_consolidation([s.clone() for s in snap], imp, 0.5)             # equal values: accepted, the L2 anchor stays
    assert opt._anchor[0].data_ptr() == l2_ptr and opt._l2_on and opt._l2_lambda == 0.1
    with pytest.raises(ValueError, match='same snapshot'):
        opt.set_l2_anchor(other, 0.1)
    opt.set_l2_anchor(None, 0.0)                                           # clearing L2 keeps the anchor the consolidation needs
    assert opt._anchor is not None and not opt._l2_on
    opt.set_consolidation(None, None, 0.0)
    assert opt._anchor is None
    # the optimiser's checkpoint layout is torch-Adam's: consolidation is not optimiser state
    opt.set_consolidation(snap, imp, 0.5)
    plain = C.FusedAdam(_params('cpu'), lr=1e-3, betas=[0.5, 0.99])
    assert opt.state_dict() == plain.state_dict() and set(opt.state_dict()) == {'state', 'param_groups'}
    for p in ps:
        p.grad = torch.zeros_like(p)
    with pytest.raises(RuntimeError):
        opt.step()                                                         # CPU parameters: fails loudly, no fallback


def test_consolidation_state_dict_round_trips_by_name(C):
    g = torch.Generator().manual_seed(0)
    named = [('b.weight', torch.randn(3, 2, generator=g)), ('a.bias', torch.randn(5, generator=g))]
    c = C.Consolidation(named, gamma=0.9)
    assert [tuple(w.shape) for w in c.importance] == [(3, 2), (5,)] and c.flat.numel() == 11
    assert all(w.data_ptr() == c.flat.data_ptr() + 4 * o for w, o in zip(c.importance, (0, 6)))     # views of ONE flat buffer
    assert all(torch.equal(a, p) and a.data_ptr() != p.data_ptr() for a, (_, p) in zip(c.anchor, named))
    c.flat.copy_(torch.rand(11, generator=g))
    c.n_batches, c.finished = 7, True
    sd = c.state_dict()
    assert set(sd) == {'importance', 'anchor', 'n_batches', 'gamma'} and list(sd['importance']) == ['b.weight', 'a.bias']
    saved = {'importance': {k: v.clone() for k, v in reversed(list(sd['importance'].items()))},          # another key order
             'anchor': {k: v.clone() for k, v in reversed(list(sd['anchor'].items()))}, 'n_batches': 7, 'gamma': 0.9}
    d = C.Consolidation([(n, torch.zeros_like(p)) for n, p in named])
    d.load_state_dict(saved)
    assert d.n_batches == 7 and d.gamma == 0.9 and d.finished
    for a, b in zip(c.importance + c.anchor, d.importance + d.anchor):
        assert torch.equal(a, b)
    with pytest.raises(KeyError, match='missing'):
        d.load_state_dict({**saved, 'importance': {'b.weight': saved['importance']['b.weight']}})
    with pytest.raises(ValueError, match='shape'):
        d.load_state_dict({**saved, 'anchor': {'b.weight': torch.zeros(2, 3), 'a.bias': torch.zeros(5)}})
    with pytest.raises(RuntimeError, match='no CPU fallback|no gradient'):
        C.Consolidation(named).accumulate([torch.nn.Parameter(p) for _, p in named])
    p2 = [torch.nn.Parameter(p.clone()) for _, p in named]
    for p in p2:
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        C.Consolidation(named).accumulate(p2)


def test_checkpoints_with_and_without_consolidation_state_load(C, tmp_path):
    """A checkpoint with the reference's four keys only (what the parent commit wrote) still loads and leaves consolidation off; one that
    carries 'consolidation_state' restores anchor, importance, lambda, gamma and the batch count by name."""
    cfg = C.default_config(n_iters=10, num_classes=3, conv_dim=4)
    tr = C.Trainer([], cfg, device='cpu')
    ck = {'epoch': 4, 'model_state': tr.model.state_dict(), 'optimizer_state': tr.optim.state_dict(),
          'scheduler_state': tr.scheduler.state_dict()}
    torch.save(ck, os.path.join(tmp_path, '3_net_G.pth'))
    tr2 = C.Trainer([], cfg, device='cpu')
    assert tr2.load_network('G', 3, str(tmp_path)) is True
    assert tr2.start_epoch == 4 and tr2.consolidation is None and tr2.ewc_lambda == 0.0 and tr2.optim._importance is None
    assert tr2.load_network('G', 99, str(tmp_path)) is False
    g = torch.Generator().manual_seed(1)
    names = [n for n, _ in tr.model.named_parameters()]
    ck['consolidation_state'] = {'anchor': {n: torch.randn(p.shape, generator=g) for n, p in tr.model.named_parameters()},
                                 'importance': {n: torch.rand(p.shape, generator=g) for n, p in tr.model.named_parameters()},
                                 'lambda': 40.0, 'gamma': 0.8, 'n_batches': 5}
    torch.save(ck, os.path.join(tmp_path, '4_net_G.pth'))
    assert tr2.load_network('G', 4, str(tmp_path)) is True
    c = tr2.consolidation
    assert c.names == names and c.n_batches == 5 and c.gamma == 0.8 and tr2.ewc_lambda == 40.0
    for n, w, a in zip(names, c.importance, c.anchor):
        assert torch.equal(w, ck['consolidation_state']['importance'][n]) and torch.equal(a, ck['consolidation_state']['anchor'][n])
    assert tr2.optim._ewc_lambda == 40.0 and all(w.data_ptr() == v.data_ptr() for w, v in zip(tr2.optim._importance, c.importance))
