"""CPU-only tests of clipping by the global gradient norm: the float64 restatement (tests/clip_ref.py) pinned against
torch.nn.utils.clip_grad_norm_, the entry point's validation before any launch, the row size, set_grad_clip's argument checks and the
trainer's max_grad_norm.  No kernel is launched here."""
import ctypes
import math

import numpy as np
import pytest
import torch

import clip_ref


@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    return C


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _tiny():
    g = torch.Generator().manual_seed(7)
    return [torch.randn(s, generator=g, dtype=torch.float64) for s in ((7,), (3, 4))]


@pytest.mark.parametrize('grad_scale', [1.0, 0.5, -0.25])
@pytest.mark.parametrize('where', ['below', 'above', 'inf'])
def test_restatement_matches_clip_grad_norm(where, grad_scale):
    """Two tiny float64 tensors, max_norm below the norm, above it and infinite: the returned norm and the scaled gradients of
    torch.nn.utils.clip_grad_norm_ to 1e-12 relative.  With a grad_scale the restatement is 'scale, then clip': torch clips gradients
    that were multiplied by the scale first, and the norm is that of the scaled gradient."""
    grads = _tiny()
    true_norm = float(torch.cat([g.reshape(-1) for g in grads]).norm()) * abs(grad_scale)
    max_norm = {'below': 0.3 * true_norm, 'above': 2.0 * true_norm, 'inf': math.inf}[where]
    ps = [torch.nn.Parameter(torch.zeros_like(g)) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = g * grad_scale
    total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    r = clip_ref.clip([g.numpy() for g in grads], max_norm, grad_scale)
    assert abs(r['norm'] - float(total)) <= 1e-12 * float(total)
    assert abs(r['norm'] - true_norm) <= 1e-12 * true_norm
    for i, (p, want) in enumerate(zip(ps, clip_ref.clipped([g.numpy() for g in grads], max_norm, grad_scale))):
        assert _rel(want, p.grad.numpy()) <= 1e-12, (where, grad_scale, i)
    for i, g in enumerate(grads):
        assert abs(r['tensor_norms'][i] - float(g.norm()) * abs(grad_scale)) <= 1e-12 * r['tensor_norms'][i]
    if where == 'below':
        assert r['coef'] < 1 and abs(r['coef'] - max_norm / (true_norm + 1e-6)) <= 1e-15
    else:
        assert r['coef'] == 1.0 and r['scale'] == grad_scale


def test_restatement_edge_cases():
    zero = clip_ref.clip([np.zeros(3), np.zeros(2)], 1.0)
    assert zero['norm'] == 0.0 and zero['coef'] == 1.0
    bad = clip_ref.clip([np.array([1.0, np.nan])], 1.0)
    assert math.isnan(bad['norm']) and math.isnan(bad['coef']) and math.isnan(bad['scale'])
    ps = [torch.nn.Parameter(torch.zeros(2, dtype=torch.float64))]
    ps[0].grad = torch.tensor([1.0, math.nan], dtype=torch.float64)
    assert math.isnan(float(torch.nn.utils.clip_grad_norm_(ps, 1.0))) and bool(torch.isnan(ps[0].grad).all())      # torch propagates it too
    big = clip_ref.clip([np.array([1.0, np.inf])], 1.0)
    assert math.isinf(big['norm']) and big['coef'] == 0.0


def test_grad_norm_clip_rejects_bad_arguments_before_any_launch(C):
    """Style of test_path_entry_points_reject_bad_arguments_before_any_launch: every call fails validation on the host (the non-null
    pointers are host memory that nothing dereferences), returns a negative status, and clamd_last_error() names the problem."""
    lib = C._lib.load()
    buf = ctypes.create_string_buffer(256)
    a = ctypes.addressof(buf)
    assert lib.clamd_sizeof_grad_tensor() == 24
    name = 'clamd_grad_norm_clip'
    #        tensors ntensors chunks nchunks hyper max_norm partials clip_out tensor_norms hyper_eff stream
    cases = [
        ('no chunks', (a, 2, a, 0, a, 1.0, a, a, None, a, None)),
        ('no chunks', (a, 2, a, -3, a, 1.0, a, a, None, a, None)),
        ('no tensors', (a, 0, a, 4, a, 1.0, a, a, None, a, None)),
        ('no tensors', (a, -1, a, 4, a, 1.0, a, a, a, a, None)),
        ('null tensor or chunk table', (None, 2, a, 4, a, 1.0, a, a, None, a, None)),
        ('null tensor or chunk table', (a, 2, None, 4, a, 1.0, a, a, None, a, None)),
        ('null hyper / partials / clip_out / hyper_eff', (a, 2, a, 4, None, 1.0, a, a, None, a, None)),
        ('null hyper / partials / clip_out / hyper_eff', (a, 2, a, 4, a, 1.0, None, a, None, a, None)),
        ('null hyper / partials / clip_out / hyper_eff', (a, 2, a, 4, a, 1.0, a, None, None, a, None)),
        ('null hyper / partials / clip_out / hyper_eff', (a, 2, a, 4, a, 1.0, a, a, None, None, None)),
        ('max_norm must be > 0', (a, 2, a, 4, a, 0.0, a, a, None, a, None)),
        ('max_norm must be > 0', (a, 2, a, 4, a, -1.0, a, a, None, a, None)),
        ('max_norm must be > 0', (a, 2, a, 4, a, math.nan, a, a, None, a, None)),
        ('max_norm must be > 0', (a, 2, a, 4, a, -math.inf, a, a, None, a, None)),
    ]
    for needle, args in cases:
        rc = getattr(lib, name)(*args)
        assert rc < 0, (needle, rc)
        assert needle in lib.clamd_last_error().decode(), (needle, lib.clamd_last_error().decode())
        with pytest.raises(RuntimeError) as e:
            C._lib.call(name, *args)
        assert needle in str(e.value) and 'grad_norm_clip' in str(e.value)
    assert bytes(buf) == bytes(256)                    # untouched


def test_grad_tensor_row_matches_the_library(C):
    from continual_learning_amd.optim import _GRAD_TENSOR_DT
    assert C._lib.load().clamd_sizeof_grad_tensor() == _GRAD_TENSOR_DT.itemsize == 24
    assert [_GRAD_TENSOR_DT.fields[k][1] for k in ('g', 'n', 'first_chunk', 'nchunks')] == [0, 8, 16, 20]


@pytest.mark.parametrize('opt_name', ['FusedAdam', 'FusedSGD'])
def test_set_grad_clip_validates_and_allocates_nothing(C, opt_name):
    ps = [torch.nn.Parameter(torch.zeros(3, 2)), torch.nn.Parameter(torch.zeros(5))]
    opt = C.FusedAdam(ps, lr=1e-3, betas=[0.5, 0.99]) if opt_name == 'FusedAdam' else C.FusedSGD(ps, lr=1e-3, momentum=0.9)
    assert opt._clip is None
    for bad in (0, 0.0, -1.0, math.nan, -math.inf):
        with pytest.raises(ValueError, match='max_norm'):
            opt.set_grad_clip(bad)
        assert opt._clip is None
    with pytest.raises(RuntimeError, match='set_grad_clip'):
        opt.grad_norm
    opt.set_grad_clip(12)
    assert opt._clip == 12.0 and type(opt._clip) is float and opt._table is None
    opt.set_grad_clip(math.inf)
    assert opt._clip == math.inf
    for name in ('grad_norm', 'clip_coef', 'grad_nonfinite', 'tensor_grad_norms', 'effective_grad_scale'):
        with pytest.raises(RuntimeError, match='no step'):
            getattr(opt, name)                          # nothing exists before a step has run
    assert opt._clip_out is None and opt._hyper_eff is None and opt._clip_tab is None and opt._clip_part is None
    plain = C.FusedAdam(ps, lr=1e-3, betas=[0.5, 0.99]) if opt_name == 'FusedAdam' else C.FusedSGD(ps, lr=1e-3, momentum=0.9)
    assert opt.state_dict() == plain.state_dict()       # not optimiser state
    for p in ps:
        p.grad = torch.zeros_like(p)
    with pytest.raises(RuntimeError):
        opt.step()                                      # CPU parameters: fails loudly, no fallback
    opt.set_grad_clip(None)
    assert opt._clip is None and opt._clip_out is None


def test_trainer_max_grad_norm(C):
    from continual_learning_amd import trainer as T
    from types import SimpleNamespace
    assert C.default_config().max_grad_norm is None
    cfg = SimpleNamespace(n_iters=5, num_classes=3, conv_dim=4)
    assert T.complete_config(cfg).max_grad_norm is None
    for kind in ('adam', 'sgd'):
        tr = C.Trainer([], C.default_config(n_iters=5, num_classes=3, conv_dim=4, optimizer=kind), device='cpu')
        assert tr.optim._clip is None
        tr = C.Trainer([], C.default_config(n_iters=5, num_classes=3, conv_dim=4, optimizer=kind, max_grad_norm=12), device='cpu')
        assert tr.optim._clip == 12.0
        with pytest.raises(ValueError, match='max_norm'):
            C.Trainer([], C.default_config(n_iters=5, num_classes=3, conv_dim=4, optimizer=kind, max_grad_norm=0.0), device='cpu')
