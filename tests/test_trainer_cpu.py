"""CPU: the host side of trainer.py -- the one defaults table (complete_config), the order of the calls at the task boundary
(begin_task2, grow_head) recorded on stand-ins, the checkpoint host copy and the eval-mode context.  No kernel is launched here: the
arithmetic behind these calls is what the trainer-level GPU tests compare with stock torch."""
import argparse
import os
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

import continual_learning_amd as C
from continual_learning_amd import trainer as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GIVEN = dict(n_iters=7, train_batch_size=2, lr=1e-3, lr_exp=0.9, beta1=0.5, beta2=0.99, h_image_size=32, w_image_size=32,
             num_classes=5, conv_dim=4)


# ---------------------------------------------------------------------------------------------------------------- the defaults table
def test_partial_cfg_builds_the_default_trainer():
    cfg = SimpleNamespace(**GIVEN)
    tr = C.Trainer([], cfg, device='cpu')
    assert type(tr.optim) is C.FusedAdam
    assert not tr.per_iteration and tr.scheduler.lr_lambdas[0](2) == (1 - 2 / 7) ** 0.9              # the epoch schedule
    assert type(tr.c_loss) is C.CrossEntropyLoss and tr.likelihood_loss is tr.c_loss
    assert tr.path is None and tr.augment is None
    assert tr.cfg is cfg and vars(cfg) == vars(C.default_config(**GIVEN))


@pytest.mark.parametrize('namespace', [SimpleNamespace, argparse.Namespace])
def test_complete_config_fills_what_is_missing_on_the_same_object(namespace):
    cfg = namespace(**GIVEN, momentum=0.5)
    assert T.complete_config(cfg) is cfg
    assert vars(cfg) == vars(C.default_config(**GIVEN, momentum=0.5))
    full = C.default_config(num_classes=3, augment_scale=(0.75, 1.5), loss='ce_dice')
    before = dict(vars(full))
    assert T.complete_config(full) is full and vars(full) == before
    opt = torch.optim.SGD([nn.Parameter(torch.zeros(1))], lr=1.0)
    partial = namespace(n_iters=4, lr_exp=1.0)
    assert T.make_scheduler(opt, partial).lr_lambdas[0](1) == 0.75 and partial.lr_schedule == 'epoch' and partial.max_iters is None


def test_defaults_are_written_once():
    src = open(os.path.join(ROOT, 'continual-learning_amd', 'trainer.py')).read()
    assert 'getattr(cfg' not in src and 'getattr(self.cfg' not in src


# ------------------------------------------------------------------------------------------------------------ the task-boundary order
class FakeNet(nn.Module):
    """What begin_task2 and grow_head ask of a model: the constructor arguments, a state, named parameters and a head that grows."""
    grad_sync = None

    def __init__(self, num_classes, in_dim, conv_dim, compute_dtype='fp32'):
        super().__init__()
        self.num_classes, self.in_dim, self.conv_dim, self.compute_dtype = num_classes, in_dim, conv_dim, compute_dtype
        self.weight = nn.Parameter(torch.arange(2.0 * num_classes).reshape(num_classes, 2))
        self.bias = nn.Parameter(torch.arange(1.0 * num_classes))
        self.bn = nn.BatchNorm2d(2)

    def expand_classes(self, n, init):
        ow, ob = self.weight, self.bias
        self.weight = nn.Parameter(torch.cat([ow.detach(), torch.zeros(n, 2)]))
        self.bias = nn.Parameter(torch.cat([ob.detach(), torch.zeros(n)]))
        self.num_classes += n
        return ow, ob, self.weight, self.bias


class RecOptim:
    def __init__(self, log, l2=0.0):
        self.log, self.l2_lambda = log, l2

    def set_l2_anchor(self, anchor, lam):
        self.l2_lambda = float(lam) if anchor is not None else 0.0
        self.log.append(('set_l2_anchor', anchor, lam))

    def set_consolidation(self, anchor, importance, lam):
        self.log.append(('set_consolidation', anchor, importance, lam))

    def set_path_integral(self, omega):
        self.log.append(('set_path_integral', omega))

    def replace_params(self, mapping):
        self.log.append(('replace_params', [(id(k), id(v)) for k, v in mapping.items()]))


class RecCons:
    def __init__(self, log):
        self.log, self.anchor, self.importance, self.gamma = log, [torch.zeros(1)], [torch.ones(1)], 1.0

    def merge_from(self, previous, gamma=None):
        self.log.append(('merge_from', previous, gamma))

    def grow(self, name, new_param):
        self.log.append(('cons.grow', name, new_param))


class RecPath:
    def __init__(self, log, cons):
        self.log, self.cons, self.omega = log, cons, [torch.zeros(1)]

    def consolidate(self, named_params, previous=None):
        self.log.append(('path.consolidate', [n for n, _ in named_params], previous))
        return self.cons

    def restart(self, params):
        self.log.append(('path.restart', list(params)))

    def grow(self, name, new_param, old_param=None):
        self.log.append(('path.grow', name, new_param, old_param))


def same(a, b):
    """Equality with tensors (and the recording stand-ins) compared by identity."""
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if torch.is_tensor(a) or torch.is_tensor(b) or isinstance(a, (RecCons, RecPath)):
        return a is b
    return type(a) is type(b) and a == b


@pytest.fixture
def boundary(monkeypatch):
    """A CPU trainer whose model, optimiser and importance estimate are recording stand-ins -> (trainer, log)."""
    tr = C.Trainer([], C.default_config(num_classes=5, conv_dim=4), device='cpu')
    log = []

    def snapshot_net(*a, **kw):                 # begin_task2 builds exactly one more network: the frozen snapshot
        log.append(('snapshot',))
        return FakeNet(*a, **kw)

    tr.model = FakeNet(5, 3, 4)
    monkeypatch.setattr(T, 'UNet', snapshot_net)
    tr.optim = RecOptim(log)
    return tr, log


def test_l2_alone_anchors_to_clones_of_the_snapshot(boundary):
    tr, log = boundary
    tr.begin_task2(3, distill_lambda=0, l2_lambda=0.25)
    old = tr.old_model
    assert isinstance(old, FakeNet) and old is not tr.model and not old.training and tr.model.training
    assert (old.num_classes, old.in_dim, old.conv_dim, old.compute_dtype) == (5, 3, 4, 'fp32')
    for (n, p), (m, q) in zip(old.named_parameters(), tr.model.named_parameters()):
        assert n == m and not p.requires_grad and q.requires_grad and p.data_ptr() != q.data_ptr() and torch.equal(p, q)
    assert [e[0] for e in log] == ['snapshot', 'set_l2_anchor'] and log[1][2] == 0.25
    anchors = log[1][1]
    assert len(anchors) == 4
    for a, p in zip(anchors, old.parameters()):
        assert a is not p and a.data_ptr() != p.data_ptr() and torch.equal(a, p) and not a.requires_grad
    assert tr.consolidation is None and tr.ewc_lambda == 0.0 and tr.distill is None and tr.pod is None and tr.pseudo is None


def test_ewc_boundary_merges_snapshots_then_hands_the_consolidation_over(boundary):
    tr, log = boundary
    previous, new, loader = RecCons(log), RecCons(log), object()
    tr.consolidation = previous
    tr.estimate_importance = lambda data_loader: (log.append(('estimate', data_loader)), new)[1]
    tr.begin_task2(3, distill_lambda=0, ewc_lambda=5.0, ewc_gamma=0.5, l2_lambda=0.25, importance_loader=loader)
    assert same(log, [('estimate', loader), ('merge_from', previous, 0.5), ('snapshot',), ('set_l2_anchor', None, 0.0),
                      ('set_consolidation', new.anchor, new.importance, 5.0), ('set_l2_anchor', new.anchor, 0.25)]), log
    assert tr.consolidation is new and new.gamma == 0.5 and tr.ewc_lambda == 5.0
    del log[:]
    tr.begin_task2(3, distill_lambda=0, ewc_lambda=2.0)          # no L2 term: an earlier one is cleared and stays cleared; default loader
    assert same(log, [('estimate', tr.train_data_loader), ('merge_from', new, 1.0), ('snapshot',), ('set_l2_anchor', None, 0.0),
                      ('set_consolidation', new.anchor, new.importance, 2.0)]), log


def test_path_boundary_consolidates_restarts_and_doubles_lambda(boundary):
    tr, log = boundary
    previous, new = RecCons(log), RecCons(log)
    tr.consolidation, tr.path = previous, RecPath(log, new)
    tr.begin_task2(3, distill_lambda=0, si_lambda=1.5, l2_lambda=0.25)
    assert same(log, [('path.consolidate', ['weight', 'bias', 'bn.weight', 'bn.bias'], previous), ('path.restart', list(tr.model.parameters())), ('snapshot',),
                      ('set_l2_anchor', None, 0.0), ('set_consolidation', new.anchor, new.importance, 3.0),
                      ('set_l2_anchor', new.anchor, 0.25)]), log
    assert tr.consolidation is new and tr.ewc_lambda == 3.0


def test_grow_head_grows_the_owners_first_then_the_optimiser_reads_them(boundary):
    tr, log = boundary
    cons = RecCons(log)
    tr.consolidation, tr.ewc_lambda, tr.path, tr.optim.l2_lambda = cons, 5.0, RecPath(log, None), 0.25
    ow, ob = tr.model.weight, tr.model.bias
    tr.grow_head(2)
    nw, nb = tr.model.weight, tr.model.bias
    assert nw is not ow and nw.shape == (7, 2) and nb.shape == (7,)
    assert same(log, [('cons.grow', 'weight', nw), ('cons.grow', 'bias', nb), ('path.grow', 'weight', nw, ow), ('path.grow', 'bias', nb, ob),
                      ('replace_params', [(id(ow), id(nw)), (id(ob), id(nb))]), ('set_path_integral', tr.path.omega),
                      ('set_l2_anchor', None, 0.0), ('set_consolidation', cons.anchor, cons.importance, 5.0),
                      ('set_l2_anchor', cons.anchor, 0.25)]), log
    assert tr.cfg.num_classes == tr.model.num_classes == 7
    del log[:]
    tr.consolidation = tr.path = None                             # the L2 term alone: replace_params grows the optimiser's own anchors
    tr.grow_head(1)
    assert [e[0] for e in log] == ['replace_params'] and tr.cfg.num_classes == 8


def test_begin_task2_grows_after_the_handover_and_freezes_last(boundary):
    tr, log = boundary
    new = RecCons(log)
    tr.estimate_importance = lambda data_loader: new
    tr.begin_task2(5, distill_lambda=0, ewc_lambda=5.0, new_classes=2, freeze_bn=True)
    assert [e[0] for e in log] == ['snapshot', 'set_l2_anchor', 'set_consolidation', 'cons.grow', 'cons.grow', 'replace_params',
                                   'set_l2_anchor', 'set_consolidation']
    assert tr.old_model.num_classes == 5 and tr.model.num_classes == tr.cfg.num_classes == 7      # the snapshot keeps its width
    assert tr.model.training and not tr.model.bn.training


def test_a_bad_argument_is_refused_before_the_replay_loader_is_touched(boundary):
    tr, log = boundary

    class Untouchable:
        def __iter__(self):
            raise AssertionError('the loader was read before the arguments were checked')

    with pytest.raises(ValueError, match='pod_lambda must be >= 0'):
        tr.begin_task2(3, distill_lambda=0, replay=2, replay_batch=1, replay_loader=Untouchable(), pod_lambda=-1.0)
    with pytest.raises(ValueError, match="loss='ce_dice' with unbiased=True"):
        tr.cfg.loss = 'ce_dice'                                   # the last check of all
        tr.begin_task2(3, distill_lambda=0, replay=2, replay_batch=1, replay_loader=Untouchable(), unbiased=True)
    assert log == [] and tr.replay is None and tr.replay_batch == 0 and tr.old_model is None


# ------------------------------------------------------------------------------------------------------------------ the eval context
class Predictor(nn.Module):
    def __init__(self):
        super().__init__()
        self.frozen, self.live = nn.BatchNorm2d(1), nn.BatchNorm2d(1)
        self.frozen.eval()
        self.seen = []

    def predict(self, x):
        self.seen.append((self.training, self.frozen.training, self.live.training))
        return torch.zeros(x.shape[0], dtype=torch.int64)


def test_test_runs_in_eval_mode_and_hands_every_module_its_own_mode_back(boundary):
    tr, _ = boundary
    tr.model = Predictor()
    batch = (torch.zeros(4, 3), torch.tensor([0, 0, 1, 0]))
    assert tr.test([batch, batch]) == 75.0
    assert tr.model.seen == [(False, False, False)] * 2
    assert (tr.model.training, tr.model.frozen.training, tr.model.live.training) == (True, False, True)


def test_test_hands_the_modes_back_after_an_error_too(boundary):
    tr, _ = boundary
    tr.model = Predictor()
    batch = (torch.zeros(4, 3), torch.tensor([0, 0, 1, 0]))

    def failing():
        yield batch
        raise KeyError('the loader failed')

    with pytest.raises(KeyError):
        tr.test(failing())
    assert (tr.model.training, tr.model.frozen.training, tr.model.live.training) == (True, False, True)     # also after an error


# --------------------------------------------------------------------------------------------------------------------- the host copy
def test_host_copy_keeps_the_structure_and_the_host_tensors():
    a, b, c = torch.zeros(2), torch.ones(3, dtype=torch.int64), torch.zeros((), dtype=torch.uint8)
    state = {'anchor': {'w': a, 'b': b}, 'n_batches': 3, 'rng': None, 'image_shape': (3, 8, 8), 'segments': [{'lo': 1, 'seen': [0, 2]}, (c, 'x')],
             0: {'step': c, 'gamma': 0.5}}
    got = T._host_copy(state)
    assert list(got) == list(state) and got is not state
    assert got['anchor']['w'] is a and got['anchor']['b'] is b and got[0]['step'] is c and got['segments'][1][0] is c
    assert type(got['image_shape']) is tuple and got['image_shape'] == (3, 8, 8) and type(got['segments']) is list
    assert type(got['segments'][1]) is tuple and got['segments'][1][1] == 'x' and got['segments'][0] == {'lo': 1, 'seen': [0, 2]}
    assert got['n_batches'] == 3 and got['rng'] is None and got[0]['gamma'] == 0.5 and set(got[0]) == {'step', 'gamma'}
