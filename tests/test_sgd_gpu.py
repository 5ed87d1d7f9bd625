"""GPU: the fused SGD step (csrc/optim.hip, optim.FusedSGD) -- per element against the float64 restatement of tests/sgd_ref.py across its
grid of settings, the exact cases, a trajectory against torch.optim.SGD with checkpoints handed over both ways, the two penalty sums, a
whole small UNet against the stock-torch module in float64, and the trainer with optimizer='sgd' and the per-iteration schedule."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import sgd_ref
from conftest import rel_l2
from grid_util import Banded, POISON, _per_element
from oracle import torch_cpu as TC

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
SIZES = (1, 3, 257, 4095, 4096, 8195)
NO_DECAY = 2                                   # index of the tensor with decay_mult 0
f32 = lambda v: float(np.float32(v))           # the value the kernel reads from its fp32 hyper buffer


@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    C._lib.load()
    return C


_INPUTS = {}


def _inputs():
    """Standard-normal values with some exact zeros, generated once on the host: p, g, buf, old per tensor and omega in [0, 2)."""
    if not _INPUTS:
        rng = np.random.default_rng(11)
        def normal(n):
            a = rng.standard_normal(n).astype(np.float32)
            a[rng.random(n) < 0.05] = 0.0
            return torch.from_numpy(a)
        for name in ('p', 'g', 'buf', 'old'):
            _INPUTS[name] = [normal(n) for n in SIZES]
        _INPUTS['omega'] = [torch.from_numpy((rng.random(n) * 2).astype(np.float32)) for n in SIZES]
        _INPUTS['omega'][3][:7] = 0.0
    return _INPUTS


def _launch(C, P, G, Bf, old, omega, hyper, l2_on):
    """One clamd_sgd_step over the six tensors through a table built here; returns (ewc accumulator, l2 accumulator)."""
    from continual_learning_amd.optim import _SGD_TENSOR_DT
    lib = C._lib.load()
    chunk = lib.clamd_adam_chunk_elems()
    t = np.zeros(len(SIZES), dtype=_SGD_TENSOR_DT)
    chunks = []
    for i, n in enumerate(SIZES):
        t[i] = (P.views[i].data_ptr(), G.views[i].data_ptr(), Bf.views[i].data_ptr() if Bf is not None else 0,
                old[i].data_ptr() if old is not None else 0, n, 0.0 if i == NO_DECAY else 1.0, 0.0)
        chunks += [(i, c) for c in range((n + chunk - 1) // chunk)]
    tensors = torch.from_numpy(t.view(np.uint8).copy()).to(DEV)
    chunks_dev = torch.tensor(chunks, dtype=torch.int32, device=DEV)
    hyper_dev = torch.tensor(hyper, dtype=torch.float32, device=DEV)
    imp = torch.tensor([w.data_ptr() for w in omega], dtype=torch.int64).to(DEV) if omega is not None else None
    ewc = torch.full((1 + len(chunks),), POISON, device=DEV) if omega is not None else None
    l2 = torch.full((1 + len(chunks),), POISON, device=DEV) if l2_on else None
    ptr = C._lib.ptr
    C._lib.call('clamd_sgd_step', ptr(tensors), ptr(imp), ptr(chunks_dev), len(chunks), ptr(hyper_dev), ptr(ewc), ptr(l2), C._lib.stream_ptr())
    torch.cuda.synchronize()
    return ewc, l2


@pytest.mark.parametrize('gs', [1.0, 0.375])
@pytest.mark.parametrize('terms', ['none', 'l2', 'ewc', 'both'])
@pytest.mark.parametrize('wd', [0.0, 0.05])
@pytest.mark.parametrize('mu,nesterov', [(0.0, False), (0.9, False), (0.9, True)])
def test_sgd_step_per_element(C, mu, nesterov, wd, terms, gs):
    """One step from a known state: p and buf of every element against the float64 restatement within bounds derived from the number of
    roundings (sgd_ref.bounds), guard bands bit-intact, two runs from the same state bit-identical.  Gradients at element phases 0..3, one
    parameter and some buffers at odd phases, tensor NO_DECAY without weight decay."""
    inp = _inputs()
    lr = 0.1
    l2_lam = 0.3 if terms in ('l2', 'both') else 0.0
    ewc_lam = 0.7 if terms in ('ewc', 'both') else 0.0
    P = Banded(SIZES, (0, 0, 0, 1, 0, 0), inp['p'])
    G = Banded(SIZES, (0, 1, 2, 3, 1, 2), inp['g'])
    Bf = Banded(SIZES, (0, 3, 0, 0, 2, 1), inp['buf']) if mu > 0 else None
    anchored = terms != 'none'
    old = Banded(SIZES, (1, 2, 0, 3, 0, 3), inp['old']).views if anchored else None
    omega = Banded(SIZES, (2, 0, 1, 0, 0, 3), inp['omega']).views if ewc_lam else None
    hyper = [lr, mu, wd, 1.0 if nesterov else 0.0, gs, l2_lam, ewc_lam, 0.0]
    ewc, l2 = _launch(C, P, G, Bf, old, omega, hyper, l2_lam > 0)
    got_p, got_b = P.flat.clone(), (Bf.flat.clone() if Bf is not None else None)
    assert P.guards_intact() and G.guards_intact() and (Bf is None or Bf.guards_intact()), 'a store outside [0, n) of a tensor'
    assert torch.equal(G.flat.view(torch.int32), G.before.view(torch.int32))
    l2_ref = ewc_ref = 0.0
    for i, n in enumerate(SIZES):
        ref = sgd_ref.sgd_step(inp['p'][i].numpy(), inp['g'][i].numpy(), inp['buf'][i].numpy() if mu > 0 else None,
                               inp['old'][i].numpy() if anchored else None, inp['omega'][i].numpy() if ewc_lam else None,
                               lr=f32(lr), momentum=f32(mu), weight_decay=f32(wd), nesterov=nesterov, grad_scale=f32(gs),
                               decay_mult=0.0 if i == NO_DECAY else 1.0, l2_lambda=f32(l2_lam), ewc_lambda=f32(ewc_lam))
        bb, pb = sgd_ref.bounds(inp['p'][i].numpy(), ref, lr=f32(lr), momentum=f32(mu))
        key = ('sgd', mu, nesterov)
        _per_element(f'sgd p[{i}] n={n} mu={mu} nesterov={nesterov} wd={wd} {terms} gs={gs}', key, P.views[i].cpu(),
                     torch.from_numpy(ref['p']), torch.from_numpy(pb))
        if mu > 0:
            _per_element(f'sgd buf[{i}] n={n} mu={mu} nesterov={nesterov} wd={wd} {terms} gs={gs}', key, Bf.views[i].cpu(),
                         torch.from_numpy(ref['buf']), torch.from_numpy(bb))
        l2_ref += ref['l2']
        ewc_ref += ref['ewc']
    if l2 is not None:
        assert abs(float(l2[0]) - l2_ref) <= 2e-6 * l2_ref
    if ewc is not None:
        assert abs(float(ewc[0]) - ewc_ref) <= 2e-6 * ewc_ref
    # the same launch from the same state: the same bits
    P.restore()
    if Bf is not None:
        Bf.restore()
    ewc2, l22 = _launch(C, P, G, Bf, old, omega, hyper, l2_lam > 0)
    assert torch.equal(P.flat.view(torch.int32), got_p.view(torch.int32))
    assert Bf is None or torch.equal(Bf.flat.view(torch.int32), got_b.view(torch.int32))
    assert ewc is None or torch.equal(ewc.view(torch.int32), ewc2.view(torch.int32))
    assert l2 is None or torch.equal(l2.view(torch.int32), l22.view(torch.int32))


def _param(values):
    return nn.Parameter(values.to(DEV).clone())


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def test_exact_cases(C):
    rng = np.random.default_rng(12)
    n = 4099
    p0 = torch.from_numpy(rng.standard_normal(n).astype(np.float32))
    g = torch.from_numpy(rng.standard_normal(n).astype(np.float32))
    # lr = 0: p bit-unchanged while buf moves
    p = _param(p0)
    opt = C.FusedSGD([p], lr=0.0, momentum=0.9, nesterov=True, weight_decay=0.05)
    p.grad = g.to(DEV)
    opt.step()
    assert torch.equal(_bits(p), _bits(p0.to(DEV)))
    buf = opt.state[p]['momentum_buffer']
    assert buf.shape == p.shape and torch.count_nonzero(buf) > n // 2
    # grad_scale = 0.5 on 2g equals grad_scale = 1 on g, bit for bit (p and buf, two steps)
    outs = []
    for scale, mult in ((1.0, 1.0), (0.5, 2.0)):
        p = _param(p0)
        opt = C.FusedSGD([p], lr=0.1, momentum=0.9, nesterov=True, weight_decay=0.05, grad_scale=scale)
        for _ in range(2):
            p.grad = (g * mult).to(DEV)
            opt.step()
        outs.append((_bits(p).clone(), _bits(opt.state[p]['momentum_buffer']).clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # mu = 0, wd = 0, no anchor: p - lr * g within 1 ulp; no state
    p = _param(p0)
    opt = C.FusedSGD([p], lr=0.1)
    p.grad = g.to(DEV)
    opt.step()
    want = p0.double().numpy() - f32(0.1) * g.double().numpy()
    got = p.detach().cpu().numpy()
    assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))
    assert opt.state_dict()['state'] == {}
    # a change of param_groups[0]['lr'] is picked up at the next step
    p1 = p.detach().clone()
    opt.param_groups[0]['lr'] = 0.05
    opt.step()
    want = p1.cpu().double().numpy() - f32(0.05) * g.double().numpy()
    got = p.detach().cpu().numpy()
    assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))
    assert not torch.equal(p.detach(), p1)


@pytest.mark.parametrize('nesterov', [False, True])
def test_trajectory_and_checkpoint_interchange_with_torch_sgd(C, nesterov):
    """4 steps on one tensor against torch.optim.SGD in float64 (rel_l2 < 1e-6 for p and momentum_buffer at every step, the bar of the
    Adam golden test); after step 2 the state goes FusedSGD -> torch SGD and torch SGD -> a fresh FusedSGD, and both continue two steps."""
    rng = np.random.default_rng(13)
    n, kw = 5000, dict(lr=0.05, momentum=0.9, nesterov=nesterov, weight_decay=0.05)
    p0 = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).view(50, 100)
    grads = [torch.from_numpy(rng.standard_normal(n).astype(np.float32)).view(50, 100) for _ in range(4)]
    p = _param(p0)
    opt = C.FusedSGD([p], **kw)
    rp = nn.Parameter(p0.double().clone())
    ropt = torch.optim.SGD([rp], **kw)

    def check(fp, fopt, tp, topt, what):
        assert rel_l2(fp.detach().cpu().numpy(), tp.detach().numpy()) < 1e-6, what
        assert rel_l2(fopt.state[fp]['momentum_buffer'].cpu().numpy(), topt.state[tp]['momentum_buffer'].numpy()) < 1e-6, what

    handed = None
    for i, g in enumerate(grads):
        p.grad, rp.grad = g.to(DEV), g.double().clone()
        opt.step(); ropt.step()
        check(p, opt, rp, ropt, f'step {i}')
        if handed is not None:
            tp, topt, fp, fopt = handed
            tp.grad, fp.grad = g.double().clone(), g.to(DEV)
            topt.step(); fopt.step()
            assert rel_l2(tp.detach().numpy(), rp.detach().numpy()) < 1e-6, f'FusedSGD -> torch, step {i}'
            assert rel_l2(topt.state[tp]['momentum_buffer'].numpy(), ropt.state[rp]['momentum_buffer'].numpy()) < 1e-6
            check(fp, fopt, rp, ropt, f'torch -> FusedSGD, step {i}')
        if i == 1:
            sd = opt.state_dict()
            assert set(sd['state'][0]) == {'momentum_buffer'} and sd['state'][0]['momentum_buffer'].shape == p.shape
            tp = nn.Parameter(p.detach().cpu().double())
            topt = torch.optim.SGD([tp], lr=1.0)
            topt.load_state_dict(sd)
            fp = _param(rp.detach().float())
            fopt = C.FusedSGD([fp], lr=1.0)
            fopt.load_state_dict(ropt.state_dict())
            handed = (tp, topt, fp, fopt)


def test_penalties_match_float64_sums_and_repeat_bit_for_bit(C):
    """1 100 003 elements = 269 workgroups, so the final sum's strided loop runs.  lr = 0 and no momentum: every step sees the same state."""
    n = 1100003
    g = torch.Generator().manual_seed(14)
    p0, old = torch.randn(n, generator=g), torch.randn(n, generator=g)
    omega = torch.rand(n, generator=g) * 2
    p = _param(p0)
    opt = C.FusedSGD([p], lr=0.0)
    anchor = [old.to(DEV)]
    opt.set_consolidation(anchor, [omega.to(DEV)], 0.7)
    opt.set_l2_anchor(anchor, 0.3)
    p.grad = torch.zeros(n, device=DEV)
    d = p0.double() - old.double()
    l2_ref = 0.3 * float((d * d).sum())
    ewc_ref = 0.35 * float((omega.double() * d * d).sum())
    seen = []
    for _ in range(5):
        opt.step()
        seen.append((_bits(opt.l2_penalty()).item(), _bits(opt.consolidation_penalty()).item()))
    assert opt._nchunks > 256
    l2, ewc = float(opt.l2_penalty()), float(opt.consolidation_penalty())
    print(f'l2 penalty rel err {abs(l2 - l2_ref) / l2_ref:.2e}, consolidation penalty rel err {abs(ewc - ewc_ref) / ewc_ref:.2e}')
    assert abs(l2 - l2_ref) <= 2e-6 * l2_ref and abs(ewc - ewc_ref) <= 2e-6 * ewc_ref
    assert len(set(seen)) == 1, seen
    assert torch.equal(_bits(p), _bits(p0.to(DEV)))


def test_whole_model_training_loop_matches_torch(C):
    """UNet(4, 3, 8), 32x32, batch 2, BatchNorm in train mode, 4 steps: FusedSGD(lr 0.01, momentum 0.9, Nesterov, weight decay 1e-4) with a
    LambdaLR against the stock-torch module in float64 with torch.optim.SGD, pattern and rtol = 2e-4 of
    test_frozen_bn_training_loop_matches_torch.  (For scale: the same stock-torch loop in fp32 on the CPU departs from the float64 one by
    at most 1e-7 relative on these four losses.)"""
    nc, cd, B, H, W = 4, 8, 2, 32, 32
    torch.manual_seed(5)
    ref = TC.build_unet(nc, 3, cd).double()
    sd = {k: (v.float() if v.is_floating_point() else v).clone() for k, v in ref.state_dict().items()}
    ref.load_state_dict(sd)
    m = C.UNet(nc, 3, cd).to(DEV)
    m.load_state_dict(sd)
    m.train(); ref.train()
    kw = dict(lr=0.01, momentum=0.9, nesterov=True, weight_decay=1e-4)
    opt = C.FusedSGD(m.parameters(), **kw)
    ropt = torch.optim.SGD(ref.parameters(), **kw)
    lam = lambda n: (1 - n / 10) ** 0.9
    sch, rsch = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lam), torch.optim.lr_scheduler.LambdaLR(ropt, lr_lambda=lam)
    crit, rcrit = C.CrossEntropyLoss(), nn.CrossEntropyLoss()
    losses, rlosses = [], []
    for i in range(4):
        x = torch.from_numpy(C.synth.images(31, B, 3, H, W, first_image=B * i))
        y = torch.from_numpy(C.synth.labels(31, B, H, W, nc, first_image=B * i))
        out = m(x.to(DEV)); opt.zero_grad(); loss = crit(out, y.to(DEV)); loss.backward(); opt.step(); sch.step()
        losses.append(float(loss.detach()))
        _, rl = TC.train_step(ref, ropt, rcrit, x.double(), y)
        rsch.step()
        rlosses.append(float(rl.detach()))
    print('losses', losses, 'float64 torch', rlosses)
    np.testing.assert_allclose(losses, rlosses, rtol=2e-4)
    assert losses[-1] != losses[0]
    names = dict(m.named_parameters())
    for k, rp in ref.named_parameters():       # the optimiser's arithmetic is pinned per element above; here: every tensor has its buffer
        assert opt.state[names[k]]['momentum_buffer'].shape == rp.shape and opt.state[names[k]]['momentum_buffer'].any()


def _data(C, nc=4):
    return [(torch.from_numpy(C.synth.images(7, 2, 3, 32, 32, first_image=2 * i)),
             torch.from_numpy(C.synth.labels(7, 2, 32, 32, nc, first_image=2 * i))) for i in range(2)]


def test_trainer_with_sgd_and_the_iteration_schedule(C, tmp_path):
    data = _data(C)
    mk = lambda: C.default_config(optimizer='sgd', lr_schedule='iteration', conv_dim=4, num_classes=4, n_iters=2, lr=0.02,
                                  decay_norm_and_bias=False, compute_dtype='fp32', stats_every=1)
    torch.manual_seed(3)
    tr = C.Trainer(data, mk())
    assert isinstance(tr.optim, C.FusedSGD)
    g = tr.optim.param_groups[0]
    assert (g['momentum'], g['nesterov'], g['weight_decay']) == (0.9, True, 1e-4)
    bn_and_bias = {id(p) for n, p in tr.model.named_parameters() if p.dim() == 1}
    assert tr.optim._no_decay == bn_and_bias and 0 < len(bn_and_bias) < len(list(tr.model.parameters()))
    lrs = []
    tr.optim.pre_step_hooks.append(lambda: lrs.append(tr.optim.param_groups[0]['lr']))
    tr.train_val(epochs=1)
    # max_iters None: n_iters * len(loader) = 4
    np.testing.assert_allclose(lrs, [0.02 * (1 - n / 4) ** 0.9 for n in range(2)], rtol=1e-15)
    path = tr.save_network('unet', 'e1', 0, str(tmp_path))
    ck = torch.load(path, map_location='cpu', weights_only=False)
    # the saved optimiser state loads into torch.optim.SGD
    stock = torch.optim.SGD([nn.Parameter(p.detach().cpu().clone()) for p in tr.model.parameters()], lr=1.0)
    stock.load_state_dict(ck['optimizer_state'])
    sp = stock.param_groups[0]
    assert sp['momentum'] == 0.9 and sp['nesterov'] and sp['lr'] == pytest.approx(0.02 * 0.5 ** 0.9, rel=1e-15)
    for p, q in zip(sp['params'], tr.model.parameters()):
        assert torch.equal(stock.state[p]['momentum_buffer'], tr.optim.state[q]['momentum_buffer'].cpu())
    # one more step: the uninterrupted run against a fresh Trainer that loaded the checkpoint, bit for bit
    x, y = data[0][0].to(DEV), data[0][1].to(DEV)
    tr.train_step(x, y)
    tr2 = C.Trainer(data, mk())
    assert tr2.load_network('unet', 'e1', str(tmp_path))
    lrs2 = []
    tr2.optim.pre_step_hooks.append(lambda: lrs2.append(tr2.optim.param_groups[0]['lr']))
    tr2.train_step(x, y)
    assert lrs2 == [lrs[2]] and lrs[2] == pytest.approx(0.02 * 0.5 ** 0.9, rel=1e-15)
    for (k, a), (_, b) in zip(tr.model.state_dict().items(), tr2.model.state_dict().items()):
        assert torch.equal(a, b), k
    for a, b in zip(tr.model.parameters(), tr2.model.parameters()):
        assert torch.equal(_bits(tr.optim.state[a]['momentum_buffer']), _bits(tr2.optim.state[b]['momentum_buffer']))
    # a checkpoint written with the other optimiser is refused by name
    adam = C.Trainer(data, C.default_config(conv_dim=4, num_classes=4, n_iters=2, compute_dtype='fp32', stats_every=1))
    with pytest.raises(ValueError, match="'sgd'.*'adam'"):
        adam.load_network('unet', 'e1', str(tmp_path))
    # task 2: both anchor terms inside the SGD kernel, the head grown by one class
    head = [p for p in tr.model.parameters()][-2:]
    rows = head[0].shape[0]
    before = [tr.optim.state[p]['momentum_buffer'].clone() for p in head]
    tr.begin_task2(2, l2_lambda=0.1, ewc_lambda=0.5, new_classes=1)
    grown = [p for p in tr.model.parameters()][-2:]
    for p, b in zip(grown, before):
        buf = tr.optim.state[p]['momentum_buffer']
        assert p.shape[0] == rows + 1 and torch.equal(buf[:rows], b) and not buf[rows:].any()
    assert {id(p) for p in grown if p.dim() == 1} <= tr.optim._no_decay
    w0 = torch.cat([p.detach().flatten() for p in tr.model.parameters()]).clone()
    data5 = _data(C, 5)
    tr.train_step(data5[0][0].to(DEV), data5[0][1].to(DEV))
    tr.train_step(data5[1][0].to(DEV), data5[1][1].to(DEV))
    assert len(lrs) == 5 and lrs[3] == pytest.approx(0.02 * 0.25 ** 0.9) and lrs[4] == 0.0
    l2, ewc = float(tr.optim.l2_penalty()), float(tr.optim.consolidation_penalty())
    assert np.isfinite(l2) and l2 > 0 and np.isfinite(ewc) and ewc > 0, (l2, ewc)
    w1 = torch.cat([p.detach().flatten() for p in tr.model.parameters()])
    assert torch.isfinite(w1).all() and not torch.equal(w0, w1)


def test_default_trainer_is_the_fused_adam_loop_bit_for_bit(C):
    """A default-config Trainer (Adam, epoch schedule) against the loop it has always run, written out: two steps, the same bits."""
    data = _data(C)
    cfg = C.default_config(conv_dim=4, num_classes=4, n_iters=5, lr=1e-3, compute_dtype='fp32', stats_every=1)
    assert cfg.optimizer == 'adam' and cfg.lr_schedule == 'epoch'
    torch.manual_seed(4)
    tr = C.Trainer(data, cfg)
    assert isinstance(tr.optim, C.FusedAdam)
    m = C.UNet(4, 3, 4, compute_dtype='fp32').to(DEV)
    m.load_state_dict({k: v.detach().clone() for k, v in tr.model.state_dict().items()})
    opt = C.FusedAdam(m.parameters(), lr=1e-3, betas=[cfg.beta1, cfg.beta2])
    sch = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda n: (1 - n / cfg.n_iters) ** cfg.lr_exp)
    crit = C.CrossEntropyLoss().to(DEV)
    tr.train_val(epochs=1)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        sch.step()
    for x, y in data:
        out = m(x.to(DEV)); opt.zero_grad(); loss = crit(out, y.to(DEV)); loss.backward(); opt.step()
    assert opt.param_groups[0]['lr'] == tr.optim.param_groups[0]['lr']
    for (k, a), (_, b) in zip(tr.model.state_dict().items(), m.state_dict().items()):
        assert torch.equal(a, b), k
    for a, b in zip(tr.model.parameters(), m.parameters()):
        assert torch.equal(_bits(tr.optim.state[a]['exp_avg']), _bits(opt.state[b]['exp_avg']))
