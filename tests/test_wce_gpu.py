"""GPU: CrossEntropyLoss(weight=, label_smoothing=, focal_gamma=) under autograd, its hand-over of d logits to the UNet's backward pass, the
default path's library calls, and the Trainer with class weights / label smoothing (checkpoint round trip, set_class_weights, grow_head, a
pseudo-label task-2 step, the refused combinations).  The kernels themselves are held per element by tests/test_wce_grid_gpu.py."""
import math

import pytest
import torch

import wce_ref
from test_wce_grid_gpu import C_BOUND, DEV, EPS, MODES, _case, _reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    C._lib.load()
    return C


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('B,H,W', [(3, 8, 12), (2, 5, 7)])
def test_module_under_autograd(C, B, H, W, mode):
    cs = _case(21, B, H, W, 3.0, seed=11)
    eps, gamma = MODES[mode]
    crit = C.CrossEntropyLoss(weight=cs.wd.cpu(), label_smoothing=eps, focal_gamma=gamma).to(DEV)
    assert crit.weight.is_cuda
    for nu in (False, True):
        ref = _reference(cs, mode, nu)
        plain = None
        for up in (1.0, -2.5):
            z = cs.zd.clone().requires_grad_()
            loss = crit(z, cs.yd, cs.nud) if nu else crit(z, cs.yd)
            (loss * up).backward()
            torch.cuda.synchronize()
            assert abs(float(loss.detach()) - ref.l3[0]) < 1e-5 * max(1.0, abs(ref.l3[0]))
            assert [float(v) for v in crit.parts] == pytest.approx(ref.l3, rel=1e-5, abs=1e-5) and int(crit.bad_labels) == 2
            if plain is None:                   # upstream gradient 1: d logits as the kernel wrote it, under the grid file's bound
                plain = z.grad.clone()
                rk = float(((plain.double() - ref.grad).abs() / (EPS * ref.s_px[:, None]))[ref.live].max())
                assert rk <= C_BOUND[mode] and float(plain[~ref.live].abs().max()) == 0.0
            else:                               # any other: that tensor times the upstream gradient, one fp32 product per element
                assert torch.equal(z.grad, plain * torch.tensor(up, dtype=torch.float32, device=DEV))
    # smoothing or the focal term without weights: unit weights
    if mode != 'weights':
        unit = C.CrossEntropyLoss(label_smoothing=eps, focal_gamma=gamma)
        r1 = wce_ref.wce(cs.zd.double(), cs.yd, None, eps=eps, gamma=gamma)
        assert abs(float(unit(cs.zd, cs.yd)) - float(r1.l3[0])) < 1e-5 * max(1.0, abs(float(r1.l3[0])))
        ones = unit._unit                       # the unit vector is made once per (K, device), not per step
        unit(cs.zd, cs.yd)
        assert unit._unit is ones and ones.tolist() == [1.0] * 21
        unit(cs.zd[:, :20].contiguous(), cs.yd.clamp(max=19))
        assert unit._unit.numel() == 20
    with pytest.raises(ValueError, match='labels shape'):
        crit(cs.zd, cs.yd[:, :3])
    with pytest.raises(ValueError, match='20 classes'):
        crit(cs.zd[:, :20], cs.yd)
    with pytest.raises(ValueError, match='image_weight must be float32'):
        crit(cs.zd, cs.yd, cs.nud.double())


def _net_and_batch(C, seed=9):
    torch.manual_seed(seed)
    m = C.UNet(4, 3, 4, compute_dtype='fp32').to(DEV).train()
    x = torch.from_numpy(C.synth.images(8, 2, 3, 32, 32)).to(DEV)
    y = torch.from_numpy(C.synth.labels(8, 2, 32, 32, 4)).to(DEV)
    y[0, :2] = -100
    return m, x, y


W4 = [0.5, 2.0, 0.0, 1.25]


@pytest.mark.parametrize('mode', list(MODES))
def test_hand_over_to_the_unet(C, monkeypatch, mode):
    """d logits reaches the UNet's backward pass as the NHWC copy the loss kernel wrote (eng.dl_src is set) and, with the hand-over off, as
    the NCHW tensor the engine converts: the same parameter gradients bit for bit in fp32."""
    eps, gamma = MODES[mode]
    crit = C.CrossEntropyLoss(weight=torch.tensor(W4), label_smoothing=eps, focal_gamma=gamma).to(DEV)

    def run():
        m, x, y = _net_and_batch(C)
        out = m(x)
        eng = next(iter(m._engines.values()))
        loss = crit(out, y)
        taken = eng.dl_src is not None
        loss.backward()
        torch.cuda.synchronize()
        return torch.cat([p.grad.flatten() for p in m.parameters()]).clone(), taken, out.detach().clone(), float(loss)

    ga, taken_a, out, la = run()
    monkeypatch.setattr(C.loss, 'HANDOVER', False)
    gb, taken_b, _, lb = run()
    assert taken_a and not taken_b and la == lb
    assert torch.equal(ga.view(torch.int32), gb.view(torch.int32)) and bool(ga.any())
    y = _net_and_batch(C)[2]
    ref = float(wce_ref.wce(out.double(), y, torch.tensor(W4, device=DEV).double(), eps=eps, gamma=gamma).l3[0])
    assert abs(la - ref) < 1e-5 * max(1.0, abs(ref))


def test_defaults_issue_the_calls_they_always_did(C, monkeypatch):
    """CrossEntropyLoss() with its new arguments at their defaults: the entry points of the plain path, in their order, for the aligned, the
    image-weighted and the odd-sized forward and for the backward; the new entry point only with one of the three set."""
    names = []
    real_call, real_hbm = C.loss.call, C.unet._hbm

    def call(name, *a):
        names.append(name)
        return real_call(name, *a)

    def hbm(tag, nbytes, name, *a):
        names.append(name)
        return real_hbm(tag, nbytes, name, *a)

    monkeypatch.setattr(C.loss, 'call', call)
    monkeypatch.setattr(C.unet, '_hbm', hbm)
    cs, odd = _case(5, 2, 8, 12, 3.0), _case(5, 2, 5, 7, 3.0)

    def calls(crit, c, *extra):
        del names[:]
        z = c.zd.clone().requires_grad_()
        crit(z, c.yd, *extra).backward()
        torch.cuda.synchronize()
        return list(names)

    plain = C.CrossEntropyLoss()
    assert calls(plain, cs) == ['clamd_ce_count', 'clamd_ce_fwd_bwd_counted', 'clamd_scale_by_device_scalar']
    assert calls(plain, cs, cs.nud) == ['clamd_ce_count', 'clamd_ce_fwd_bwd_weighted', 'clamd_scale_by_device_scalar']
    assert calls(plain, odd) == ['clamd_ce_fwd_bwd', 'clamd_scale_by_device_scalar']
    assert calls(C.CrossEntropyLoss(255), cs) == ['clamd_ce_count', 'clamd_ce_fwd_bwd_counted', 'clamd_scale_by_device_scalar']
    for crit in (C.CrossEntropyLoss(weight=cs.wd), C.CrossEntropyLoss(label_smoothing=0.1), C.CrossEntropyLoss(focal_gamma=2.0)):
        for c, extra in ((cs, ()), (cs, (cs.nud,)), (odd, ())):
            assert calls(crit, c, *extra) == ['clamd_ce_class_fwd_bwd', 'clamd_scale_by_device_scalar']


def _data(C, nc=4):
    return [(torch.from_numpy(C.synth.images(7, 2, 3, 32, 32, first_image=2 * i)),
             torch.from_numpy(C.synth.labels(7, 2, 32, 32, nc, first_image=2 * i))) for i in range(2)]


@pytest.mark.parametrize('kw', [dict(class_weights=W4), dict(label_smoothing=0.1), dict(class_weights=W4, focal_gamma=2.0)],
                         ids=['class_weights', 'label_smoothing', 'weights+focal'])
def test_trainer(C, tmp_path, kw):
    data = _data(C)
    mk = lambda: C.default_config(conv_dim=4, num_classes=4, n_iters=3, lr=1e-3, compute_dtype='fp32', stats_every=1, **kw)
    torch.manual_seed(5)
    tr = C.Trainer(data, mk())
    assert tr.class_criterion_active() and type(tr.likelihood_loss) is C.CrossEntropyLoss and not tr.likelihood_loss.generalised
    w = None if 'class_weights' not in kw else torch.tensor(W4, device=DEV).double()
    rkw = dict(eps=kw.get('label_smoothing', 0.0), gamma=kw.get('focal_gamma', 0.0))
    losses = []
    for _ in range(2):
        for x, y in data:
            out, loss = tr.train_step(x.to(DEV), y.to(DEV))
            ref = float(wce_ref.wce(out.detach().double(), y.to(DEV), w, **rkw).l3[0])
            assert abs(float(loss) - ref) <= 1e-5 * abs(ref), (float(loss), ref)
            assert int(tr.c_loss.bad_labels) == 0 and float(tr.c_loss.parts[0]) == float(loss)
            losses.append(float(loss))
    assert all(math.isfinite(v) for v in losses) and losses[-1] != losses[0]
    # a checkpoint round trip: one more step of the uninterrupted run against a fresh Trainer that loaded the file, bit for bit.  The
    # weights in the file are the ACTIVE ones (changed here after construction), not the configuration's
    if w is not None:
        tr.set_class_weights([1.5, 0.25, 1.0, 3.0])
    tr.save_network('unet', 'e1', 0, str(tmp_path))
    x, y = data[0][0].to(DEV), data[0][1].to(DEV)
    _, la = tr.train_step(x, y)
    tr2 = C.Trainer(data, mk())
    assert tr2.load_network('unet', 'e1', str(tmp_path))
    if w is not None:
        assert tr2.class_weight.tolist() == [1.5, 0.25, 1.0, 3.0]
    _, lb = tr2.train_step(x, y)
    assert float(la) == float(lb)
    for (k, a), (_, b) in zip(tr.model.state_dict().items(), tr2.model.state_dict().items()):
        assert torch.equal(a, b), k
    assert tr.estimate_importance(data, max_batches=1) is not None          # on the plain log-likelihood
    with pytest.raises(ValueError, match='distill_lambda > 0'):
        tr.begin_task2(2)
    with pytest.raises(ValueError, match='unbiased=True'):
        tr.begin_task2(2, distill_lambda=0.0, unbiased=True)
    assert tr.old_model is None


def test_trainer_checkpoint_without_the_key_and_scheme_weights(C, tmp_path):
    data = _data(C)
    mk = lambda **kw: C.default_config(conv_dim=4, num_classes=4, n_iters=3, lr=1e-3, compute_dtype='fp32', stats_every=1, **kw)
    torch.manual_seed(5)
    plain = C.Trainer(data, mk())
    plain.train_step(data[0][0].to(DEV), data[0][1].to(DEV))
    snap = plain.snapshot(0)
    snap.pop('_event').synchronize()
    assert 'class_weight_state' not in snap
    plain.save_network('unet', 'e0', 0, str(tmp_path))
    tr = C.Trainer(data, mk(class_weights=W4))
    assert tr.load_network('unet', 'e0', str(tmp_path)) and tr.class_weight.tolist() == W4      # a file without the key: the configuration's stay
    # a scheme and a loader: the counts taken on the device equal the host's
    host = torch.cat([torch.stack([(masks == k).sum((1, 2)) for k in range(4)], 1) for _, masks in data])
    for scheme in ('median_frequency', 'inverse_log'):
        got = tr.set_class_weights(scheme, data)
        assert got.is_cuda and torch.equal(got.cpu(), C.class_weights(host, scheme)) and tr.c_loss.weight is got
    # grow_head extends the vector with ones; the pseudo-label task step composes through the image weight
    before = tr.class_weight.clone()
    tr.begin_task2(4, distill_lambda=0.0, pseudo_label=True, pseudo_adaptive=True, new_classes=2)
    assert tr.cfg.num_classes == 6 and torch.equal(tr.class_weight, torch.cat([before, before.new_ones(2)]))
    x, y = data[0][0].to(DEV), data[0][1].to(DEV).clone()
    y[:, :4] = 5
    w0 = torch.cat([p.detach().flatten() for p in tr.model.parameters()]).clone()
    out, loss = tr.train_step(x, y)
    assert out.shape[1] == 6 and math.isfinite(float(loss)) and float(loss) > 0
    w1 = torch.cat([p.detach().flatten() for p in tr.model.parameters()])
    assert bool(torch.isfinite(w1).all()) and not torch.equal(w0, w1)
    assert tr.set_class_weights([1, 1, 2, 2, 3, 3]).numel() == 6
    with pytest.raises(ValueError, match="loss='ce_dice' with class_weights"):
        C.Trainer(data, mk(loss='ce_dice', label_smoothing=0.1))
