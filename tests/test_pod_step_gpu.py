"""GPU: Local POD above the C ABI -- LocalPODLoss through autograd, the task step with the logits-level term (Trainer.begin_task2(pod_lambda=)),
and the feature level through a block that runs on its own (blocks.py).  The references are the float64 / float32 restatements of
tests/test_pod_cpu.py; the tolerances are those of the tests named at each check."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_pod_cpu import pod_closed_form, pod_loss

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)


@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    C._lib.load()
    return C


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def test_module_through_autograd(C):
    torch.manual_seed(3)
    a = torch.randn(2, 5, 8, 16, device=DEV, requires_grad=True)
    b = torch.randn(2, 3, 8, 16, device=DEV, requires_grad=True)
    pod = C.LocalPODLoss(levels=3, lam=0.7)
    loss = pod(a, b, channels=3, merge_extra=True)
    want_loss, want, _ = pod_closed_form(a.detach().cpu().double(), b.detach().cpu().double(), 3, True, False, True, 3, 0.7)
    assert float(loss.detach()) == pytest.approx(float(want_loss), rel=1e-5)
    loss.backward()
    assert b.grad is None, 'old is detached'
    unit = a.grad.clone()
    assert rel_l2(unit.cpu().numpy(), want.numpy()) < 1e-5
    a.grad = None
    (0.5 * pod(a, b, channels=3, merge_extra=True)).backward()          # an upstream gradient of 0.5: a power of two, so exactly half
    assert torch.equal(a.grad, 0.5 * unit)
    # a forward whose result is dropped keeps nothing: the kept gradient and the workspace go with the graph
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    out = pod(a, b, channels=3, merge_extra=True)
    assert torch.cuda.memory_allocated() > before
    del out
    assert torch.cuda.memory_allocated() == before
    with torch.no_grad():                                                  # no gradient wanted: the loss alone, the same bits
        assert torch.equal(pod(a, b, channels=3, merge_extra=True), loss.detach())
    with pytest.raises(ValueError, match='channels must be in'):
        pod(a, b, channels=4)
    with pytest.raises(ValueError, match='multiples of'):
        pod(a[:, :, :6], b[:, :, :6])


def _batches(C, n, K):
    return [(torch.from_numpy(C.synth.images(20 + i, 2, 3, 32, 32)).to(DEV), torch.from_numpy(C.synth.labels(20 + i, 2, 32, 32, K)).to(DEV))
            for i in range(n)]


def _task2_run(C, pod_lambda, log=None, check=False):
    """UNet(3 -> 5, 3, 8) at 32x32, bs2: one task-1 step, begin_task2(3, distill_lambda=0, new_classes=2, pod_lambda), two task-2 steps.
    -> per step (loss, every parameter gradient), and the final weights."""
    torch.manual_seed(7)
    cfg = C.default_config(n_iters=100, lr=1e-3, num_classes=3, conv_dim=8, stats_every=1)
    task1, task2 = _batches(C, 1, 3), _batches(C, 2, 5)
    tr = C.Trainer(task1, cfg)
    tr.train_step(*task1[0])
    tr.begin_task2(3, distill_lambda=0, new_classes=2, pod_lambda=pod_lambda)
    assert (tr.pod is not None) == (pod_lambda > 0) and tr.model.num_classes == 5
    steps = []
    for x, y in task2:
        state = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
        if log is not None:
            log.clear()
        outputs, loss = tr.train_step(x, y)
        grads = [p.grad.detach().clone() for p in tr.model.parameters()]
        steps.append((loss.detach().clone(), grads))
        if check:
            # the same logits: the criterion's loss plus the restatement's term (tests/test_incremental_gpu.py's step tolerance, fp32: 2e-3)
            with torch.no_grad():
                old = tr.old_model(x)
            z = outputs.detach()
            ce = F.cross_entropy(z, y)
            term, dpod, _ = pod_closed_form(z.cpu().double(), old.cpu().double(), 3, True, False, True, 3, pod_lambda)
            print(f'task-2 step: ours {float(loss):.6f}, cross-entropy {float(ce):.6f} + POD {float(term):.6f}')
            assert float(loss) == pytest.approx(float(ce) + float(term), rel=2e-3, abs=2e-5)
            # the engine handed the summed NCHW gradient, at the weights (and running statistics) the step started from
            m2 = C.UNet(5, 3, 8).to(DEV).train()
            m2.load_state_dict(state)
            zz = z.clone().requires_grad_()
            dce, = torch.autograd.grad(F.cross_entropy(zz, y), zz)
            out2 = m2(x)
            assert rel_l2(out2.detach().cpu().numpy(), z.cpu().numpy()) < 1e-6, 'the second model does not start where the step started'
            out2.backward(dce + dpod.float().to(DEV))
            rels = {}
            for (n_, p), g in zip(m2.named_parameters(), grads):
                if float(p.grad.norm()) > 1e-6:          # conv biases in front of a train-mode BatchNorm have ~0 gradient
                    rels[n_] = rel_l2(g.cpu().numpy(), p.grad.cpu().numpy())
            print('gradient rel_l2 per tensor:', {k: f'{v:.2e}' for k, v in rels.items()})
            assert len(rels) >= 20 and max(rels.values()) < 2e-3, max(rels.items(), key=lambda kv: kv[1])
    return steps, [p.detach().clone() for p in tr.model.parameters()]


def test_task_step_with_pod(C, monkeypatch):
    calls = []
    real = C.unet._hbm

    def logged(family, nbytes, name, *args):
        calls.append(name)
        real(family, nbytes, name, *args)

    monkeypatch.setattr(C.unet, '_hbm', logged)
    first, w1 = _task2_run(C, 0.5, log=calls, check=True)
    assert calls.count('clamd_local_pod_fwd_bwd') == 1, calls            # the last step's launches
    second, w2 = _task2_run(C, 0.5)
    for (l1, g1), (l2, g2) in zip(first, second):
        assert torch.equal(l1, l2) and all(torch.equal(a, b) for a, b in zip(g1, g2)), 'two runs of the step differ'
    assert all(torch.equal(a, b) for a, b in zip(w1, w2))
    plain, _ = _task2_run(C, 0.0, log=calls)
    assert 'clamd_local_pod_fwd_bwd' not in calls and any(n.startswith('clamd_ce_') for n in calls), calls
    assert not torch.equal(plain[0][0], first[0][0])


def test_feature_level_through_a_block(C):
    """LocalPODLoss(square=True) on model.enc1(x) against the stock-torch block plus the restatement (conv_dim 8, 16x16); the bounds of
    tests/test_unet_gpu.py::test_blocks_run_on_their_own (fp32: 2e-5 on the output, 2e-3 on the gradients)."""
    from oracle import torch_cpu as TC
    torch.manual_seed(11)
    m = C.UNet(5, 3, 8).to(DEV).train()
    ref = TC.build_unet(5, 3, 8).to(DEV).train()
    ref.load_state_dict(m.state_dict())
    old = TC.build_unet(5, 3, 8).to(DEV).eval()
    x = torch.randn(2, 3, 16, 16, device=DEV)
    with torch.no_grad():
        fo = old.enc1(x)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    fa, fb = m.enc1(xa), ref.enc1(xb)
    assert rel_l2(fa.detach().cpu().numpy(), fb.detach().cpu().numpy()) < 2e-5
    la = C.LocalPODLoss(square=True)(fa, fo)
    lb = pod_loss(fb, fo, fo.shape[1], False, True, True, 3, 1.0)
    assert float(la.detach()) == pytest.approx(float(lb.detach()), rel=1e-4)
    la.backward(); lb.backward()
    gtol = 2e-3
    assert rel_l2(xa.grad.cpu().numpy(), xb.grad.cpu().numpy()) < gtol
    pa, pb = dict(m.enc1.named_parameters()), dict(ref.enc1.named_parameters())
    assert list(pa) == list(pb)
    for k in pa:
        r = pb[k].grad
        assert float((pa[k].grad - r).norm()) <= gtol * float(r.norm()) + 1e-6 * r.numel() ** 0.5, k
    ga, gb = (torch.cat([d[k].grad.reshape(-1) for k in pa]) for d in (pa, pb))
    assert float((ga - gb).norm() / gb.norm()) < gtol
