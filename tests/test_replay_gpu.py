"""GPU: exemplar replay -- the three kernels against numpy / torch restatements (exact: they move and count integers, copy bits, and decode
with the data path's arithmetic), the sampler's determinism, the task step with a memory against the same step fed the mixed batches, and
the checkpoint.  Shapes: 16 x 16 takes the four-pixel path, 5 x 7 the one-pixel path inside less than a workgroup, 32 x 48 / 64 x 80 several
workgroups per image."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
K = 6                      # classes of the store tests: capacity 5 covers the five foreground classes
SHAPES = [(16, 16), (5, 7), (32, 48)]
QTOL = 1 / 255 + 1e-6      # half a quantisation step in x units (tests/test_replay_cpu.py::test_quantisation_error_is_half_a_step)


@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    C._lib.load()
    return C


def _labels(B, H, W, k, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, k, (B, H, W), generator=g)
    y[torch.rand(B, H, W, generator=g) < 0.1] = -100
    return y


def _byte_images(B, H, W, seed):
    """data.prepare_sample's formula (ToTensor, Normalize(0.5, 0.5)) on random bytes, in float32 on the host."""
    u = torch.randint(0, 256, (B, 3, H, W), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    return (u.float() / 255.0 - 0.5) / 0.5


def _memory(C, H, W, storage='uint8', **kw):
    return C.ReplayMemory(K, (3, H, W), storage=storage, **kw).add_task((1, K), 5)


SRC1, SLOTS1 = [0, 1, 2, 3], [3, 0, 4, 1]          # out of order
SRC2, SLOTS2 = [2, 3], [0, 2]                      # slot 0 overwritten, slot 2 filled last
HELD = [2, 3, 3, 0, 2]                             # the batch image each slot ends up holding


def _stored(C, x, y, storage, labels_view=False):
    B, _, H, W = x.shape
    mem = _memory(C, H, W, storage)
    xd, yd = x.to(DEV), y.to(DEV)
    if labels_view:       # the same labels one element into a larger buffer: 8-byte aligned only, the one-pixel path
        buf = torch.empty(B * H * W + 1, dtype=torch.int64, device=DEV)
        yd = buf[1:].view(B, H, W).copy_(yd)
        assert yd.data_ptr() % 32 == 8 and yd.is_contiguous()
    mem.store(xd, yd, SRC1, SLOTS1)
    mem.store(xd, yd, SRC2, SLOTS2)
    torch.cuda.synchronize()
    return mem


# ------------------------------------------------------------------------------------------------------------------------------ counts
@pytest.mark.parametrize('H,W', [(16, 16), (5, 7), (64, 80)])
def test_class_pixel_counts(C, H, W):
    B, k = 3, 21
    y = _labels(B, H, W, k, seed=H)
    y[0, 0, 0], y[1, H - 1, W - 1], y[2, 1, 2], y[2, 2, 1] = k, -1, k, 1000
    want = np.stack([np.bincount(im[(im >= 0) & (im < k)], minlength=k) for im in y.numpy().reshape(B, -1)])
    counts = C.class_pixel_counts(y.to(DEV), k)
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (B, k)
    assert np.array_equal(counts.cpu().numpy(), want)
    assert int(counts.bad_labels) == 4
    assert int(want.sum()) + 4 + int((y == -100).sum()) == B * H * W


# ------------------------------------------------------------------------------------------------------------------------ store -> gather
@pytest.mark.parametrize('H,W', SHAPES)
def test_store_then_gather(C, H, W):
    y = _labels(4, H, W, K, seed=W)
    # uint8 storage of images that came from bytes: bit-identical
    x = _byte_images(4, H, W, seed=H)
    mem = _stored(C, x, y, 'uint8')
    gx, gy = mem.gather(list(range(5)))
    assert gx.dtype == torch.float32 and gy.dtype == torch.int64
    assert torch.equal(gx.cpu(), x[HELD]) and torch.equal(gy.cpu(), y[HELD])
    assert int(mem.bad_labels) == 0 and int(mem.bad_slots) == 0
    # ... through the one-pixel path (labels at a storage offset of one element): the same store
    view = _stored(C, x, y, 'uint8', labels_view=True)
    assert torch.equal(view.images, mem.images) and torch.equal(view.labels, mem.labels)
    # fp32 storage: the bits, whatever they are
    xr = torch.randn(4, 3, H, W, generator=torch.Generator().manual_seed(1)) * 3
    mem = _stored(C, xr, y, 'fp32')
    gx, gy = mem.gather(list(range(5)))
    assert torch.equal(gx.cpu().view(torch.int32), xr[HELD].view(torch.int32)) and torch.equal(gy.cpu(), y[HELD])
    # uint8 storage of arbitrary images in [-1, 1): half a quantisation step
    xs = torch.from_numpy(C.synth.images(1234, 4, 3, H, W))
    gx, gy = _stored(C, xs, y, 'uint8').gather(list(range(5)))
    err = float((gx.cpu() - xs[HELD]).abs().max())
    print(f'{H}x{W}: max |gather - x| = {err:.7f} (bound {QTOL:.7f})')
    assert err <= QTOL and torch.equal(gy.cpu(), y[HELD])


def test_store_counts_labels_that_are_no_class(C):
    y = _labels(4, 16, 16, K, seed=2)
    y[1, 3, 3], y[1, 4, 4] = K, -1
    mem = _stored(C, _byte_images(4, 16, 16, 3), y, 'uint8')
    assert int(mem.bad_labels) == 2                     # image 1 was stored once
    want = y[HELD].clone()
    want[(want < 0) | (want >= K)] = -100
    assert torch.equal(mem.gather(list(range(5)))[1].cpu(), want)
    with pytest.raises(ValueError, match='distinct'):
        mem.store(torch.zeros(4, 3, 16, 16, device=DEV), y.to(DEV), [0, 1], [2, 2])
    with pytest.raises(ValueError, match='slots in'):
        mem.store(torch.zeros(4, 3, 16, 16, device=DEV), y.to(DEV), [0], [5])


# ------------------------------------------------------------------------------------------------------------------------------- flips
@pytest.mark.parametrize('storage', ['uint8', 'fp32'])
@pytest.mark.parametrize('H,W', SHAPES)
def test_flips(C, H, W, storage):
    mem = _stored(C, _byte_images(4, H, W, seed=7), _labels(4, H, W, K, seed=8), storage)
    slots = [4, 0, 3]
    x0, y0 = mem.gather(slots)
    assert all(torch.equal(a, b) for a, b in zip(mem.gather(slots, [0, 0, 0]), (x0, y0)))
    for code, dims in ((1, (-1,)), (2, (-2,)), (3, (-2, -1))):
        x, y = mem.gather(slots, [code] * 3)
        assert torch.equal(x, torch.flip(x0, dims)) and torch.equal(y, torch.flip(y0, dims)), code
    x, y = mem.gather(slots, [2, 0, 1])                    # a code per exemplar
    assert torch.equal(x[0], torch.flip(x0[0], (-2,))) and torch.equal(x[1], x0[1]) and torch.equal(y[2], torch.flip(y0[2], (-1,)))


# --------------------------------------------------------------------------------------------------------------------------------- mix
def _filled_pair(C, n=2, **kw):
    """n memories with the same seed, offered the same three batches through the policy."""
    mems = [C.ReplayMemory(K, (3, 16, 16), **kw).add_task((1, K), 5) for _ in range(n)]
    for i in range(3):
        x = torch.from_numpy(C.synth.images(40 + i, 4, 3, 16, 16)).to(DEV)
        y = torch.from_numpy(C.synth.labels(40 + i, 4, 16, 16, K, cell=8)).to(DEV)
        for m in mems:
            m.observe(x, y)
    return [m.finish() for m in mems]


def test_mix(C):
    a, b = _filled_pair(C, seed=11)
    assert a.n_filled >= 2 and torch.equal(a.images, b.images) and torch.equal(a.filled, b.filled)
    x, y = _byte_images(2, 16, 16, 5).to(DEV), _labels(2, 16, 16, K, 6).to(DEV)
    mx, my = a.mix(x, y, 3)
    assert tuple(mx.shape) == (5, 3, 16, 16) and tuple(my.shape) == (5, 16, 16)
    assert torch.equal(mx[:2], x) and torch.equal(my[:2], y)
    slots, flips = b.draw(3)                                # the twin's generator gives what a drew
    gx, gy = a.gather(slots, flips)
    assert torch.equal(mx[2:], gx) and torch.equal(my[2:], gy)
    assert set(slots.tolist()) <= set(a.filled.tolist())
    rx, ry = a.mix(x, y, 0)
    assert rx is x and ry is y
    assert int(a.bad_slots) == 0


def test_slot_guard(C):
    mem = _stored(C, _byte_images(4, 16, 16, 1), _labels(4, 16, 16, K, 2), 'uint8')
    x, y = mem.gather([1, 5])                               # slot == capacity: handled by the kernel, a zero image and all-ignore labels
    assert float(x[1].abs().max()) == 0.0 and bool((y[1] == -100).all())
    assert torch.equal(x[0], mem.gather([1])[0][0])
    assert int(mem.bad_slots) == 1


def test_same_seed_same_draws(C):
    a, b = _filled_pair(C, seed=3)
    c, = _filled_pair(C, n=1, seed=4)
    da = [a.draw(4) for _ in range(5)]
    db = [b.draw(4) for _ in range(5)]
    assert all(torch.equal(s1, s2) and torch.equal(f1, f2) for (s1, f1), (s2, f2) in zip(da, db))
    assert any(int(f.max()) > 0 for _, f in da) and all(0 <= int(f.min()) and int(f.max()) < 4 for _, f in da)
    dc = [c.draw(4) for _ in range(5)]
    assert not all(torch.equal(s1, s2) and torch.equal(f1, f2) for (s1, f1), (s2, f2) in zip(da, dc))
    nf, = _filled_pair(C, n=1, seed=3, flip=False)
    assert int(nf.draw(4)[1].abs().max()) == 0


# --------------------------------------------------------------------------------------------------------------------------- task step
def _batches(C, n, k):
    return [(torch.from_numpy(C.synth.images(20 + i, 2, 3, 32, 32)).to(DEV), torch.from_numpy(C.synth.labels(20 + i, 2, 32, 32, k)).to(DEV))
            for i in range(n)]


def _task2_run(C, replay, log=None):
    """UNet(3 -> 5, 3, 8) at 32x32, bs2: one task-1 step, begin_task2(3, distill_lambda=0, new_classes=2), two task-2 steps -- with the
    trainer's own memory (replay=True), or without one, fed the batches a twin memory mixes (replay=False).
    -> the trainer, per step (loss, every parameter gradient, outputs.shape[0]), the final weights."""
    torch.manual_seed(7)
    cfg = C.default_config(n_iters=100, lr=1e-3, num_classes=3, conv_dim=8, stats_every=1)
    task1, task2 = _batches(C, 1, 3), _batches(C, 2, 5)
    tr = C.Trainer(task1, cfg)
    tr.train_step(*task1[0])
    twin = None
    if replay:
        tr.begin_task2(3, distill_lambda=0, new_classes=2, replay=4, replay_batch=2, replay_loader=task1, replay_flip=False)
        assert tr.replay is not None and tr.replay.capacity == 4 and tr.replay_boundary == 3
    else:
        tr.begin_task2(3, distill_lambda=0, new_classes=2)
        assert tr.replay is None
        twin = C.ReplayMemory(3, (3, 32, 32), flip=False, seed=0).add_task((1, 3), 4).fill(task1, DEV)
    assert tr.model.num_classes == 5
    steps = []
    for x, y in task2:
        if log is not None:
            log.clear()
        if twin is not None:
            x, y = twin.mix(x, y, 2)
            if log is not None:
                log.clear()
        outputs, loss = tr.train_step(x, y)
        steps.append((loss.detach().clone(), [p.grad.detach().clone() for p in tr.model.parameters()], outputs.shape[0]))
    return tr, steps, [p.detach().clone() for p in tr.model.parameters()]


def test_task_step_with_replay(C, monkeypatch):
    calls = []
    real = C.unet._hbm

    def logged(family, nbytes, name, *args):
        calls.append(name)
        real(family, nbytes, name, *args)

    monkeypatch.setattr(C.unet, '_hbm', logged)
    tr, first, w1 = _task2_run(C, True, log=calls)
    assert calls.count('clamd_replay_mix') == 1, calls          # the last step's launches
    assert tr.replay.n_filled >= 1 and int(tr.replay.bad_slots) == 0 and int(tr.replay.bad_labels) == 0
    _, second, w2 = _task2_run(C, False, log=calls)
    assert 'clamd_replay_mix' not in calls and any(n.startswith('clamd_ce_') for n in calls), calls
    for (l1, g1, n1), (l2, g2, n2) in zip(first, second):
        assert n1 == n2 == 4
        assert torch.equal(l1, l2), (float(l1), float(l2))
        assert all(torch.equal(a, b) for a, b in zip(g1, g2)), 'the step on the mixed batch differs from the step with the memory'
    assert all(torch.equal(a, b) for a, b in zip(w1, w2))
    # the epoch loop: statistics of the caller's rows against the caller's labels
    tr.train_data_loader = _batches(C, 2, 5)
    stats = tr.train_epoch(0)
    assert set(stats) >= {'loss', 'pixel_acc', 'mean_iu'} and np.isfinite(stats['loss']) and 0.0 <= stats['pixel_acc'] <= 100.0


def test_checkpoint_carries_the_memory(C, tmp_path):
    torch.manual_seed(7)
    task1 = _batches(C, 2, 3)
    tr = C.Trainer(task1, C.default_config(n_iters=100, lr=1e-3, num_classes=3, conv_dim=8))
    tr.train_step(*task1[0])
    tr.begin_task2(3, distill_lambda=0, replay=4, replay_batch=2, replay_storage='fp32')
    x, y = task1[1]
    tr.replay.mix(x, y, 2)                                   # the generator has moved on before the checkpoint
    tr.save_network('unet', 'r', 0, str(tmp_path))
    fresh = C.Trainer(task1, C.default_config(n_iters=100, lr=1e-3, num_classes=3, conv_dim=8))
    assert fresh.replay is None
    assert fresh.load_network('unet', 'r', str(tmp_path))
    assert fresh.replay_batch == 2 and fresh.replay_boundary == 3 and fresh.replay.storage == 'fp32'
    assert fresh.replay.n_filled == tr.replay.n_filled and torch.equal(fresh.replay.images, tr.replay.images)
    for _ in range(2):
        a, b = tr.replay.mix(x, y, 2), fresh.replay.mix(x, y, 2)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
