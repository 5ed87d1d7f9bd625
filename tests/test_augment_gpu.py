"""GPU: clamd_augment_batch against the numpy restatement of its definition (tests/augment_ref.py) on every element -- labels equal,
images within a bound derived below, padding exact --, the bit-level cases (identity, flip, the one-pixel path against the four-pixel path),
the step guard and the host refusals, the sampler's determinism, and the task step with augmentation against the same step fed the augmented
batches.  Shapes: 16 x 16 takes the four-pixel path, 5 x 7 the one-pixel path inside less than a workgroup, 32 x 48 several workgroups, and
836 x 840 a second grid-stride trip (test_second_grid_stride_trip).

The image bound, |out - ref| <= 16 * 2^-24 * M with M the largest magnitude among the element's four taps.  u = 2^-24 is fp32's unit
roundoff; the weights are exact (16-bit integers times 2^-16).  A horizontal lerp a + w * (b - a), 0 <= w < 1: the difference is at most 2M
and rounds by at most 2uM; the product carries that through (at most 2uM more of its own rounding); the sum is at most M(1 + 4u) and rounds
by at most uM: 5uM in all, to first order in u, and one rounding fewer where the compiler contracts the product and the sum into an fma.
The vertical lerp is a convex combination of two values each within 5uM of their exact ones, so it carries at most 5uM through, and adds at
most 5uM of its own by the same count: 10uM.  16 is that figure rounded up to a power of two (and covers the second-order terms).  The
restatement itself is float64 (error ~ 2^-53 M)."""
import numpy as np
import pytest
import torch

from augment_ref import augment_ref

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
U = 2.0 ** -24
FILL, IGN = -2.5, 255                 # neither occurs in the inputs: padding is told from copied pixels
POISON_I, POISON_L = 0x7FC0DEAD, -777777
GUARD = 64                            # elements before and behind every output: a multiple of 4, the alignment of the buffer is kept
ONE = 65536
IDENT, FLIP = (ONE, 0, 0, 0), (ONE, 0, 0, 1)


@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    C._lib.load()
    return C


def _inputs(B, Cc, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cc, H, W, generator=g) * 3
    x[B // 2, :, H // 2, :] *= 1e4 / 3                       # one row of large values
    y = torch.randint(0, 21, (B, H, W), generator=g)
    y[torch.rand(B, H, W, generator=g) < 0.1] = -100
    return x, y


def _out_buffers(x, y, guard=GUARD):
    """Outputs inside poisoned guard bands -> (image buffer, image view, label buffer, label view)."""
    bx = torch.full((x.numel() + 2 * guard,), POISON_I, dtype=torch.int32, device=DEV).view(torch.float32)
    by = torch.full((y.numel() + 2 * guard,), POISON_L, dtype=torch.int64, device=DEV)
    return bx, bx[guard:guard + x.numel()].view(x.shape), by, by[guard:guard + y.numel()].view(y.shape)


def _launch(C, x, y, rows, guard=GUARD, inputs=None, fill=FILL, ign=IGN):
    """One launch into guarded outputs -> (images, labels) on the host and the guard counter; the bands must be intact."""
    xd, yd = inputs if inputs is not None else (x.to(DEV), y.to(DEV))
    bx, ox, by, oy = _out_buffers(x, y, guard)
    params = torch.tensor(rows, dtype=torch.int64).to(DEV)
    rx, ry = C.augment_batch(xd, yd, params, fill, ign, out=(ox, oy))
    assert rx is ox and ry is oy
    torch.cuda.synchronize()
    ib = bx.view(torch.int32)
    assert bool((ib[:guard] == POISON_I).all()) and bool((ib[guard + x.numel():] == POISON_I).all()), 'image guard band overwritten'
    assert bool((by[:guard] == POISON_L).all()) and bool((by[guard + y.numel():] == POISON_L).all()), 'label guard band overwritten'
    return ox.cpu(), oy.cpu(), int(ry.bad_params)


def _check(tag, gx, gy, x, y, rows, fill=FILL, ign=IGN):
    """Every element against the restatement: labels equal, images within 16 u M (M = 0 outside: padding is exactly fill)."""
    rx, ry, inside, M = augment_ref(x.numpy(), y.numpy(), rows, fill, ign)
    assert np.array_equal(gy.numpy(), ry), f'{tag}: labels differ at {int((gy.numpy() != ry).sum())} pixels'
    assert (ry[~inside] == ign).all()
    err = np.abs(gx.numpy().astype(np.float64) - rx)
    bound = 16 * U * M
    ratio = float((err[M > 0] / bound[M > 0]).max()) if (M > 0).any() else 0.0
    print(f'{tag}: {int(inside.sum())}/{inside.size} pixels inside, max |out - ref| / (16 u M) = {ratio:.4f}')
    assert (err <= bound).all(), f'{tag}: {int((err > bound).sum())} elements beyond the bound, worst ratio {ratio:.3f}'
    return ratio


def _rows(H, W):
    """Hand-made params, in launches of three."""
    mid = ((1 << 24) + 166) // 333                          # scale 333 / 256
    return {
        'identity, flip, both at a fraction': [IDENT, FLIP, (ONE, 1, -1, 1)],
        'step 2^13 and 2^19': [(1 << 13, H * ONE // 3, W * ONE // 5, 1), (1 << 19, H * 32768 - (H // 2) * (1 << 19) - 32768, W * 32768 - (W // 2) * (1 << 19) - 32768, 0),
                               (1 << 13, -3 * 8192 - 4096, (W - 1) * ONE + 20000, 0)],
        'zoom-out, fill on all four sides': [(98304, -H * 16384 - 16384, -W * 16384 - 16384, 0), (98304, -H * 16384 - 16384, -W * 16384 - 16384, 1),
                                             (2 * ONE, -H * 32768 + 5, -W * 32768 + 77, 1)],
        'half out on each side': [(ONE, -(H // 2) * ONE + 1, 0, 0), (ONE, (H // 2) * ONE + 32767, 12345, 1), (ONE, 54321, -(W // 2) * ONE + 32768, 0)],
        'half out right, fractions': [(ONE, -7, (W // 2) * ONE + 65535, 1), (ONE, 32767, -32767, 0), (ONE, 32768, 32768, 1)],
        'fractions and mid scales': [(ONE, 65535, -65535, 0), (mid, 3 * ONE + 32768, 2 * ONE + 1, 1), (43691, H * 8192 + 32767, W * 9000 + 65535, 0)],
    }


# ----------------------------------------------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize('H,W', [(16, 16), (5, 7), (32, 48)])
def test_every_element_against_the_restatement(C, H, W):
    x, y = _inputs(3, 3, H, W, seed=H * 64 + W)
    xd, yd = x.to(DEV), y.to(DEV)
    for name, rows in _rows(H, W).items():
        gx, gy, bad = _launch(C, x, y, rows, inputs=(xd, yd))
        assert bad == 0
        _check(f'{H}x{W} {name}', gx, gy, x, y, rows)
    fractions = {r[1] & 65535 for rows in _rows(H, W).values() for r in rows}
    assert {1, 32767, 32768, 65535} <= fractions


def test_single_channel_and_defaults(C):
    """C = 1, and the default fill / ignore_index with fresh outputs."""
    x, y = _inputs(3, 1, 16, 16, seed=3)
    rows = [(98304, -16 * 16384 - 16384, -16 * 16384, 1), (43691, 70000, 90001, 0), FLIP]
    gx, gy, bad = _launch(C, x, y, rows)
    _check('16x16 C=1', gx, gy, x, y, rows)
    ox, oy = C.augment_batch(x.to(DEV), y.to(DEV), torch.tensor(rows).to(DEV))
    _check('16x16 C=1 defaults', ox.cpu(), oy.cpu(), x, y, rows, 0.0, -100)
    assert int(oy.bad_params) == 0 and ox.bad_params is oy.bad_params
    # either half alone
    only_x, none = C.augment_batch(x.to(DEV), None, torch.tensor(rows).to(DEV))
    assert none is None and torch.equal(only_x, ox)
    none, only_y = C.augment_batch(None, y.to(DEV), torch.tensor(rows).to(DEV))
    assert none is None and torch.equal(only_y, oy)


def test_second_grid_stride_trip(C):
    """The grid is capped at 2048 workgroups of 256 lanes = 524 288 lanes, one item each per trip.  On the four-pixel path an item is four
    pixels: 3 images of 836 x 840 are 3 * 836 * 210 = 526 680 items, so lanes 0 ... 2391 take a second trip (image 2's last rows).  Run
    twice: the same bits."""
    H, W = 836, 840
    assert W % 4 == 0 and 3 * H * (W // 4) > 2048 * 256 > 2 * H * (W // 4)
    x, y = _inputs(3, 3, H, W, seed=11)
    xd, yd = x.to(DEV), y.to(DEV)
    rows = [(43691, H * 9000 + 3, W * 7000 + 32768, 1), (87381, -H * 10000, -W * 12000 + 1, 0), (ONE, 40000, -40000, 1)]
    gx, gy, bad = _launch(C, x, y, rows, inputs=(xd, yd))
    assert bad == 0
    _check(f'{H}x{W}', gx, gy, x, y, rows)
    gx2, gy2, _ = _launch(C, x, y, rows, inputs=(xd, yd))
    assert torch.equal(gx.view(torch.int32), gx2.view(torch.int32)) and torch.equal(gy, gy2)


# ------------------------------------------------------------------------------------------------------------------------------ bit level
@pytest.mark.parametrize('H,W', [(16, 16), (5, 7), (32, 48)])
def test_identity_and_flip_return_the_bits(C, H, W):
    x, y = _inputs(3, 3, H, W, seed=5)
    gx, gy, _ = _launch(C, x, y, [IDENT] * 3)
    assert torch.equal(gx.view(torch.int32), x.view(torch.int32)) and torch.equal(gy, y)
    gx, gy, _ = _launch(C, x, y, [FLIP] * 3)
    assert torch.equal(gx.view(torch.int32), torch.flip(x, [-1]).view(torch.int32)) and torch.equal(gy, torch.flip(y, [-1]))


@pytest.mark.parametrize('which', ['images', 'labels'])
def test_one_pixel_path_gives_the_four_pixel_paths_bits(C, which):
    """The same batch with the image (or label) tensors one element into a larger buffer: W % 4 == 0, but the output base is only 4-byte
    (8-byte) aligned, which selects the one-pixel instantiation.  Same bits, guard bands intact."""
    H = W = 16
    x, y = _inputs(3, 3, H, W, seed=9)
    rows = _rows(H, W)['fractions and mid scales']
    want_x, want_y, _ = _launch(C, x, y, rows)
    xd, yd = x.to(DEV), y.to(DEV)
    bx, ox, by, oy = _out_buffers(x, y)
    if which == 'images':
        src = torch.empty(x.numel() + 1, device=DEV)
        xd = src[1:].view(x.shape).copy_(xd)
        bx, ox, _, _ = _out_buffers(x, y, GUARD + 1)
        assert xd.data_ptr() % 16 == 4 and ox.data_ptr() % 16 == 4 and oy.data_ptr() % 32 == 0
        n, g = x.numel(), GUARD + 1
    else:
        src = torch.empty(y.numel() + 1, dtype=torch.int64, device=DEV)
        yd = src[1:].view(y.shape).copy_(yd)
        _, _, by, oy = _out_buffers(x, y, GUARD + 1)
        assert yd.data_ptr() % 32 == 8 and oy.data_ptr() % 32 == 8 and ox.data_ptr() % 16 == 0
        n, g = y.numel(), GUARD + 1
    C.augment_batch(xd, yd, torch.tensor(rows).to(DEV), FILL, IGN, out=(ox, oy))
    torch.cuda.synchronize()
    assert torch.equal(ox.cpu().view(torch.int32), want_x.view(torch.int32)) and torch.equal(oy.cpu(), want_y)
    buf, poison = (bx.view(torch.int32), POISON_I) if which == 'images' else (by, POISON_L)
    assert bool((buf[:g] == poison).all()) and bool((buf[g + n:] == poison).all())


# ------------------------------------------------------------------------------------------------------------------- guard and refusals
def test_step_guard(C):
    x, y = _inputs(3, 3, 16, 16, seed=2)
    gx, gy, bad = _launch(C, x, y, [(0, 0, 0, 0), IDENT, ((1 << 19) + 1, 0, 0, 1)])
    assert bad == 2
    for b in (0, 2):
        assert bool((gx[b] == FILL).all()) and bool((gy[b] == IGN).all())
    assert torch.equal(gx[1].view(torch.int32), x[1].view(torch.int32)) and torch.equal(gy[1], y[1])
    _check('guard', gx, gy, x, y, [(0, 0, 0, 0), IDENT, ((1 << 19) + 1, 0, 0, 1)])


def test_host_refusals(C):
    x, y = torch.zeros(2, 3, 8, 8, device=DEV), torch.zeros(2, 8, 8, dtype=torch.int64, device=DEV)
    ox, oy = torch.empty_like(x), torch.empty_like(y)
    p, bad = torch.tensor([IDENT] * 2).to(DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    ptr, s = C._lib.ptr, C._lib.stream_ptr()

    def refused(message, *args):
        with pytest.raises(RuntimeError) as e:
            C._lib.call('clamd_augment_batch', *args)
        assert str(e.value).endswith('): ' + message), str(e.value)

    good = [ptr(x), ptr(y), ptr(p), 2, 3, 8, 8, ptr(ox), ptr(oy), 0.0, -100, ptr(bad), s]

    def but(**kw):
        names = ['images', 'labels', 'params', 'B', 'C', 'H', 'W', 'out_images', 'out_labels', 'fill', 'ignore_index', 'bad', 'stream']
        return [kw.get(n, v) for n, v in zip(names, good)]

    C._lib.call('clamd_augment_batch', *good)
    for kw in (dict(B=0), dict(C=0), dict(H=0), dict(W=-1)):
        refused('augment_batch: empty problem', *but(**kw))
    for kw in (dict(H=4097), dict(W=4097)):
        refused('augment_batch: H and W must be at most 4096', *but(**kw))
    for kw in (dict(out_images=None), dict(images=None), dict(out_labels=None), dict(labels=None)):
        refused('augment_batch: images and out_images go together, and so do labels and out_labels', *but(**kw))
    refused('augment_batch: neither images nor labels', *but(images=None, out_images=None, labels=None, out_labels=None))
    for kw in (dict(params=None), dict(bad=None)):
        refused('augment_batch: null params or bad', *but(**kw))
    for kw in (dict(images=ptr(x) + 2), dict(out_images=ptr(ox) + 1), dict(labels=ptr(y) + 4), dict(out_labels=ptr(oy) + 4), dict(params=ptr(p) + 4),
               dict(bad=ptr(bad) + 2)):
        refused('augment_batch: misaligned tensor', *but(**kw))
    torch.cuda.synchronize()
    assert int(bad) == 0
    with pytest.raises(TypeError, match='params must be an int64'):
        C.augment_batch(x, y, p[:1])
    with pytest.raises(TypeError, match='float32'):
        C.augment_batch(x.double(), y, p)
    with pytest.raises(ValueError, match='out_images must be a contiguous'):
        C.augment_batch(x, y, p, out=(ox[:1], oy))


# ----------------------------------------------------------------------------------------------------------------------------- sampler
def test_sampler_is_seeded(C):
    x, y = _inputs(3, 3, 16, 16, seed=4)
    xd, yd = x.to(DEV), y.to(DEV)
    a, b, c = C.RandomScaleCrop(seed=3), C.RandomScaleCrop(seed=3), C.RandomScaleCrop(seed=4)
    pa = [a.draw(3, 16, 16, DEV) for _ in range(4)]
    pb = [b.draw(3, 16, 16, DEV) for _ in range(4)]
    pc = [c.draw(3, 16, 16, DEV) for _ in range(4)]
    assert all(p.is_cuda and p.dtype == torch.int64 and tuple(p.shape) == (3, 4) for p in pa)
    assert all(torch.equal(p, q) for p, q in zip(pa, pb)) and not all(torch.equal(p, q) for p, q in zip(pa, pc))
    allp = torch.cat(pa)
    assert int(allp[:, 0].min()) >= 32768 and int(allp[:, 0].max()) <= 131072 and set(allp[:, 3].tolist()) <= {0, 1}
    assert any(int(p[:, 3].max()) for p in pa + pc)
    (ax, ay), (bx, by) = a(xd, yd), b(xd, yd)                # the fifth draw of either
    assert torch.equal(ax.view(torch.int32), bx.view(torch.int32)) and torch.equal(ay, by) and int(ay.bad_params) == 0
    nf = C.RandomScaleCrop(seed=3, flip=False)
    assert all(int(nf.draw(3, 16, 16, DEV)[:, 3].abs().max()) == 0 for _ in range(4))
    # the drawn params through the restatement, too
    p = c.draw(3, 16, 16, DEV)
    gx, gy = C.augment_batch(xd, yd, p, FILL, IGN)
    _check('16x16 drawn', gx.cpu(), gy.cpu(), x, y, p.tolist())
    # state_dict -> load_state_dict: the next draw is the one the original makes
    st = a.state_dict()
    assert st['rng'].device.type == 'cpu'
    d = C.RandomScaleCrop(seed=77).load_state_dict(st)
    assert d.seed == 3 and torch.equal(d.draw(3, 16, 16, DEV), a.draw(3, 16, 16, DEV))


# --------------------------------------------------------------------------------------------------------------------------- task step
def _batches(C, n, k=6):
    return [(torch.from_numpy(C.synth.images(60 + i, 4, 3, 32, 32)).to(DEV), torch.from_numpy(C.synth.labels(60 + i, 4, 32, 32, k)).to(DEV))
            for i in range(n)]


def _cfg(C, **kw):
    return C.default_config(n_iters=100, lr=1e-3, num_classes=6, conv_dim=8, stats_every=1, **kw)


def _steps(C, augment, replay, log=None):
    """UNet(6, 3, 8) at 32 x 32, bs 4, fp32, two steps: a Trainer with cfg.augment (augment=True), or one without, fed augment_batch of the
    same batches with the params of a second RandomScaleCrop of the same seed.  replay: after begin_task2(6, distill_lambda=0, replay=8,
    replay_batch=2) -- the trainer's own memory, or a twin memory mixing in front of the twin sampler.
    -> the trainer, per step (loss, the labels the loss saw for rows [0, B), rows of the outputs), the final weights."""
    torch.manual_seed(7)
    task1, task2 = _batches(C, 2), _batches(C, 2)[::-1]
    tr = C.Trainer(task1, _cfg(C, augment=augment, augment_seed=5))
    assert (tr.augment is not None) == augment
    sampler = memory = None
    if replay and augment:
        tr.begin_task2(6, distill_lambda=0, replay=8, replay_batch=2, replay_loader=task1)
    elif replay:
        tr.begin_task2(6, distill_lambda=0)
        memory = C.ReplayMemory(6, (3, 32, 32), seed=0).add_task((1, 6), 8).fill(task1, DEV)
    if not augment:
        sampler = C.RandomScaleCrop(seed=5)
    steps = []
    for x, y in task2:
        if memory is not None:
            x, y = memory.mix(x, y, 2)
        if sampler is not None:
            x, y = C.augment_batch(x, y, sampler.draw(x.shape[0], 32, 32, DEV))
        if log is not None:
            log.clear()
        outputs, loss = tr.train_step(x, y)
        if sampler is not None:
            assert tr.step_labels is y                      # without augmentation: the caller's tensor
        steps.append((loss.detach().clone(), tr.step_labels.clone(), y[:4].clone(), outputs.shape[0]))
    return tr, steps, [p.detach().clone() for p in tr.model.parameters()]


@pytest.mark.parametrize('replay', [False, True])
def test_task_step_with_augmentation(C, monkeypatch, replay):
    calls = []
    real = C.unet._hbm

    def logged(family, nbytes, name, *args):
        calls.append((name, nbytes))
        real(family, nbytes, name, *args)

    monkeypatch.setattr(C.unet, '_hbm', logged)
    rows = 6 if replay else 4
    tr, first, w1 = _steps(C, True, replay, log=calls)
    assert [c for c in calls if c[0] == 'clamd_augment_batch'] == [('clamd_augment_batch', rows * 32 * 32 * (8 * 3 + 16))], calls      # one launch
    _, second, w2 = _steps(C, False, replay, log=calls)
    assert not any(c[0] == 'clamd_augment_batch' for c in calls)
    for (l1, s1, _, n1), (l2, s2, y2, n2) in zip(first, second):
        assert n1 == n2 == rows
        assert torch.equal(l1, l2), (float(l1), float(l2))
        assert torch.equal(s1, y2) and tuple(s1.shape) == (4, 32, 32), 'step_labels are not the augmented labels of rows [0, B)'
    assert all(torch.equal(a, b) for a, b in zip(w1, w2)), 'the step with cfg.augment differs from the step on the augmented batch'
    assert not torch.equal(first[0][1], _batches(C, 2)[1][1])            # and the batch did change
    # the epoch loop: the confusion matrix reads step_labels
    tr.train_data_loader = _batches(C, 2)
    stats = tr.train_epoch(0)
    assert set(stats) >= {'loss', 'pixel_acc', 'mean_iu'} and np.isfinite(stats['loss']) and 0.0 <= stats['pixel_acc'] <= 100.0


def test_checkpoint_carries_the_sampler(C, tmp_path):
    torch.manual_seed(7)
    data = _batches(C, 2)
    tr = C.Trainer(data, _cfg(C, augment=True, augment_seed=5, augment_scale=(0.75, 1.5)))
    tr.train_step(*data[0])                                  # the generator has moved on before the checkpoint
    tr.save_network('unet', 'a', 0, str(tmp_path))
    fresh = C.Trainer(data, _cfg(C, augment=True, augment_seed=99))
    assert fresh.load_network('unet', 'a', str(tmp_path))
    assert fresh.augment.seed == 5 and fresh.augment.scale == (0.75, 1.5) and fresh.augment.ignore_index == tr.augment.ignore_index
    for _ in range(2):
        assert torch.equal(fresh.augment.draw(4, 32, 32, DEV), tr.augment.draw(4, 32, 32, DEV))
    plain = C.Trainer(data, _cfg(C))
    assert plain.augment is None and 'augment_state' not in plain.snapshot(0)
