"""CPU: the augmentation's yardstick (tests/augment_ref.py) against torch's own resize at the two windows where they coincide, the
params arithmetic against plain Python integers, the two geometric guarantees of params_from_draws proved from the params alone, and the
sampler's constructor and state.  No kernel is launched here."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from augment_ref import augment_ref

import continual_learning_amd as C
from continual_learning_amd import augment

SIZES = [(5, 7), (16, 16), (6, 9)]


def _sample(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 3, H, W, generator=g, dtype=torch.float64) * 3
    y = torch.randint(0, 21, (2, H, W), generator=g)
    return x, y


# --------------------------------------------------------------------------------------------------------------- the yardstick vs torch
@pytest.mark.parametrize('H,W', SIZES)
@pytest.mark.parametrize('corner', ['top-left', 'bottom-right'])
def test_restatement_matches_torch_resize(H, W, corner):
    """step = 32768 is scale 2; output pixel i then samples source i / 2 - 1 / 4, which is y0 = -16384 in Q16: the top-left H x W window of
    F.interpolate(scale_factor=2).  y0 = H * 32768 - 16384 starts at row H of the enlarged image: its bottom-right window, where torch clamps
    the second tap at the far edge."""
    x, y = _sample(H, W, seed=H * 100 + W)
    if corner == 'top-left':
        y0, x0, win = -16384, -16384, (slice(0, H), slice(0, W))
    else:
        y0, x0, win = H * 32768 - 16384, W * 32768 - 16384, (slice(H, 2 * H), slice(W, 2 * W))
    params = [(32768, y0, x0, 0)] * 2
    gx, gy, inside, M = augment_ref(x.numpy(), y.numpy(), params)
    assert inside.all()
    want_x = F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False)[(..., *win)]
    want_y = F.interpolate(y.double()[:, None], scale_factor=2, mode='nearest-exact')[:, 0][(..., *win)].long()
    np.testing.assert_allclose(gx, want_x.numpy(), rtol=1e-12, atol=0)
    assert np.array_equal(gy, want_y.numpy())
    assert (M >= np.abs(gx) * (1 - 1e-12)).all()         # a convex combination never exceeds its largest tap


def test_restatement_identity_flip_and_guard():
    x, y = _sample(5, 7, seed=1)
    gx, gy, inside, _ = augment_ref(x.numpy(), y.numpy(), [(65536, 0, 0, 0), (65536, 0, 0, 1)])
    assert inside.all()
    assert np.array_equal(gx[0], x[0].numpy()) and np.array_equal(gy[0], y[0].numpy())
    assert np.array_equal(gx[1], x[1].numpy()[..., ::-1]) and np.array_equal(gy[1], y[1].numpy()[..., ::-1])
    gx, gy, inside, _ = augment_ref(x.numpy(), y.numpy(), [(0, 0, 0, 0), ((1 << 19) + 1, 0, 0, 0)], fill=0.5, ignore_index=255)
    assert not inside.any() and (gx == 0.5).all() and (gy == 255).all()
    # shifted by one whole pixel: the last column / row falls outside, at the same pixels for the image and the labels
    gx, gy, inside, _ = augment_ref(x.numpy(), y.numpy(), [(65536, 65536, 65536, 0)] * 2, fill=-7.0)
    assert inside[:, :-1, :-1].all() and not inside[:, -1].any() and not inside[:, :, -1].any()
    assert np.array_equal(gx[:, :, :-1, :-1], x.numpy()[:, :, 1:, 1:]) and (gx[:, :, -1] == -7.0).all() and (gy[:, :, -1] == -100).all()


# ------------------------------------------------------------------------------------------------------------------- params_from_draws
def _params_py(q, ry, rx, flip, H, W):
    """The issue's formulas in Python integers."""
    step = ((1 << 24) + q // 2) // q
    out = [step]
    for r, N in ((ry, H), (rx, W)):
        slack = N * (65536 - step)
        lo, hi = min(0, slack), max(0, slack)
        out.append(lo + ((r * (hi - lo + 1)) >> 31) + (step >> 1) - 32768)
    return out + [flip]


@pytest.mark.parametrize('H,W', [(5, 5), (16, 5), (4096, 16), (4096, 4096)])
def test_params_from_draws_at_the_corners(H, W):
    rmax = (1 << 31) - 1
    cases = [(q, ry, rx, f) for q in (32, 128, 256, 512, 2048) for ry in (0, rmax) for rx in (0, rmax) for f in (0, 1)]
    got = C.params_from_draws(*(torch.tensor(col) for col in zip(*cases)), H, W)
    assert got.dtype == torch.int64 and tuple(got.shape) == (len(cases), 4)
    assert got.tolist() == [_params_py(*c, H, W) for c in cases]
    steps = {c[0]: p[0] for c, p in zip(cases, got.tolist())}
    assert steps[32] == 1 << 19 and steps[2048] == 1 << 13 and steps[256] == 1 << 16          # the kernel's range, end to end


def test_scale_one_is_the_identity():
    rmax = (1 << 31) - 1
    got = C.params_from_draws(torch.tensor([256, 256]), torch.tensor([0, rmax]), torch.tensor([rmax, 12345]), torch.tensor([0, 1]), 16, 4096)
    assert got.tolist() == [[65536, 0, 0, 0], [65536, 0, 0, 1]]


@pytest.mark.parametrize('H,W', [(5, 7), (16, 16), (4096, 4096)])
def test_draws_keep_the_window_and_the_source_where_they_belong(H, W):
    """10 000 seeded draws over q in [32, 2048].  Output pixel i samples the Q16 position t_i = y0 + 32768 + i * step (pixel s covers
    [s * 65536, (s + 1) * 65536)) and stands for the window cell [t_i - step / 2, t_i + step / 2).
    q >= 256: the first and the last sample lie inside the source, hence all do (t_i is monotone): no output pixel is outside.
    q < 256: the window [t_0 - (step >> 1), t_0 - (step >> 1) + N * step) contains the first and the last source pixel centre."""
    g = torch.Generator().manual_seed(H)
    n = 10000
    q = torch.randint(32, 2049, (n,), generator=g)
    q[:4] = torch.tensor([32, 255, 256, 2048])
    ry, rx = torch.randint(1 << 31, (n,), generator=g), torch.randint(1 << 31, (n,), generator=g)
    ry[:4], rx[:4] = torch.tensor([0, (1 << 31) - 1, 0, (1 << 31) - 1]), torch.tensor([(1 << 31) - 1, 0, 0, (1 << 31) - 1])
    p = C.params_from_draws(q, ry, rx, torch.zeros(n, dtype=torch.int64), H, W)
    step = p[:, 0]
    assert torch.equal(step, ((1 << 24) + q // 2) // q) and int(step.min()) == 1 << 13 and int(step.max()) == 1 << 19
    big, small = q >= 256, q < 256
    assert int(big.sum()) > 1000 and int(small.sum()) > 500
    for origin, N in ((p[:, 1], H), (p[:, 2], W)):
        first, last = origin + 32768, origin + 32768 + (N - 1) * step
        assert bool((first[big] >= 0).all()) and bool((last[big] < N * 65536).all())
        edge = first - (step >> 1)
        assert bool((edge[small] <= 32768).all()) and bool((edge[small] + N * step[small] > (N - 1) * 65536 + 32768).all())
    # the restatement agrees on the pinned corners: nothing outside at scale >= 1, padding on the drawn side at scale 1/8
    for i in range(4) if H <= 16 else ():
        _, _, inside, _ = augment_ref(None, np.zeros((1, H, W), np.int64), [p[i].tolist()])
        assert inside.all() == (int(q[i]) >= 255), int(q[i])          # q = 255 widens the window by 0.4 %: still no pixel outside
    if H <= 16:
        _, _, inside, _ = augment_ref(None, np.zeros((1, H, W), np.int64), [p[0].tolist()])
        # ry = 0 puts the window's first edge as far before the source as it goes (the source at the bottom), rx = 2^31 - 1 at the source's own
        assert inside[0, -1].any() and inside[0, :, 0].any() and not inside[0, 0].any() and not inside[0, :, -1].any()


# ----------------------------------------------------------------------------------------------------------------------------- sampler
def test_random_scale_crop_refuses_bad_scales():
    for scale in [(0.1, 2.0), (0.5, 8.5), (2.0, 0.5), 1.0, (1.0,)]:
        with pytest.raises(ValueError, match='scale'):
            C.RandomScaleCrop(scale=scale)
    a = C.RandomScaleCrop(scale=(1, 1))
    assert (a.qmin, a.qmax) == (256, 256)
    a = C.RandomScaleCrop(scale=(1 / 8, 8))
    assert (a.qmin, a.qmax) == (32, 2048)
    assert C.RandomScaleCrop().scale == (0.5, 2.0)


def test_draw_on_the_host_generator_is_seeded_and_in_range():
    """draw is plain torch: on a CPU generator it gives the same arithmetic (the kernel itself has no CPU path)."""
    a, b, c = C.RandomScaleCrop(seed=5), C.RandomScaleCrop(seed=5), C.RandomScaleCrop(seed=6)
    pa, pb, pc = (s.draw(64, 16, 24, device='cpu') for s in (a, b, c))
    assert pa.dtype == torch.int64 and tuple(pa.shape) == (64, 4)
    assert torch.equal(pa, pb) and not torch.equal(pa, pc)
    assert int(pa[:, 0].min()) >= 32768 and int(pa[:, 0].max()) <= 131072 and set(pa[:, 3].tolist()) == {0, 1}
    nf = C.RandomScaleCrop(seed=5, flip=False).draw(64, 16, 24, device='cpu')
    assert int(nf[:, 3].abs().max()) == 0 and torch.equal(nf[:, :3], pa[:, :3])       # the flip is drawn last: the rest is unchanged
    one = C.RandomScaleCrop(scale=(1, 1), flip=False).draw(3, 16, 24, device='cpu')
    assert one.tolist() == [[65536, 0, 0, 0]] * 3
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        a(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        C.augment_batch(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64), one[:1])


def test_state_dict_round_trip_on_the_host():
    """Before the first draw the state holds no generator state; afterwards a host byte tensor, which a fresh sampler keeps until its own
    first draw creates the generator (as ReplayMemory does) -- on the same device type the draws then continue where they stopped."""
    a = C.RandomScaleCrop(scale=(0.75, 1.5), flip=False, fill=0.25, ignore_index=255, seed=9)
    st = a.state_dict()
    assert st == dict(scale=(0.75, 1.5), flip=False, fill=0.25, ignore_index=255, seed=9, rng=None)
    a.draw(4, 8, 8, device='cpu')
    st = a.state_dict()
    assert torch.is_tensor(st['rng']) and st['rng'].device.type == 'cpu'
    b = C.RandomScaleCrop().load_state_dict(st)
    assert (b.qmin, b.qmax, b.flip, b.fill, b.ignore_index, b.seed) == (192, 384, False, 0.25, 255, 9)
    assert b.gen is None and torch.equal(b.state_dict()['rng'], st['rng'])
    assert torch.equal(a.draw(4, 8, 8, device='cpu'), b.draw(4, 8, 8, device='cpu'))
    with pytest.raises(ValueError, match='draws on cpu'):
        b.draw(4, 8, 8, device='meta')
    with pytest.raises(ValueError, match='scale'):
        C.RandomScaleCrop().load_state_dict(dict(st, scale=(0.01, 1.0)))


def test_default_config_carries_the_augmentation_switches():
    cfg = C.default_config()
    assert (cfg.augment, cfg.augment_scale, cfg.augment_flip, cfg.augment_seed) == (False, (0.5, 2.0), True, 0)
    assert 'clamd_augment_batch' in C._lib.SIGNATURES and hasattr(augment, 'params_from_draws')
