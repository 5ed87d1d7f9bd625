"""Training-augmentation measurements, alternated in one process (as tools/replay_ab.py).

(a) clamd_augment_batch at K = 21, C = 3, 256 x 256 for 16 images and for 12 + 4 (the mixed batch of a replay step: the same 16 rows, drawn
    separately), params from RandomScaleCrop(0.5 - 2, flip): device events around 50 launches after warm-up, 5 rounds, interleaved; median
    (min, max), algorithmic bytes B * H * W * (8 C + 16) / median time beside the float4 copy rate bench.py quotes for this part.
(b) The stock-torch restatement on the same params: F.grid_sample(bilinear, align_corners=False, padding_mode='border') plus the mask, a
    nearest grid_sample of the labels through float, and flip.  Its results are compared with the kernel's and the differences printed --
    the restatement samples in fp32, so neither the images nor the labels along object boundaries need agree.
(c) The whole fp32 step of UNet(21, 3, 64) at 16 images with and without cfg.augment, alternated.

    python tools/augment_ab.py > profiles/augment.txt        (--steps-only / --kernels-only: one part)
"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import continual_learning_amd as C  # noqa: E402

K, CH, H, W, N, ROUNDS = 21, 3, 256, 256, 50, 5
COPY_RATE = 6.29      # TB/s, a float4 copy on this part (bench.py)


def timed(fn, n=N):
    for _ in range(5):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def report(cases):
    """cases: {name: (algorithmic bytes or None, fn)} -> {name: sorted times}, printed as median (min, max)."""
    rounds = [{k: timed(fn) for k, (_, fn) in cases.items()} for _ in range(ROUNDS)]
    out = {}
    for k, (nbytes, _) in cases.items():
        t = sorted(r[k] for r in rounds)
        out[k] = t
        rate = f'   {nbytes / 1e6:6.1f} MB algorithmic   {nbytes / t[ROUNDS // 2] / 1e6:.2f} TB/s (copy rate {COPY_RATE})' if nbytes else ''
        print(f'{k:46s} {t[ROUNDS // 2]:8.1f} us (min {t[0]:.1f}, max {t[-1]:.1f}){rate}')
    return out


def torch_augment(x, y, params, fill=0.0, ignore_index=-100):
    """The stock-torch restatement: a sampling grid in fp32, two grid_sample passes, the mask, the flip."""
    B, _, h, w = x.shape
    step, y0, x0, flip = (params[:, i] for i in range(4))
    ii = torch.arange(h, device=x.device)
    jj = torch.arange(w, device=x.device)
    sy = y0[:, None] + ii[None, :] * step[:, None]                     # [B, H] Q16
    sx = x0[:, None] + jj[None, :] * step[:, None]                     # [B, W] (un-flipped: the flip is a pass of its own below)
    inside = ((sy + 32768 >= 0) & (sy + 32768 < h * 65536))[:, :, None] & ((sx + 32768 >= 0) & (sx + 32768 < w * 65536))[:, None, :]
    gy = (2 * (sy.float() / 65536) + 1) / h - 1
    gx = (2 * (sx.float() / 65536) + 1) / w - 1
    grid = torch.stack([gx[:, None, :].expand(B, h, w), gy[:, :, None].expand(B, h, w)], dim=-1)
    ox = F.grid_sample(x, grid, mode='bilinear', padding_mode='border', align_corners=False)
    ox = torch.where(inside[:, None], ox, torch.full((), fill, device=x.device))
    oy = F.grid_sample(y[:, None].float(), grid, mode='nearest', padding_mode='border', align_corners=False)[:, 0].long()
    oy = torch.where(inside, oy, torch.full((), ignore_index, device=x.device, dtype=torch.int64))
    f = flip.bool()
    return torch.where(f[:, None, None, None], ox.flip(-1), ox), torch.where(f[:, None, None], oy.flip(-1), oy)


def kernels():
    x = torch.from_numpy(C.synth.images(9, 16, CH, H, W)).cuda()
    y = torch.from_numpy(C.synth.labels(9, 16, H, W, K)).cuda()
    aug = C.RandomScaleCrop(seed=1)
    p16 = aug.draw(16, H, W)
    p124 = torch.cat([aug.draw(12, H, W), aug.draw(4, H, W)])
    nbytes = 16 * H * W * (8 * CH + 16)
    ox, oy = torch.empty_like(x), torch.empty_like(y)
    ident = torch.tensor([[65536, 0, 0, 0]] * 16, device='cuda')      # scale 1 and no padding: every output pixel reads its four taps
    print(f'(a) kernel, K {K}, {CH} x {H} x {W}, params of RandomScaleCrop(0.5 - 2, flip), seed 1; scales '
          + ' '.join(f'{65536 / s:.2f}' for s in p16[:, 0].tolist()))
    cases = {'augment_batch 16 (preallocated outputs)': (nbytes, lambda: C.augment_batch(x, y, p16, out=(ox, oy))),
             'augment_batch 12 + 4 (preallocated outputs)': (nbytes, lambda: C.augment_batch(x, y, p124, out=(ox, oy))),
             'augment_batch 16 (two output allocations)': (nbytes, lambda: C.augment_batch(x, y, p16)),
             'augment_batch 16 identity params': (nbytes, lambda: C.augment_batch(x, y, ident, out=(ox, oy))),
             'RandomScaleCrop.draw 16 (the draws alone)': (None, lambda: aug.draw(16, H, W)),
             'RandomScaleCrop.__call__ 16 (with the draws)': (None, lambda: aug(x, y))}
    report(cases)
    print('(b) against the stock-torch restatement (grid_sample bilinear + mask, grid_sample nearest on float labels, flip), the same params')
    a, b = C.augment_batch(x, y, p16), torch_augment(x, y, p16)
    print(f'    images: max |kernel - torch| {float((a[0] - b[0]).abs().max()):.2e}; labels that differ: {int((a[1] != b[1]).sum())} of {a[1].numel()}')
    t = report({'kernel 16': (None, lambda: C.augment_batch(x, y, p16)), 'torch  16': (None, lambda: torch_augment(x, y, p16))})
    k, r = t['kernel 16'], t['torch  16']
    print('    ' + ('the spreads overlap: no win claimed' if k[-1] >= r[0] else f'kernel faster, median ratio {r[ROUNDS // 2] / k[ROUNDS // 2]:.2f}x'))


def steps():
    x = torch.from_numpy(C.synth.images(9, 16, CH, H, W)).cuda()
    y = torch.from_numpy(C.synth.labels(9, 16, H, W, K)).cuda()
    tr = C.Trainer([(x, y)], C.default_config(n_iters=10000, num_classes=K, conv_dim=64, compute_dtype='fp32', augment=True))
    tr.train_step(x, y)
    sides = {'A step with cfg.augment': tr.augment, 'B plain step': None}

    def run(name, n=10):
        tr.augment = sides[name]
        return timed(lambda: tr.train_step(x, y), n) / 1e3

    rounds = [{name: run(name) for name in sides} for _ in range(ROUNDS)]
    print('(c) whole fp32 step, UNet(21, 3, 64) at 16 x 256 x 256, 10 steps per round, alternated')
    for name in sides:
        t = sorted(r[name] for r in rounds)
        print(f'    {name:24s} {t[ROUNDS // 2]:.3f} ms (min {t[0]:.3f}, max {t[-1]:.3f})')
    a, b = (sorted(r[n] for r in rounds) for n in sides)
    print(f'    difference of the medians {1e3 * (a[ROUNDS // 2] - b[ROUNDS // 2]):+.0f} us' + ('; the spreads overlap' if a[0] <= b[-1] and b[0] <= a[-1] else ''))


if __name__ == '__main__':
    if '--steps-only' not in sys.argv:
        kernels()
    if '--kernels-only' not in sys.argv:
        steps()
