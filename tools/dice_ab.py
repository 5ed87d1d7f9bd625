"""Cross-entropy + soft Dice measurements, alternated in one process (as tools/augment_ab.py).

(a) clamd_ce_dice_fwd_bwd (sums, coefficient and gradient pass + finalize) against clamd_ce_count + clamd_ce_fwd_bwd_counted at K = 21,
    16 x 256 x 256, without and with the bf16 / fp32 NHWC copy: device events around 50 calls after warm-up, 5 rounds, interleaved; median
    (min, max), algorithmic bytes / median time beside the float4 copy rate bench.py quotes for this part.  Algorithmic bytes: the logits
    twice and the labels twice for Dice (once each for CE), d logits once, the NHWC copy once.  The logits are 88 MB: whether the second read
    is served from the 256 MiB Infinity Cache is what the achieved rate beside the copy rate shows.
(b) The whole fp32 step of UNet(21, 3, 64) at 16 images with loss='ce_dice' against the plain step, alternated.

    python tools/dice_ab.py > profiles/dice.txt        (--steps-only / --kernels-only: one part)
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import continual_learning_amd as C  # noqa: E402

K, B, H, W, N, ROUNDS = 21, 16, 256, 256, 50, 5
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


def spread(rounds, name):
    return sorted(r[name] for r in rounds)


def overlap(a, b):
    return a[0] <= b[-1] and b[0] <= a[-1]


def kernels():
    lib, ptr, call = C._lib.load(), C._lib.ptr, C._lib.call
    z = torch.randn(B, K, H, W, device='cuda') * 3
    y = torch.from_numpy(C.synth.labels(9, B, H, W, K)).cuda()
    d = torch.empty_like(z)
    l3 = torch.empty(3, device='cuda')
    px = B * H * W
    s = C._lib.stream_ptr()
    print(f'(a) K {K}, {B} x {H} x {W}: {N} calls per round, {ROUNDS} rounds, interleaved')
    for name, dcode, esize in ((None, 0, 0), ('bf16', 1, 2), ('fp32', 0, 4)):
        nh = None if name is None else torch.empty(B, H, W, 32, dtype=C.ops.TORCH_DT[dcode], device='cuda')
        ldc = 0 if nh is None else 32
        cases = {}
        for per_image in (0, 1):
            wsb = lib.clamd_ce_dice_workspace_bytes(B, K, H, W, per_image)
            ws = torch.empty(wsb // 4, device='cuda')
            cases[f'ce_dice per_image {per_image}'] = (px * (3 * K * 4 + 16 + 32 * esize), lambda ws=ws, wsb=wsb, per_image=per_image: call(
                'clamd_ce_dice_fwd_bwd', ptr(z), ptr(y), ptr(d), ptr(nh), ldc, dcode, ptr(l3), ptr(ws), wsb, B, K, H, W, -100, 1.0, 1.0, 1e-5, 0, 1,
                per_image, 1.0, s))
        wsc = lib.clamd_ce_workspace_bytes()
        wc = torch.empty(wsc // 4, device='cuda')

        def ce():
            call('clamd_ce_count', ptr(y), B, K, H, W, -100, ptr(wc), wsc, s)
            call('clamd_ce_fwd_bwd_counted', ptr(z), ptr(y), ptr(d), ptr(nh), ldc, dcode, ptr(l3), ptr(wc), wsc, B, K, H, W, -100, 1.0, s)
        cases['ce count + counted'] = (px * (2 * K * 4 + 16 + 32 * esize), ce)
        rounds = [{k: timed(fn) for k, (_, fn) in cases.items()} for _ in range(ROUNDS)]
        print(f'  NHWC copy: {name}')
        for k, (nbytes, _) in cases.items():
            t = spread(rounds, k)
            print(f'    {k:24s} {t[ROUNDS // 2]:8.1f} us (min {t[0]:.1f}, max {t[-1]:.1f})   {nbytes / 1e6:6.1f} MB algorithmic   '
                  f'{nbytes / t[ROUNDS // 2] / 1e6:.2f} TB/s (copy rate {COPY_RATE})')
        a, b = spread(rounds, 'ce_dice per_image 0'), spread(rounds, 'ce count + counted')
        print(f'    ce_dice - ce, medians: {a[ROUNDS // 2] - b[ROUNDS // 2]:+.1f} us' + ('; the spreads overlap: no difference claimed' if overlap(a, b) else ''))


def steps():
    x = torch.from_numpy(C.synth.images(9, B, 3, H, W)).cuda()
    y = torch.from_numpy(C.synth.labels(9, B, H, W, K)).cuda()
    tr = C.Trainer([(x, y)], C.default_config(n_iters=10000, num_classes=K, conv_dim=64, compute_dtype='fp32', loss='ce_dice'))
    sides = {'A step with loss=ce_dice': tr.c_loss, 'B plain step': tr.likelihood_loss}
    for crit in sides.values():
        tr.c_loss = crit
        tr.train_step(x, y)

    def run(name, n=10):
        tr.c_loss = sides[name]
        return timed(lambda: tr.train_step(x, y), n) / 1e3

    rounds = [{name: run(name) for name in sides} for _ in range(ROUNDS)]
    print(f'(b) whole fp32 step, UNet({K}, 3, 64) at {B} x {H} x {W}, 10 steps per round, alternated')
    for name in sides:
        t = spread(rounds, name)
        print(f'    {name:26s} {t[ROUNDS // 2]:.3f} ms (min {t[0]:.3f}, max {t[-1]:.3f})')
    a, b = (spread(rounds, n) for n in sides)
    print(f'    difference of the medians {1e3 * (a[ROUNDS // 2] - b[ROUNDS // 2]):+.0f} us' + ('; the spreads overlap: no difference claimed' if overlap(a, b) else ''))


if __name__ == '__main__':
    if '--steps-only' not in sys.argv:
        kernels()
    if '--kernels-only' not in sys.argv:
        steps()
