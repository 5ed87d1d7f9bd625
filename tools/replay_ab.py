"""Exemplar-replay measurements, alternated in one process (as tools/pseudo_ab.py).

(a) The three launches at K = 21, C = 3, 256 x 256 -- clamd_class_pixel_counts and clamd_replay_store at batch 16, clamd_replay_mix at 12 current +
    4 replayed images, uint8 and fp32 storage: device events around 50 launches after warm-up, 5 rounds, interleaved; median (min, max),
    algorithmic bytes / median time beside the float4 copy rate bench.py quotes for this part (6.29 TB/s).
(b) ReplayMemory.mix against its stock-torch restatement (index, convert, normalise, flip, cat), same slots and flips, alternated.
(c) The whole fp32 step of UNet(21, 3, 64): 12 images + replay_batch = 4 against the plain step at 16 images of the same tree (no file on
    the plain step's path differs from the commit before the feature); the difference is the mix launch.

    python tools/replay_ab.py > profiles/replay.txt        (--steps-only / --kernels-only: one part)
"""
import os
import sys

import torch

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


def memory(storage, x, y):
    mem = C.ReplayMemory(K, (CH, H, W), storage=storage, seed=1).add_task((1, K), 40)
    mem.observe(x, y)
    mem.observe(x.flip(0), y.flip(0))
    return mem.finish()


def torch_mix(mem, x, y, slots, flips):
    """The stock-torch restatement of mix: one allocation and one pass per operation."""
    ex = mem.images[slots]
    if mem.storage == 'uint8':      # a tensor divisor: torch divides by a Python scalar as a multiplication by its reciprocal, one ulp off
        ex = (ex.to(torch.float32) / torch.full((), 255.0, device=ex.device) - 0.5) / 0.5
    ey = mem.labels[slots].to(torch.int64)
    ey = torch.where(ey == 255, torch.full_like(ey, mem.ignore_index), ey)
    # one flip code per exemplar: a horizontal and a vertical pass over the rows that take it
    fw, fh = (flips & 1).bool(), (flips & 2).bool()
    ex = torch.where(fw[:, None, None, None], ex.flip(-1), ex)
    ex = torch.where(fh[:, None, None, None], ex.flip(-2), ex)
    ey = torch.where(fw[:, None, None], ey.flip(-1), ey)
    ey = torch.where(fh[:, None, None], ey.flip(-2), ey)
    return torch.cat([x, ex]), torch.cat([y, ey])


def kernels():
    x = torch.from_numpy(C.synth.images(9, 16, CH, H, W)).cuda()
    y = torch.from_numpy(C.synth.labels(9, 16, H, W, K)).cuda()
    mems = {s: memory(s, x, y) for s in C.replay.STORAGES}
    npx = H * W
    lib, ptr, st = C._lib, C._lib.ptr, C._lib.stream_ptr()
    counts, bad = torch.empty(16, K, dtype=torch.int32, device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda')
    idx = torch.arange(16, dtype=torch.int32, device='cuda')          # image r -> slot r
    cases = {'class_pixel_counts B16': (16 * npx * 8, lambda: lib.call('clamd_class_pixel_counts', ptr(y), ptr(counts), ptr(bad), 16, K, H, W, -100, st))}
    for s, mem in mems.items():
        px = 1 if s == 'uint8' else 4
        cases[f'replay_store B16 {s}'] = (16 * npx * (CH * (4 + px) + 9), lambda mem=mem, s=s: lib.call(
            'clamd_replay_store', ptr(x), ptr(y), ptr(idx), ptr(idx), 16, ptr(mem.images), ptr(mem.labels), int(s == 'fp32'), mem.images.shape[0],
            ptr(mem.bad_labels), 16, CH, H, W, K, -100, st))
    x12, y12 = x[:12].contiguous(), y[:12].contiguous()
    fixed = {}
    for s, mem in mems.items():
        px = 1 if s == 'uint8' else 4
        fixed[s] = mem.draw(4)
        nbytes = npx * (12 * (8 * CH + 16) + 4 * (CH * (px + 4) + 9))
        cases[f'replay_mix 12 + 4 {s} (kernel, fixed slots)'] = (nbytes, lambda mem=mem, s=s: mem._launch(x12, y12, 12, *fixed[s]))
    print(f'(a) kernels, K {K}, {CH} x {H} x {W}; counts and store through the C ABI alone, mix with its two output allocations')
    report(cases)
    print('(b) mix against the stock-torch restatement, 12 + 4, the same slots and flips')
    cases = {}
    for s, mem in mems.items():
        a, b = mem._launch(x12, y12, 12, *fixed[s]), torch_mix(mem, x12, y12, *fixed[s])
        diff = float((a[0] - b[0]).abs().max())
        print(f'    {s}: restatement against kernel: images bit-identical {torch.equal(a[0], b[0])} (max difference {diff:.1e}), labels identical {torch.equal(a[1], b[1])}')
        assert diff <= 2.4e-7 and torch.equal(a[1], b[1]), f'{s}: the restatement disagrees with the kernel'      # 2 ulp at 1: torch's own division
        cases[f'kernel {s}'] = (None, lambda mem=mem, s=s: mem._launch(x12, y12, 12, *fixed[s]))
        cases[f'torch  {s}'] = (None, lambda mem=mem, s=s: torch_mix(mem, x12, y12, *fixed[s]))
        cases[f'ReplayMemory.mix {s} (with the draws)'] = (None, lambda mem=mem: mem.mix(x12, y12, 4))
    t = report(cases)
    for s in mems:
        k, r = t[f'kernel {s}'], t[f'torch  {s}']
        verdict = 'the spreads overlap: no win claimed' if k[-1] >= r[0] else f'kernel faster, median ratio {r[ROUNDS // 2] / k[ROUNDS // 2]:.2f}x'
        print(f'    {s}: {verdict}')


def steps():
    x = torch.from_numpy(C.synth.images(9, 16, CH, H, W)).cuda()
    y = torch.from_numpy(C.synth.labels(9, 16, H, W, K)).cuda()
    x12, y12 = x[:12].contiguous(), y[:12].contiguous()
    tr = C.Trainer([(x, y)], C.default_config(n_iters=10000, num_classes=K, conv_dim=64, compute_dtype='fp32'))
    tr.train_step(x, y)
    tr.begin_task2(K, distill_lambda=0, replay=40, replay_batch=4)
    mem = tr.replay
    sides = {'A 12 + replay_batch 4': (mem, x12, y12), 'B plain step at 16': (None, x, y)}

    def run(name, n=10):
        tr.replay, xx, yy = sides[name]
        return timed(lambda: tr.train_step(xx, yy), n) / 1e3

    rounds = [{name: run(name) for name in sides} for _ in range(ROUNDS)]
    print('(c) whole fp32 step, UNet(21, 3, 64) at 256 x 256, 10 steps per round, alternated')
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
