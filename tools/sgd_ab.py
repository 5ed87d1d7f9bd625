"""Interleaved A/B of the whole train step with FusedAdam and with FusedSGD (momentum 0.9, Nesterov, weight decay 1e-4) in ONE process,
config 2 of BASELINE.md (UNet(21, 3, 64), 256 x 256, batch 16): best round of each (ms per step); then the optimiser steps alone (device
events around `--opt-steps` back-to-back optimizer steps on fixed gradients, after warm-up), three interleaved rounds, each with its
algorithmic bytes (Adam 28 B, SGD with momentum 20 B, + L2 24 B, + L2 + EWC 28 B per parameter) and GB/s, and the median of the rounds.

    python tools/sgd_ab.py --dtype fp32
    python tools/sgd_ab.py --only sgd --rounds 1 --steps 5 --opt-steps 20         # one side alone (under rocprofv3 --kernel-trace --stats)
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import continual_learning_amd as C

ap = argparse.ArgumentParser()
ap.add_argument('--dtype', default='fp32', choices=['fp32', 'bf16', 'bf16x3'])
ap.add_argument('--size', type=int, default=256)
ap.add_argument('--batch', type=int, default=16)
ap.add_argument('--conv-dim', type=int, default=64)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--steps', type=int, default=10)
ap.add_argument('--opt-steps', type=int, default=200)
ap.add_argument('--only', choices=['adam', 'sgd', 'sgd_l2', 'sgd_l2_ewc'], default=None)
a = ap.parse_args()

dev = torch.device('cuda', 0)
x = torch.from_numpy(C.synth.images(1234, a.batch, 3, a.size, a.size)).to(dev)
y = torch.from_numpy(C.synth.labels(1234, a.batch, a.size, a.size, 21)).to(dev)
crit = C.CrossEntropyLoss()
BYTES = {'adam': 28, 'sgd': 20, 'sgd_l2': 24, 'sgd_l2_ewc': 28}
LABEL = {'adam': 'Adam', 'sgd': 'SGD with momentum', 'sgd_l2': 'SGD + L2', 'sgd_l2_ewc': 'SGD + L2 + EWC'}
runs = []
for mode in ([a.only] if a.only else list(BYTES)):
    torch.manual_seed(1234)
    m = C.UNet(21, 3, a.conv_dim, compute_dtype=a.dtype).to(dev).train()
    if mode == 'adam':
        o = C.FusedAdam(m.parameters(), lr=1e-4, betas=[0.5, 0.99])
    else:
        o = C.FusedSGD(m.parameters(), lr=1e-3, momentum=0.9, nesterov=True, weight_decay=1e-4)
    old = [p.detach().clone() for p in m.parameters()]
    if mode == 'sgd_l2_ewc':
        g = torch.Generator(device=dev).manual_seed(1)
        o.set_consolidation(old, [torch.rand(p.shape, device=dev, generator=g) for p in old], 0.01)
    if mode in ('sgd_l2', 'sgd_l2_ewc'):
        o.set_l2_anchor(old, 0.01)

    def step(m=m, o=o):
        out = m(x); o.zero_grad(); loss = crit(out, y); loss.backward(); o.step()
        return loss
    for _ in range(3):
        step()                    # builds the engine
    runs.append((mode, step, m, o))

# the whole step: Adam against SGD with momentum (the anchor terms change the optimiser kernel only)
whole = [r for r in runs if r[0] in ('adam', 'sgd')]
best = {k: 1e9 for k, *_ in whole}
for rd in range(a.rounds):
    for k, step, _, _ in whole:
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(a.steps):
            loss = step()
        torch.cuda.synchronize()
        best[k] = min(best[k], (time.perf_counter() - t0) / a.steps)
if whole:
    print(a.dtype, f'{a.size}x{a.size} bs{a.batch}', '  '.join(f'{k}: {t * 1e3:.3f} ms/step ({a.batch / t:.1f} img/s)' for k, t in best.items()),
          f'loss {float(loss.detach()):.4f}')


def timed(fn, n):
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


# the optimizer steps alone, on the gradients the last train step left (the kernel + the fixed-order penalty sums; Adam: + its prepare)
times = {k: [] for k, *_ in runs}
for rd in range(3):
    for k, _, m, o in runs:
        numel = sum(p.numel() for p in m.parameters())
        ms = timed(o.step, a.opt_steps)
        times[k].append(ms)
        print(f'round {rd} {LABEL[k]}: {ms:.4f} ms  {BYTES[k]} B x {numel} = {BYTES[k] * numel / 1e6:.1f} MB  {BYTES[k] * numel / ms / 1e6:.0f} GB/s')
for k, _, m, _ in runs:
    numel = sum(p.numel() for p in m.parameters())
    ms = statistics.median(times[k])
    gbs = [BYTES[k] * numel / t / 1e6 for t in times[k]]
    print(f'median {LABEL[k]}: {ms:.4f} ms  {BYTES[k] * numel / ms / 1e6:.0f} GB/s  (rounds {min(gbs):.0f} .. {max(gbs):.0f} GB/s)')
