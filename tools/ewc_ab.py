"""Interleaved A/B of the plain train step, the step with the L2-to-old-weights term and the step with elastic weight consolidation in ONE
process, config 2 of BASELINE.md (UNet(21, 3, 64), 256 x 256, batch 16): best round of each (ms per step); then the three Adam kernels
alone (device events around `--adam-steps` back-to-back optimizer steps on fixed gradients, after warm-up) and clamd_importance_accum alone,
each with its algorithmic bytes (28 / 32 / 36 B and 12 B per parameter) and GB/s.

    python tools/ewc_ab.py --dtype fp32
    python tools/ewc_ab.py --only ewc --rounds 1 --steps 5 --adam-steps 20         # one side alone (under rocprofv3 --kernel-trace --stats)
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import continual_learning_amd as C

ap = argparse.ArgumentParser()
ap.add_argument('--dtype', default='fp32', choices=['fp32', 'bf16', 'bf16x3'])
ap.add_argument('--size', type=int, default=256)
ap.add_argument('--batch', type=int, default=16)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--steps', type=int, default=10)
ap.add_argument('--adam-steps', type=int, default=200)
ap.add_argument('--only', choices=['plain', 'l2', 'ewc'], default=None)
a = ap.parse_args()

dev = torch.device('cuda', 0)
x = torch.from_numpy(C.synth.images(1234, a.batch, 3, a.size, a.size)).to(dev)
y = torch.from_numpy(C.synth.labels(1234, a.batch, a.size, a.size, 21)).to(dev)
crit = C.CrossEntropyLoss()
BYTES = {'plain': 28, 'l2': 32, 'ewc': 36}
runs = []
for mode in ([a.only] if a.only else ['plain', 'l2', 'ewc']):
    torch.manual_seed(1234)
    m = C.UNet(21, 3, 64, compute_dtype=a.dtype).to(dev).train()
    o = C.FusedAdam(m.parameters(), lr=1e-4, betas=[0.5, 0.99])
    old = [p.detach().clone() for p in m.parameters()]
    if mode == 'l2':
        o.set_l2_anchor(old, 0.01)
    elif mode == 'ewc':
        g = torch.Generator(device=dev).manual_seed(1)
        o.set_consolidation(old, [torch.rand(p.shape, device=dev, generator=g) for p in old], 0.01)

    def step(m=m, o=o):
        out = m(x); o.zero_grad(); loss = crit(out, y); loss.backward(); o.step()
        return loss
    for _ in range(3):
        step()                    # builds the engine
    runs.append((mode, step, m, o))
best = {k: 1e9 for k, *_ in runs}
for rd in range(a.rounds):
    for k, step, _, _ in runs:
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(a.steps):
            loss = step()
        torch.cuda.synchronize()
        best[k] = min(best[k], (time.perf_counter() - t0) / a.steps)
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


# the optimizer steps alone, on the gradients the last train step left (prepare + Adam kernel + the fixed-order penalty sums)
numel = 0
for rd in range(3):
    for k, _, m, o in runs:
        numel = sum(p.numel() for p in m.parameters())
        ms = timed(o.step, a.adam_steps)
        print(f'adam {k}: {ms:.4f} ms  {BYTES[k]} B x {numel} = {BYTES[k] * numel / 1e6:.1f} MB  {BYTES[k] * numel / ms / 1e6:.0f} GB/s')
# the accumulate kernel alone: importance += grad^2 over all 82 tensors in one launch
_, _, m, _ = runs[-1]
cons = C.Consolidation(m.named_parameters())
params = list(m.parameters())
for rd in range(3):
    ms = timed(lambda: cons.accumulate(params), a.adam_steps)
    print(f'importance_accum: {ms:.4f} ms  12 B x {numel} = {12 * numel / 1e6:.1f} MB  {12 * numel / ms / 1e6:.0f} GB/s')
