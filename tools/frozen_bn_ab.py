"""Interleaved A/B of the train-mode step against the frozen-BatchNorm step (every nn.BatchNorm2d in eval mode under model.train()) in ONE
process, config 2 of BASELINE.md by default (UNet(21, 3, 64), 256 x 256, batch 16).  Same weights, same batch, same optimizer; the two
models alternate in rounds of `--steps` steps and the best round of each is reported (ms per step).

    python tools/frozen_bn_ab.py --dtype fp32
    python tools/frozen_bn_ab.py --dtype bf16 --only frozen --rounds 1 --steps 5      # one side alone (under rocprofv3 --kernel-trace --stats)
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn

import continual_learning_amd as C

ap = argparse.ArgumentParser()
ap.add_argument('--dtype', default='fp32', choices=['fp32', 'bf16', 'bf16x3'])
ap.add_argument('--size', type=int, default=256)
ap.add_argument('--batch', type=int, default=16)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--steps', type=int, default=10)
ap.add_argument('--only', choices=['train', 'frozen'], default=None)
a = ap.parse_args()

dev = torch.device('cuda', 0)
x = torch.from_numpy(C.synth.images(1234, a.batch, 3, a.size, a.size)).to(dev)
y = torch.from_numpy(C.synth.labels(1234, a.batch, a.size, a.size, 21)).to(dev)
crit = C.CrossEntropyLoss()
runs = []
for mode in ([a.only] if a.only else ['train', 'frozen']):
    torch.manual_seed(1234)
    m = C.UNet(21, 3, 64, compute_dtype=a.dtype).to(dev).train()
    if mode == 'frozen':
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.eval()
    o = C.FusedAdam(m.parameters(), lr=1e-4, betas=[0.5, 0.99])

    def step(m=m, o=o):
        out = m(x); o.zero_grad(); loss = crit(out, y); loss.backward(); o.step()
        return loss
    for _ in range(3):
        step()                    # builds the engine
    runs.append((mode, step))
best = {k: 1e9 for k, _ in runs}
for rd in range(a.rounds):
    for k, step in runs:
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(a.steps):
            loss = step()
        torch.cuda.synchronize()
        best[k] = min(best[k], (time.perf_counter() - t0) / a.steps)
print(a.dtype, f'{a.size}x{a.size} bs{a.batch}', '  '.join(f'{k}: {t * 1e3:.3f} ms/step ({a.batch / t:.1f} img/s)' for k, t in best.items()),
      f'loss {float(loss.detach()):.4f}')
