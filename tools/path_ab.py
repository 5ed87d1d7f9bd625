"""Interleaved A/B of the optimiser steps with and without the path integral of Synaptic Intelligence in ONE process, on the 82 tensors of
UNet(21, 3, 64) with fixed gradients: the Adam and SGD steps alone, plain and tracked (device events around `--opt-steps` back-to-back
steps, after warm-up), and the unfused composition from stock torch -- a clone of the parameters before the plain step, then `_foreach`
ops for omega -= g * (p - before) -- each with its algorithmic bytes and GB/s; then the boundary pass clamd_path_importance alone.

    python tools/path_ab.py
    python tools/path_ab.py --only adam_tracked --rounds 1 --opt-steps 20         # one side alone (under rocprofv3 --kernel-trace --stats)
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import continual_learning_amd as C

SIDES = ['adam_plain', 'adam_tracked', 'adam_unfused', 'sgd_plain', 'sgd_tracked', 'sgd_unfused']
ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--opt-steps', type=int, default=200)
ap.add_argument('--only', choices=SIDES, default=None)
a = ap.parse_args()

dev = torch.device('cuda', 0)
# the step's own bytes per parameter, and what the path integral adds: fused, omega read and written; unfused, the clone (p read, the copy
# written) and the pass over g, both copies of theta and omega (four reads, one write)
BYTES = {'adam_plain': 28, 'adam_tracked': 36, 'adam_unfused': 28 + 8 + 20, 'sgd_plain': 20, 'sgd_tracked': 28, 'sgd_unfused': 20 + 8 + 20}
runs = []
for side in ([a.only] if a.only else SIDES):
    kind, mode = side.split('_')
    torch.manual_seed(1234)
    m = C.UNet(21, 3, 64).to(dev).train()
    params = list(m.parameters())
    g = torch.Generator(device=dev).manual_seed(1)
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=g) * 1e-3
    if kind == 'adam':
        o = C.FusedAdam(params, lr=1e-4, betas=[0.5, 0.99])
    else:
        o = C.FusedSGD(params, lr=1e-4, momentum=0.9, nesterov=True, weight_decay=1e-4)
    path = C.PathIntegral(m.named_parameters())
    if mode == 'tracked':
        o.set_path_integral(path.omega)
    step = o.step
    if mode == 'unfused':
        grads = [p.grad for p in params]
        datas = [p.detach() for p in params]

        def step(o=o, datas=datas, grads=grads, omega=path.omega):
            before = [p.clone() for p in datas]
            o.step()
            delta = torch._foreach_sub(datas, before)
            torch._foreach_addcmul_(omega, grads, delta, value=-1.0)
    runs.append((side, step, m, o, path))


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


numel = 0
for rd in range(a.rounds):
    for k, step, m, _, _ in runs:
        numel = sum(p.numel() for p in m.parameters())
        ms = timed(step, a.opt_steps)
        print(f'{k}: {ms:.4f} ms  {BYTES[k]} B x {numel} = {BYTES[k] * numel / 1e6:.1f} MB  {BYTES[k] * numel / ms / 1e6:.0f} GB/s')
# the boundary pass alone: importance = decay * importance + max(0, omega) / ((p - start)^2 + xi) over all 82 tensors in one launch
_, _, m, _, path = runs[-1]
from continual_learning_amd import _lib                     # noqa: E402
from continual_learning_amd.consolidate import _PATH_ROW_DT  # noqa: E402
cons = C.Consolidation(m.named_parameters())
rows = [(w.data_ptr(), om.data_ptr(), p.data_ptr(), s.data_ptr(), w.numel())
        for w, om, p, s in zip(cons.importance, path.omega, m.parameters(), path.start)]
tab, chunks, nchunks = _lib.job_table(_PATH_ROW_DT, rows, [w.numel() for w in cons.importance], dev, 'clamd_sizeof_path_tensor')
for rd in range(a.rounds):
    ms = timed(lambda: _lib.call('clamd_path_importance', _lib.ptr(tab), _lib.ptr(chunks), nchunks, 1.0, path.xi, _lib.stream_ptr()), a.opt_steps)
    print(f'path_importance: {ms:.4f} ms  20 B x {numel} = {20 * numel / 1e6:.1f} MB  {20 * numel / ms / 1e6:.0f} GB/s')
