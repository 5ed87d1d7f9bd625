"""Interleaved A/B of clipping by the global gradient norm in ONE process, on the 82 tensors of UNet(21, 3, 64) with fixed gradients, for
FusedSGD and FusedAdam: (a) the plain fused step, (b) the norm pass + finalize + the step on the effective scale (set_grad_clip), and
(c) torch.nn.utils.clip_grad_norm_(foreach=True) followed by the plain fused step -- device events around `--opt-steps` back-to-back steps,
after warm-up, each with its algorithmic bytes and GB/s; then clamd_grad_norm_clip alone.  The learning rate is 0 so that every step sees
the same state, and (c)'s max_norm lies above the norm: the foreach pass still multiplies every gradient (by 1), as it does in training,
without driving them to zero over the repetitions.

    python tools/clip_ab.py
    python tools/clip_ab.py --only sgd_fused --rounds 1 --opt-steps 20         # one side alone (under rocprofv3 --kernel-trace --stats)
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import continual_learning_amd as C
from continual_learning_amd import _lib

SIDES = ['sgd_plain', 'sgd_fused', 'sgd_foreach', 'adam_plain', 'adam_fused', 'adam_foreach']
ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--opt-steps', type=int, default=200)
ap.add_argument('--only', choices=SIDES, default=None)
a = ap.parse_args()

dev = torch.device('cuda', 0)
# the step's own bytes per parameter, and what clipping adds: fused, every gradient read once more; foreach, the norm's read and the
# in-place multiply's read and write
STEP = {'sgd': 20, 'adam': 28}
EXTRA = {'plain': 0, 'fused': 4, 'foreach': 12}
MAX_NORM = 1e6
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
        o = C.FusedAdam(params, lr=0.0, betas=[0.5, 0.99])
    else:
        o = C.FusedSGD(params, lr=0.0, momentum=0.9, nesterov=True, weight_decay=1e-4)
    if mode == 'fused':
        o.set_grad_clip(MAX_NORM)
    step = o.step
    if mode == 'foreach':
        def step(o=o, params=params):
            torch.nn.utils.clip_grad_norm_(params, MAX_NORM, foreach=True)
            o.step()
    runs.append((side, step, m, o))


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
    for k, step, m, _ in runs:
        kind, mode = k.split('_')
        per = STEP[kind] + EXTRA[mode]
        numel = sum(p.numel() for p in m.parameters())
        ms = timed(step, a.opt_steps)
        print(f'{k}: {ms:.4f} ms  {per} B x {numel} = {per * numel / 1e6:.1f} MB  {per * numel / ms / 1e6:.0f} GB/s')
# the norm pass and its finalize alone, on the tables of a clipping optimiser
for k, _, m, o in runs:
    if k.endswith('_fused'):
        ptr = _lib.ptr
        n = len(o.param_groups[0]['params'])
        call = lambda: _lib.call('clamd_grad_norm_clip', ptr(o._clip_tab), n, ptr(o._chunks_dev), o._nchunks, ptr(o._hyper), MAX_NORM,
                                 ptr(o._clip_part), ptr(o._clip_out), ptr(o._tensor_norms), ptr(o._hyper_eff), _lib.stream_ptr())
        for rd in range(a.rounds):
            ms = timed(call, a.opt_steps)
            print(f'grad_norm_clip: {ms:.4f} ms  4 B x {numel} = {4 * numel / 1e6:.1f} MB  {4 * numel / ms / 1e6:.0f} GB/s  '
                  f'({o._nchunks} + 1 workgroups, 2 launches; norm {float(o.grad_norm):.6g})')
        break
