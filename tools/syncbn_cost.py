"""What synchronised BatchNorm adds to a train step on ONE GPU: a world-1 RCCL ("nccl") group, the model converted with
nn.SyncBatchNorm.convert_sync_batchnorm (18 forward + 18 backward all-reduces of 2 Cp + 1 doubles on the critical chain, plus the
totals / finalize launches) against the same model unconverted, interleaved in ONE process.  Config 2 of BASELINE.md by default
(UNet(21, 3, 64), 256 x 256, batch 16).  Same weights, same batch; the best round of each side is reported (ms per step).  A world-1
all-reduce moves no data: this is the launch and synchronisation overhead of the split path, not the cost over xGMI at 8 ranks.

    python tools/syncbn_cost.py --dtype fp32
    python tools/syncbn_cost.py --dtype bf16 --rounds 7
"""
import argparse
import os
import socket
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.distributed as dist
import torch.nn as nn

import continual_learning_amd as C

ap = argparse.ArgumentParser()
ap.add_argument('--dtype', default='fp32', choices=['fp32', 'bf16', 'bf16x3'])
ap.add_argument('--size', type=int, default=256)
ap.add_argument('--batch', type=int, default=16)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--steps', type=int, default=10)
a = ap.parse_args()

dev = torch.device('cuda', 0)
torch.cuda.set_device(dev)
with socket.socket() as s:
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK='0', WORLD_SIZE='1')
C.ddp.init_rccl(dev, rank=0, world_size=1)
x = torch.from_numpy(C.synth.images(1234, a.batch, 3, a.size, a.size)).to(dev)
y = torch.from_numpy(C.synth.labels(1234, a.batch, a.size, a.size, 21)).to(dev)
crit = C.CrossEntropyLoss()
runs = []
try:
    for mode in ('plain', 'sync'):
        torch.manual_seed(1234)
        m = C.UNet(21, 3, 64, compute_dtype=a.dtype).to(dev).train()
        if mode == 'sync':
            nn.SyncBatchNorm.convert_sync_batchnorm(m)
        o = C.FusedAdam(m.parameters(), lr=1e-4, betas=[0.5, 0.99])

        def step(m=m, o=o):
            out = m(x); o.zero_grad(); loss = crit(out, y); loss.backward(); o.step()
            return loss
        for _ in range(3):
            step()                    # builds the engine (and, on the converted side, the BatchNorm group's communicator)
        runs.append((mode, step))
    best = {k: 1e9 for k, _ in runs}
    for rd in range(a.rounds):
        for k, step in runs:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(a.steps):
                loss = step()
            torch.cuda.synchronize()
            best[k] = min(best[k], (time.perf_counter() - t0) / a.steps)
    print(a.dtype, f'{a.size}x{a.size} bs{a.batch}', '  '.join(f'{k}: {t * 1e3:.3f} ms/step' for k, t in best.items()),
          f'added: {(best["sync"] - best["plain"]) * 1e3:+.3f} ms/step', f'loss {float(loss.detach()):.4f}')
finally:
    dist.destroy_process_group()
