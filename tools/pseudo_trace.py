"""A few task-1 steps (plain loss: ce4_kernel, the yardstick) and a few pseudo-label task-2 steps at batch 16, 256 x 256, c_old = 11 -> 21
classes, bf16, for a kernel trace:

    rocprofv3 --kernel-trace --stats -d <dir> -o pseudo -- python tools/pseudo_trace.py
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import continual_learning_amd as C  # noqa: E402

B, K, c_old, H, W = 16, 21, 11, 256, 256
x = torch.from_numpy(C.synth.images(9, B, 3, H, W)).cuda()
y1 = torch.from_numpy(C.synth.labels(9, B, H, W, K, class_lo=0, class_hi=c_old)).cuda()
y2 = torch.from_numpy(C.synth.labels(9, B, H, W, K, class_lo=c_old, class_hi=K)).cuda()
tr = C.Trainer([(x, y2)], C.default_config(n_iters=10000, num_classes=c_old, conv_dim=64, compute_dtype='bf16'))
for _ in range(3):
    tr.train_step(x, y1)
tr.begin_task2(c_old=c_old, distill_lambda=0, new_classes=K - c_old, pseudo_label=True, pseudo_adaptive=True)
for _ in range(5):
    tr.train_step(x, y2)
counts = tr.pseudo.counts
tr.pseudo = None                      # the plain loss at 21 classes in the same trace: the plain ce4_kernel<24, 4> beside the weighted one
for _ in range(5):
    tr.train_step(x, y2)
torch.cuda.synchronize()
print(f'last pseudo-label step: accepted {counts[:, 1].tolist()} of {counts[:, 0].tolist()} background pixels per image')
