"""A/B of the class-incremental loss launch against the distillation path it replaces, alternated in one process (as tools/step_ab.py):

    new   clamd_ce_count + clamd_ce_unbiased_fwd_bwd (KD term, NHWC copy in the compute dtype)
    old   clamd_ce_fwd_bwd with the KD term (scalar kernel) + the clamd_nchw_to_nhwc pass the backward then makes

K = 21, c_old = 11, batch 16, 256 x 256; device events around 50 launches after warm-up, 5 rounds each (the spread of the same binary).
Then the whole task-2 step (old-model forward + forward + loss + backward + Adam) of one grown UNet(11 -> 21, 3, 64), unbiased=True against
unbiased=False (DistillationCrossEntropy), alternated, fp32 and bf16.

    python tools/incremental_ab.py > profiles/incremental_ab.txt
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import continual_learning_amd as C  # noqa: E402

lib, ptr = C._lib, C._lib.ptr
L = lib.load()
B, K, c_old, H, W, lam, N = 16, 21, 11, 256, 256, 10.0, 50
torch.manual_seed(0)
z = torch.randn(B, K, H, W, device='cuda') * 3
zo = torch.randn(B, c_old, H, W, device='cuda') * 3
y = torch.randint(0, K, (B, H, W), device='cuda')
d, l3 = torch.empty_like(z), torch.empty(3, device='cuda')
wsb = L.clamd_ce_workspace_bytes()
ws = torch.zeros(wsb // 4, device='cuda')
s = lib.stream_ptr()


def timed(fn):
    for _ in range(5):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(N):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / N


for name, dcode in (('fp32', 0), ('bf16', 1), ('bf16x3', 2)):
    nh = torch.zeros(B, H, W, 32, dtype=C.ops.TORCH_DT[dcode], device='cuda')
    esize = 2 if dcode == 1 else 4

    def new():
        lib.call('clamd_ce_count', ptr(y), B, K, H, W, -100, ptr(ws), wsb, s)
        lib.call('clamd_ce_unbiased_fwd_bwd', ptr(z), ptr(y), ptr(zo), c_old, c_old, lam, ptr(d), ptr(nh), 32, dcode, ptr(l3), ptr(ws), wsb,
                 B, K, H, W, -100, 1.0, s)

    def old():
        lib.call('clamd_ce_fwd_bwd', ptr(z), ptr(y), ptr(zo), c_old, c_old, 2.0, lam, ptr(d), ptr(l3), ptr(ws), wsb, B, K, H, W, -100, 1.0, s)
        lib.call('clamd_nchw_to_nhwc', ptr(d), ptr(nh), 32, B, K, H, W, 32, 1.0, dcode, s)

    rounds = [(timed(new), timed(old)) for _ in range(5)]
    tn, to = sorted(r[0] for r in rounds), sorted(r[1] for r in rounds)
    nbytes = B * H * W * ((2 * K + c_old) * 4 + 8 + 32 * esize)
    print(f'{name}: new {tn[2]:.1f} us (min {tn[0]:.1f}, max {tn[-1]:.1f})   old pair {to[2]:.1f} us (min {to[0]:.1f}, max {to[-1]:.1f})   '
          f'ratio {to[2] / tn[2]:.2f}x   new: {nbytes / 1e6:.0f} MB algorithmic, {nbytes / tn[2] / 1e6:.2f} TB/s')


# ---- the whole task-2 step on the same grown model, the two criteria alternated
for dtype in ('fp32', 'bf16'):
    x = torch.from_numpy(C.synth.images(9, B, 3, H, W)).cuda()
    yy = torch.from_numpy(C.synth.labels(9, B, H, W, K, class_lo=c_old, class_hi=K)).cuda()
    tr = C.Trainer([(x, yy)], C.default_config(n_iters=10000, num_classes=c_old, conv_dim=64, compute_dtype=dtype))
    tr.train_step(x, torch.from_numpy(C.synth.labels(9, B, H, W, K, class_lo=0, class_hi=c_old)).cuda())
    tr.begin_task2(c_old=c_old, distill_lambda=lam, new_classes=K - c_old, unbiased=True)
    crits = {'unbiased': tr.distill, 'plain CE + KD': C.DistillationCrossEntropy(c_old, 2.0, lam)}

    def steps(name, n=10):
        tr.distill = crits[name]
        for _ in range(2):
            tr.train_step(x, yy)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            tr.train_step(x, yy)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    rounds = [{name: steps(name) for name in crits} for _ in range(4)]
    print(f'whole task-2 step {dtype}: ' + '   '.join(f'{name} {sorted(r[name] for r in rounds)[0]:.3f} ms (best of 4 rounds of 10; max {max(r[name] for r in rounds):.3f})'
                                                    for name in crits))
    del tr
