"""Pseudo-label step measurements, alternated in one process (as tools/incremental_ab.py).

1. The three new launches and clamd_ce_fwd_bwd_counted (ce4_kernel, the yardstick) at K = 21, c_old = 11, batch 16, 256 x 256: device events
   around 50 launches after warm-up, 5 rounds each, algorithmic bytes / median time.
2. The whole task-2 step of one grown UNet(11 -> 21, 3, 64): A = pseudo-labels (distill_lambda=0, adaptive: old-model forward + relabelling +
   weighted loss), B = DistillationCrossEntropy (old-model forward + distillation loss), alternated, fp32 and bf16.  B runs THIS tree's
   library, not a build of the commit before the feature: misc.hip's device code is byte-identical to that commit's (compared with
   llvm-objdump when the shared inline helpers moved to ce_common.hip.h) and trainer.py's distillation branch makes the same calls, but
   the two commits were not timed against each other.

    python tools/pseudo_ab.py > profiles/pseudo_label.txt        (--steps-only / --kernels-only: one half)
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import continual_learning_amd as C  # noqa: E402

lib, ptr = C._lib, C._lib.ptr
L = lib.load()
B, K, c_old, H, W, N = 16, 21, 11, 256, 256, 50
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


def kernels():
    torch.manual_seed(0)
    z = torch.randn(B, K, H, W, device='cuda') * 3
    zo = torch.randn(B, c_old, H, W, device='cuda') * 3
    y = torch.randint(c_old, K, (B, H, W), device='cuda')
    y[torch.rand(B, H, W, device='cuda') < 0.6] = 0
    d, l3 = torch.empty_like(z), torch.empty(3, device='cuda')
    wsb = L.clamd_ce_workspace_bytes()
    ws = torch.zeros(wsb // 4, device='cuda')
    hist = torch.zeros(c_old, 100, dtype=torch.int64, device='cuda')
    lib.call('clamd_pseudo_entropy_hist', ptr(zo), c_old, c_old, ptr(y), ptr(hist), 100, B, H, W, s)
    tau = C.thresholds_from_histogram(hist, 100)
    out, counts, nu = torch.empty_like(y), torch.empty(B, 2, dtype=torch.int32, device='cuda'), torch.empty(B, device='cuda')
    nh = torch.zeros(B, H, W, 32, dtype=torch.bfloat16, device='cuda')
    npx = B * H * W
    lib.call('clamd_ce_count', ptr(y), B, K, H, W, -100, ptr(ws), wsb, s)
    cases = {
        'pseudo_entropy_hist (60 % background)': (npx * (4 * c_old + 8), lambda: lib.call('clamd_pseudo_entropy_hist', ptr(zo), c_old, c_old, ptr(y), ptr(hist), 100, B, H, W, s)),
        'pseudo_label (60 % background)': (npx * (4 * c_old + 16), lambda: lib.call('clamd_pseudo_label', ptr(zo), c_old, c_old, ptr(y), ptr(tau), ptr(out), ptr(counts), ptr(nu), 0.0, B, H, W, -100, s)),
        'ce_fwd_bwd_weighted, bf16 NHWC copy': (npx * (2 * K * 4 + 8 + 64), lambda: lib.call('clamd_ce_fwd_bwd_weighted', ptr(z), ptr(out), ptr(nu), ptr(d), ptr(nh), 32, 1, ptr(l3), ptr(ws), wsb, B, K, H, W, -100, 1.0, s)),
        'ce_fwd_bwd_counted,  bf16 NHWC copy': (npx * (2 * K * 4 + 8 + 64), lambda: lib.call('clamd_ce_fwd_bwd_counted', ptr(z), ptr(out), ptr(d), ptr(nh), 32, 1, ptr(l3), ptr(ws), wsb, B, K, H, W, -100, 1.0, s)),
        'ce_fwd_bwd_weighted, no copy': (npx * (2 * K * 4 + 8), lambda: lib.call('clamd_ce_fwd_bwd_weighted', ptr(z), ptr(out), ptr(nu), ptr(d), None, 0, 0, ptr(l3), ptr(ws), wsb, B, K, H, W, -100, 1.0, s)),
        'ce_fwd_bwd_counted,  no copy': (npx * (2 * K * 4 + 8), lambda: lib.call('clamd_ce_fwd_bwd_counted', ptr(z), ptr(out), ptr(d), None, 0, 0, ptr(l3), ptr(ws), wsb, B, K, H, W, -100, 1.0, s)),
    }
    rounds = [{k: timed(fn) for k, (_, fn) in cases.items()} for _ in range(5)]
    for k, (nbytes, _) in cases.items():
        t = sorted(r[k] for r in rounds)
        print(f'{k:40s} {t[2]:7.1f} us (min {t[0]:.1f}, max {t[-1]:.1f})   {nbytes / 1e6:6.1f} MB algorithmic   {nbytes / t[2] / 1e6:.2f} TB/s')
    print(f'    accepted {int(counts[:, 1].sum())} of {int(counts[:, 0].sum())} background pixels; launch pairs include the finalize / weight launches')


def steps():
    for dtype in ('fp32', 'bf16'):
        x = torch.from_numpy(C.synth.images(9, B, 3, H, W)).cuda()
        yy = torch.from_numpy(C.synth.labels(9, B, H, W, K, class_lo=c_old, class_hi=K)).cuda()
        tr = C.Trainer([(x, yy)], C.default_config(n_iters=10000, num_classes=c_old, conv_dim=64, compute_dtype=dtype))
        tr.train_step(x, torch.from_numpy(C.synth.labels(9, B, H, W, K, class_lo=0, class_hi=c_old)).cuda())
        tr.begin_task2(c_old=c_old, distill_lambda=0, new_classes=K - c_old, pseudo_label=True, pseudo_adaptive=True)
        sides = {'A pseudo-labels': (tr.pseudo, None), 'B DistillationCrossEntropy': (None, C.DistillationCrossEntropy(c_old, 2.0, 1.0))}

        def run(name, n=10):
            tr.pseudo, tr.distill = sides[name]
            for _ in range(2):
                tr.train_step(x, yy)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                tr.train_step(x, yy)
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) / n

        rounds = [{name: run(name) for name in sides} for _ in range(4)]
        print(f'whole task-2 step {dtype}: ' + '   '.join(f'{name} {sorted(r[name] for r in rounds)[0]:.3f} ms (best of 4 rounds of 10; max {max(r[name] for r in rounds):.3f})'
                                                        for name in sides))
        del tr


if __name__ == '__main__':
    if '--steps-only' not in sys.argv:
        kernels()
    if '--kernels-only' not in sys.argv:
        steps()
