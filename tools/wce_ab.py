"""Class-weighted / label-smoothed / focal cross-entropy measurements, alternated in one process (as tools/dice_ab.py).

clamd_ce_class_fwd_bwd (per-class count, totals, loss pass, finalize) in its three modes -- weights only, eps = 0.1, gamma = 2 -- against
clamd_ce_count + clamd_ce_fwd_bwd_counted at K = 21, 16 x 256 x 256, each with the bf16 NHWC copy (the training step's form) and without a
copy: device events around 50 calls after warm-up, 5 rounds, interleaved; median (min, max), the ratio of the medians, algorithmic bytes /
median time beside the float4 copy rate that bench.py measured on this part (a quoted constant, not measured here).  Algorithmic bytes:
the logits once, the labels twice (the count pass reads them too), d logits once, the NHWC copy once -- the same for every line.

    python tools/wce_ab.py > profiles/wce.txt
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import continual_learning_amd as C  # noqa: E402

K, B, H, W, N, ROUNDS = 21, 16, 256, 256, 50, 5
COPY_RATE = 6.29      # TB/s, a float4 copy on this part: QUOTED from bench.py's own measurement, not measured in this run
MODES = (('weights only', 0.0, 0.0), ('eps 0.1', 0.1, 0.0), ('gamma 2', 0.0, 2.0))


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


def main():
    lib, ptr, call = C._lib.load(), C._lib.ptr, C._lib.call
    z = torch.randn(B, K, H, W, device='cuda') * 3
    y = torch.from_numpy(C.synth.labels(9, B, H, W, K)).cuda()
    counts = C.class_pixel_counts(y, K).cpu()
    w = C.class_weights(counts, 'median_frequency').cuda()
    d = torch.empty_like(z)
    l3 = torch.empty(3, device='cuda')
    px = B * H * W
    s = C._lib.stream_ptr()
    wsn, wso = lib.clamd_ce_class_workspace_bytes(), lib.clamd_ce_workspace_bytes()
    wn, wo = torch.empty(wsn // 4, device='cuda'), torch.empty(wso // 4, device='cuda')
    print(f'K {K}, {B} x {H} x {W}, median-frequency weights of the batch: {N} calls per round, {ROUNDS} rounds, interleaved')
    for name, dcode, esize in (('bf16', 1, 2), (None, 0, 0)):
        nh = None if name is None else torch.empty(B, H, W, 32, dtype=C.ops.TORCH_DT[dcode], device='cuda')
        ldc = 0 if nh is None else 32

        def ce():
            call('clamd_ce_count', ptr(y), B, K, H, W, -100, ptr(wo), wso, s)
            call('clamd_ce_fwd_bwd_counted', ptr(z), ptr(y), ptr(d), ptr(nh), ldc, dcode, ptr(l3), ptr(wo), wso, B, K, H, W, -100, 1.0, s)
        cases = {'ce count + counted': ce}
        for mode, eps, gamma in MODES:
            cases[f'ce_class {mode}'] = lambda eps=eps, gamma=gamma: call(
                'clamd_ce_class_fwd_bwd', ptr(z), ptr(y), ptr(w), None, ptr(d), ptr(nh), ldc, dcode, ptr(l3), ptr(wn), wsn, B, K, H, W, -100, eps,
                gamma, 1.0, s)
        rounds = [{k: timed(fn) for k, fn in cases.items()} for _ in range(ROUNDS)]
        nbytes = px * (2 * K * 4 + 16 + 32 * esize)
        base = sorted(r['ce count + counted'] for r in rounds)
        print(f'  NHWC copy: {name}   ({nbytes / 1e6:.1f} MB algorithmic)')
        for k in cases:
            t = sorted(r[k] for r in rounds)
            note = '' if k == 'ce count + counted' else f'   x{t[ROUNDS // 2] / base[ROUNDS // 2]:.3f} of ce' + (
                ' (the spreads overlap)' if t[0] <= base[-1] and base[0] <= t[-1] else '')
            print(f'    {k:24s} {t[ROUNDS // 2]:8.1f} us (min {t[0]:.1f}, max {t[-1]:.1f})   {nbytes / t[ROUNDS // 2] / 1e6:.2f} TB/s '
                  f'(quoted copy rate {COPY_RATE}){note}')


if __name__ == '__main__':
    main()
