"""CPU: pseudo-labelling of the old classes in the task step (build-defined: the reference has no continual-learning code, parity unpinned).

The restatement of include/clamd.h's definitions (``pseudo_reference``, ``weighted_ce``, shared with tests/test_pseudo_label_gpu.py) is pinned
here: against itself in float32 / float64 away from the bin edges, against F.cross_entropy and autograd, and the thresholds against
hand-made histograms.  Binning and ``u < tau`` are step functions, so a pixel within rounding of a bin edge may fall either way; the inputs
therefore take such pixels OUT of the candidate set (``masked_case`` gives them label 1) instead of tolerating mismatches."""
import math
import os
import re
import socket
import subprocess

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

import continual_learning_amd as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DELTA = 2e-5           # half-width of the band around every bin edge that is taken out of the candidate set
MASK_CAP = 0.05        # at most this share of the pixels may be taken out
# (B, c_old, H, W, scale of the randn old logits)
SHAPES = [(4, 11, 64, 64, 3.0), (2, 11, 64, 64, 8.0), (3, 21, 32, 48, 3.0), (2, 2, 32, 32, 3.0), (16, 11, 256, 256, 3.0)]


def entropy_u(zo, c_old, dtype=torch.float64):
    """(c*, u) per pixel: the first arg-max of zo[:, :c_old] and the entropy of its softmax over ln(c_old), in `dtype`."""
    z = zo[:, :c_old].to(dtype)
    cstar = z.argmax(1)                                    # torch: the first of several maxima
    if c_old == 1:
        return cstar, torch.zeros_like(z[:, 0])
    logq = torch.log_softmax(z, 1)
    return cstar, -(logq.exp() * logq).sum(1) / math.log(c_old)


def pseudo_reference(zo, labels, c_old, NB, dtype=torch.float64, thresholds=None, ignore_index=-100, min_factor=0.0):
    """include/clamd.h's definitions with stock torch ops in `dtype` -> dict(cstar, u, bin, hist) and, with thresholds (float32 [c_old]),
    labels_out, counts (int64 [B, 2] = {n_bg, n_acc}) and nu (float32 [B])."""
    cstar, u = entropy_u(zo, c_old, dtype)
    bins = torch.floor(u * NB).long().clamp(0, NB - 1)      # u >= 0 up to rounding
    cand = labels == 0
    hist = torch.bincount((cstar * NB + bins)[cand], minlength=c_old * NB).view(c_old, NB)
    out = dict(cstar=cstar, u=u, bin=bins, hist=hist)
    if thresholds is not None:
        tau = thresholds.to(device=u.device, dtype=torch.float32).to(dtype)
        acc = cand & (u < tau[cstar])
        out['labels_out'] = torch.where(cand, torch.where(acc, cstar, torch.full_like(cstar, ignore_index)), labels)
        nbg, nacc = cand.sum((1, 2)), acc.sum((1, 2))
        out['counts'] = torch.stack([nbg, nacc], 1)
        share = torch.clamp(nacc.float() / nbg.clamp(min=1).float(), min=float(min_factor))
        out['nu'] = torch.where(nbg > 0, share, torch.ones_like(share))
    return out


def edge_mask(zo, c_old, NB, delta=DELTA):
    """Pixels whose float64 u lies within delta of a multiple of 1 / NB.  c_old == 1: u is exactly 0 in every precision, nothing to mask."""
    if c_old == 1:
        return torch.zeros(zo.shape[0], *zo.shape[2:], dtype=torch.bool)
    _, u = entropy_u(zo, c_old, torch.float64)
    r = u * NB
    return (r - r.round()).abs() / NB < delta


def masked_case(B, c_old, H, W, scale, seed=0, NB=100, k_total=None, K=None):
    """randn * scale old logits and task-2 style labels (about 60 % background, new classes c_old .. K-1, a few ignored / out-of-range
    values), the pixels near a bin edge relabelled 1 -> (zo, labels, masked share)."""
    g = torch.Generator().manual_seed(seed)
    K = K or min(32, c_old + 10)
    zo = torch.randn(B, k_total or c_old, H, W, generator=g) * scale
    y = torch.randint(c_old, K, (B, H, W), generator=g) if K > c_old else torch.ones(B, H, W, dtype=torch.int64)
    y[torch.rand(B, H, W, generator=g) < 0.6] = 0
    y[0, 0, :3] = -100; y[0, 1, 0] = K + 2; y[-1, -1, -1] = -7          # ignored, out of range, negative non-ignore
    m = edge_mask(zo, c_old, NB)
    y[m] = 1
    return zo, y, float(m.float().mean())


def weighted_ce(z, y, nu, ignore_index=-100):
    """loss = (1 / max(N, 1)) * sum_b nu_b * sum_{valid p in b} -log softmax(z_p)[y_p], N the unweighted count of valid pixels; autograd-able."""
    K = z.shape[1]
    valid = (y != ignore_index) & (y >= 0) & (y < K)
    nll = -torch.log_softmax(z, 1).gather(1, y.clamp(0, K - 1)[:, None])[:, 0]
    return (nll * valid * nu.to(z.dtype)[:, None, None]).sum() / max(int(valid.sum()), 1)


def weighted_ce_grad(z, y, nu, ignore_index=-100):
    """The closed form of the header: nu_b * (softmax - onehot) / max(N, 1) on valid pixels, 0 elsewhere."""
    K = z.shape[1]
    valid = (y != ignore_index) & (y >= 0) & (y < K)
    g = torch.softmax(z, 1) - F.one_hot(y.clamp(0, K - 1), K).permute(0, 3, 1, 2).to(z.dtype)
    return g * valid[:, None] * nu.to(z.dtype)[:, None, None, None] / max(int(valid.sum()), 1)


# ------------------------------------------------------------------------------------------------------------------------- entry points
@pytest.mark.parametrize('name,nargs', [('clamd_pseudo_entropy_hist', 10), ('clamd_pseudo_label', 14), ('clamd_ce_fwd_bwd_weighted', 17)])
def test_entry_points_in_header_ctypes_table_and_library(name, nargs):
    header = open(os.path.join(ROOT, 'include', 'clamd.h')).read()
    m = re.search(r'int\s+' + name + r'\s*\(([^;]*)\)\s*;', header)
    assert m, 'prototype missing from include/clamd.h'
    assert len(m.group(1).split(',')) == len(C._lib.SIGNATURES[name][1]) == nargs
    out = subprocess.run(['nm', '-D', '--defined-only', C._lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r'\sT\s+' + name + r'\s*$', out, re.M), 'libclamd.so does not export the entry point'


def test_weighted_argument_list_is_the_counted_one_plus_image_weight():
    header = open(os.path.join(ROOT, 'include', 'clamd.h')).read()
    args = {}
    for name in ('clamd_ce_fwd_bwd_counted', 'clamd_ce_fwd_bwd_weighted'):
        m = re.search(r'int\s+' + name + r'\s*\(([^;]*)\)\s*;', header)
        args[name] = [' '.join(a.split()) for a in m.group(1).split(',')]
    extra = [a for a in args['clamd_ce_fwd_bwd_weighted'] if a not in args['clamd_ce_fwd_bwd_counted']]
    assert extra == ['const float* image_weight']
    assert [a for a in args['clamd_ce_fwd_bwd_weighted'] if a not in extra] == args['clamd_ce_fwd_bwd_counted']


# --------------------------------------------------------------------------------------------- comparability of the step functions
@pytest.mark.parametrize('B,c_old,H,W,scale', SHAPES)
def test_masking_keeps_float32_and_float64_decisions_equal(B, c_old, H, W, scale):
    """The restatement alone stays inside the condition the GPU tests rely on: at most 5 % of the pixels are taken out, and on the rest a
    float32 evaluation bins and decides exactly as the float64 one."""
    NB = 100
    zo, y, share = masked_case(B, c_old, H, W, scale, seed=c_old + H)
    print(f'B{B} c{c_old} {H}x{W} x{scale}: masked share {100 * share:.2f} %')
    assert share <= MASK_CAP, share
    r64 = pseudo_reference(zo, y, c_old, NB, torch.float64)
    tau = C.thresholds_from_histogram(r64['hist'], NB)
    r64 = pseudo_reference(zo, y, c_old, NB, torch.float64, thresholds=tau, min_factor=0.3)
    r32 = pseudo_reference(zo, y, c_old, NB, torch.float32, thresholds=tau, min_factor=0.3)
    du = float((r32['u'].double() - r64['u']).abs().max())
    print(f'    max |u32 - u64| {du:.2e} (delta {DELTA:.0e})')
    # u <= 1 is a sum of c_old products of fp32 values: a few ulp of 1 (2^-24 = 6e-8 each), 1e-6 = 16 ulp, 20x inside delta
    assert du < 1e-6, du
    cand = y == 0
    assert torch.equal(r32['cstar'], r64['cstar'])
    assert torch.equal(r32['bin'][cand], r64['bin'][cand])
    assert torch.equal(r32['hist'], r64['hist']) and int(r64['hist'].sum()) == int(cand.sum())
    assert torch.equal(r32['labels_out'], r64['labels_out']) and torch.equal(r32['counts'], r64['counts'])
    assert torch.equal(r32['nu'], r64['nu'])
    # pass-through: everything that was not a candidate is what it was
    assert torch.equal(r64['labels_out'][~cand], y[~cand])
    assert set(r64['labels_out'][cand].unique().tolist()) <= set(range(c_old)) | {-100}


def test_reference_c_old_1_and_tie_rule():
    zo = torch.randn(2, 3, 4, 4)
    y = torch.zeros(2, 4, 4, dtype=torch.int64)
    r = pseudo_reference(zo, y, 1, 10, thresholds=torch.tensor([0.1]))
    assert float(r['u'].abs().max()) == 0.0 and int(r['cstar'].max()) == 0 and int(r['hist'][0, 0]) == 32
    assert torch.equal(r['labels_out'], y) and r['counts'].tolist() == [[16, 16], [16, 16]]
    zo = torch.tensor([1.0, 3.0, 3.0, 3.0, 0.0]).view(1, 5, 1, 1).expand(1, 5, 2, 2).contiguous()
    assert pseudo_reference(zo, torch.zeros(1, 2, 2, dtype=torch.int64), 5, 10)['cstar'].unique().tolist() == [1]


# ----------------------------------------------------------------------------------------------------------------------------- thresholds
def test_thresholds_from_hand_made_histograms():
    NB = 10
    h = torch.zeros(7, NB, dtype=torch.int64)
    # class 0: empty -> 0
    h[1, 2] = 1; h[1, 4] = 1; h[1, 7] = 1            # odd: n = 3, ceil = 2 -> reached in bin 4 -> 0.5
    h[2, 1] = 2; h[2, 6] = 2                          # even: n = 4, ceil = 2 -> reached in bin 1 -> 0.2
    h[3, NB - 1] = 9                                  # all mass in the last bin -> 1.0
    h[4, 3] = 1                                       # one pixel -> its bin's upper edge
    h[5, 0] = 1; h[5, 9] = 2                          # n = 3, ceil = 2 -> bin 9 -> 1.0
    h[6, 0] = 5; h[6, 5] = 4                          # n = 9, ceil = 5 -> bin 0 -> 0.1
    tau = C.thresholds_from_histogram(h, NB)
    assert tau.dtype == torch.float32 and tau.tolist() == [0.0] + [float(torch.tensor(v, dtype=torch.float32)) for v in (0.5, 0.2, 1.0, 0.4, 1.0, 0.1)]
    assert C.thresholds_from_histogram(h.int()).tolist() == tau.tolist()
    with pytest.raises(ValueError):
        C.thresholds_from_histogram(h, NB + 1)
    with pytest.raises(ValueError):
        C.thresholds_from_histogram(h.float(), NB)
    # against the definition, class by class, on random histograms
    g = torch.Generator().manual_seed(1)
    h = torch.randint(0, 50, (11, 100), generator=g) * (torch.rand(11, 100, generator=g) < 0.3)
    tau = C.thresholds_from_histogram(h, 100)
    for c in range(11):
        n = int(h[c].sum())
        want, run = 0.0, 0
        for j in range(100):
            run += int(h[c, j])
            if n and run >= (n + 1) // 2:
                want = (j + 1) / 100
                break
        assert float(tau[c]) == float(torch.tensor(want, dtype=torch.float32)), (c, float(tau[c]), want)


def _gloo_finish_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        lab = C.PseudoLabeler(5, bins=20)
        lab.hist = torch.randint(0, 30, (5, 20), generator=torch.Generator().manual_seed(10 + rank))
        lab.hist[3] = 0
        own = C.thresholds_from_histogram(lab.hist, 20)
        mine = lab.hist.clone()
        lab.finish()
        first = lab.thresholds.clone()
        lab.finish()                                       # again: the other rank's counts are not added a second time
        q.put((rank, own.tolist(), lab.thresholds.tolist(), lab.hist_total.tolist(), torch.equal(lab.hist, mine) and torch.equal(first, lab.thresholds)))
    finally:
        dist.destroy_process_group()


def test_finish_all_reduces_the_histogram_gloo_world2():
    world = 2
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    ps = [ctx.Process(target=_gloo_finish_worker, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = sorted(q.get(timeout=180) for _ in range(world))
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    hists = [torch.randint(0, 30, (5, 20), generator=torch.Generator().manual_seed(10 + r)) for r in range(world)]
    for h in hists:
        h[3] = 0
    total = hists[0] + hists[1]
    want = C.thresholds_from_histogram(total, 20).tolist()
    for rank, own, got, hist, kept in res:
        assert got == want and hist == total.tolist(), rank
        assert kept, 'finish() must leave the rank\'s own histogram as it was and give the same thresholds when called again'
    assert len({tuple(r[1]) for r in res}) == 2
    assert want[3] == 0.0


def test_finish_without_a_batch_and_call_without_thresholds():
    lab = C.PseudoLabeler(3)
    with pytest.raises(RuntimeError, match='no batch'):
        lab.finish()
    with pytest.raises(RuntimeError, match='thresholds'):
        lab(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))
    assert C.PseudoLabeler(3, thresholds=0.25).thresholds.tolist() == [0.25] * 3
    assert C.PseudoLabeler(2, thresholds=torch.tensor([0.5, 1.0])).thresholds.tolist() == [0.5, 1.0]
    with pytest.raises(ValueError):
        C.PseudoLabeler(3, thresholds=torch.tensor([0.5, 1.0]))
    with pytest.raises(ValueError):
        C.PseudoLabeler(0)
    with pytest.raises(ValueError):
        C.PseudoLabeler(32, bins=1000)


# ------------------------------------------------------------------------------------------------------------------------------ the loss
def test_weighted_ce_with_unit_weights_is_cross_entropy():
    torch.manual_seed(2)
    z = torch.randn(3, 7, 6, 5, dtype=torch.float64) * 3
    y = torch.randint(0, 7, (3, 6, 5)); y[0, 0, :2] = -100
    assert abs(float(weighted_ce(z, y, torch.ones(3))) - float(F.cross_entropy(z, y))) < 1e-14


def test_weighted_ce_closed_form_gradient_equals_autograd():
    torch.manual_seed(4)
    z = (torch.randn(3, 21, 6, 8, dtype=torch.float64) * 3).requires_grad_()
    y = torch.randint(0, 21, (3, 6, 8)); y[0, 0, :3] = -100; y[1, 2, 2] = 25; y[1, 3, 3] = -7
    nu = torch.tensor([0.25, 1.0, 0.0])
    g, = torch.autograd.grad(weighted_ce(z, y, nu), z)
    e = float((g - weighted_ce_grad(z.detach(), y, nu)).abs().max())
    assert e < 1e-14, e
    assert float(g[2].abs().max()) == 0.0 and float(g[0, :, 0, :3].abs().max()) == 0.0
    # the mean is over the UNWEIGHTED count: halving every weight halves the loss
    a, b = float(weighted_ce(z, y, torch.ones(3))), float(weighted_ce(z, y, torch.full((3,), 0.5)))
    assert abs(b - 0.5 * a) < 1e-14


def test_weighted_ce_all_pixels_ignored():
    z = torch.randn(2, 5, 4, 4, dtype=torch.float64, requires_grad=True)
    y = torch.full((2, 4, 4), -100)
    loss = weighted_ce(z, y, torch.tensor([0.3, 0.7]))
    g, = torch.autograd.grad(loss, z)
    assert float(loss) == 0.0 and float(g.abs().max()) == 0.0


# --------------------------------------------------------------------------------------------------------------------------- host checks
def test_cpu_tensors_are_refused():
    lab = C.PseudoLabeler(3, thresholds=0.5)
    zo, y = torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        lab(zo, y)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        lab.accumulate(zo, y)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        C.CrossEntropyLoss()(torch.zeros(1, 5, 4, 4), y, torch.ones(1))


def test_begin_task2_refuses_the_two_combinations():
    tr = C.Trainer([], C.default_config(num_classes=5, conv_dim=4), device='cpu')
    with pytest.raises(ValueError, match='unbiased'):
        tr.begin_task2(c_old=5, distill_lambda=10.0, unbiased=True, pseudo_label=True)
    with pytest.raises(ValueError, match='per-image weight'):
        tr.begin_task2(c_old=5, distill_lambda=1.0, pseudo_label=True, pseudo_adaptive=True)
    assert tr.old_model is None and tr.pseudo is None          # refused before anything was switched on
