"""CPU: the class-incremental task step (build-defined: the reference has no continual-learning code, parity unpinned).

The float64 restatement of the two loss terms (``unbiased_losses``, shared with tests/test_incremental_gpu.py) is pinned here against the
closed-form gradients of include/clamd.h and against F.cross_entropy; head growth, FusedAdam.replace_params and Consolidation.grow are
checked as far as they need no device."""
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


def unbiased_losses(z, y, zo, c_old, lam, ignore_index=-100):
    """{total, ce, kd} of include/clamd.h's definitions with autograd-able torch ops in z's dtype.  z [B,K,H,W], y [B,H,W], zo [B,>=c_old,H,W]
    or None."""
    K = z.shape[1]
    lse_all = torch.logsumexp(z, 1)
    lse_old = torch.logsumexp(z[:, :c_old], 1)
    valid = (y != ignore_index) & (y >= 0) & (y < K)
    yc = y.clamp(0, K - 1)
    logp = torch.where(yc < c_old, lse_old - lse_all, z.gather(1, yc[:, None])[:, 0] - lse_all)
    ce = -(logp * valid).sum() / max(int(valid.sum()), 1)
    kd = z.new_zeros(())
    if zo is not None and lam != 0:
        q = torch.softmax(zo[:, :c_old].to(z.dtype), 1)
        lse_bg = torch.logsumexp(torch.cat([z[:, :1], z[:, c_old:]], 1), 1)
        logpt = torch.cat([(lse_bg - lse_all)[:, None], z[:, 1:c_old] - lse_all[:, None]], 1)
        kd = lam * (-(q * logpt).sum(1) / c_old).mean()
    return ce + kd, ce, kd


def closed_form_grads(z, y, zo, c_old, lam, ignore_index=-100):
    """The two gradients as the issue / header state them."""
    B, K, H, W = z.shape
    sm = torch.softmax(z, 1)
    valid = (y != ignore_index) & (y >= 0) & (y < K)
    yc = y.clamp(0, K - 1)
    smo = torch.zeros_like(z)
    smo[:, :c_old] = torch.softmax(z[:, :c_old], 1)
    g_ce = torch.where((yc < c_old)[:, None], sm - smo, sm - F.one_hot(yc, K).permute(0, 3, 1, 2).to(z.dtype))
    g_ce = g_ce * valid[:, None] / max(int(valid.sum()), 1)
    q = torch.softmax(zo[:, :c_old].to(z.dtype), 1)
    bg = torch.ones(K, dtype=torch.bool); bg[1:c_old] = False
    lse_bg = torch.logsumexp(z[:, bg], 1)
    g_kd = sm.clone()
    g_kd[:, bg] -= q[:, :1] * torch.exp(z[:, bg] - lse_bg[:, None])
    g_kd[:, 1:c_old] -= q[:, 1:]
    return g_ce, g_kd * lam / (c_old * B * H * W)


def test_entry_point_in_header_ctypes_table_and_library():
    name = 'clamd_ce_unbiased_fwd_bwd'
    header = open(os.path.join(ROOT, 'include', 'clamd.h')).read()
    m = re.search(r'int\s+' + name + r'\s*\(([^;]*)\)\s*;', header)
    assert m, 'prototype missing from include/clamd.h'
    assert len(m.group(1).split(',')) == len(C._lib.SIGNATURES[name][1]) == 20
    out = subprocess.run(['nm', '-D', '--defined-only', C._lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r'\sT\s+' + name + r'\s*$', out, re.M), 'libclamd.so does not export the entry point'


def test_expand_classes_shapes_keys_and_old_rows():
    torch.manual_seed(0)
    m = C.UNet(11, 3, 8)
    w0, b0 = m.last[6].weight.detach().clone(), m.last[6].bias.detach().clone()
    keys0 = list(m.state_dict())
    ow, ob, nw, nb = m.expand_classes(10)
    want = C.UNet(21, 3, 8)
    assert m.num_classes == 21 and m._table[-1]['tail'][3] == 21 and m.last._block_spec[0]['tail'][3] == 21 and not m._engines
    assert list(m.state_dict()) == keys0 == list(want.state_dict())
    assert [tuple(v.shape) for v in m.state_dict().values()] == [tuple(v.shape) for v in want.state_dict().values()]
    assert [n for n, _ in m.named_parameters()] == [n for n, _ in want.named_parameters()] and len(list(m.parameters())) == 82
    assert len(m.state_dict()) == 136
    assert nw is m.last[6].weight and nb is m.last[6].bias and nw.requires_grad and nb.requires_grad
    assert torch.equal(ow, w0) and torch.equal(nw[:11], w0) and torch.equal(nb[1:11], b0[1:])
    assert torch.equal(nw[11:], w0[:1].expand(10, -1, -1, -1))
    assert float(nb[0]) == pytest.approx(float(b0[0]) - math.log(11), abs=1e-6) and torch.equal(nb[11:], nb[:1].expand(10))
    want.load_state_dict(m.state_dict(), strict=True)
    with pytest.raises(ValueError, match='exceed'):
        m.expand_classes(12)
    for bad in (0, -3):
        with pytest.raises(ValueError, match='positive'):
            m.expand_classes(bad)
    with pytest.raises(ValueError, match='init'):
        m.expand_classes(1, init='zeros')
    m.expand_classes(11, init='default')
    assert m.num_classes == 32 and torch.equal(m.last[6].weight[:21], nw)


def test_default_init_is_seeded_and_leaves_old_rows():
    rows = []
    for _ in range(2):
        torch.manual_seed(3)
        m = C.UNet(5, 3, 8)
        w0 = m.last[6].weight.detach().clone()
        torch.manual_seed(11)
        m.expand_classes(4, init='default')
        assert torch.equal(m.last[6].weight[:5], w0)
        rows.append(m.last[6].weight[5:].detach().clone())
    assert torch.equal(rows[0], rows[1]) and float(rows[0].abs().max()) > 0 and not torch.equal(rows[0][0], w0[0])


def test_background_init_softmax_identity_float64():
    torch.manual_seed(1)
    m = C.UNet(11, 3, 8).double()
    with torch.no_grad():
        m.last[6].bias.normal_()
    feat = torch.randn(3, 8, 9, 7, dtype=torch.float64) * 3
    p = torch.softmax(F.conv2d(feat, m.last[6].weight, m.last[6].bias), 1)
    m.expand_classes(10)
    assert m.last[6].weight.dtype == torch.float64
    p2 = torch.softmax(F.conv2d(feat, m.last[6].weight, m.last[6].bias), 1)
    e_old = float((p2[:, 1:11] - p[:, 1:]).abs().max())
    e_bg = float((p2[:, 0] + p2[:, 11:].sum(1) - p[:, 0]).abs().max())
    assert e_old < 1e-12 and e_bg < 1e-12, (e_old, e_bg)


def test_restatement_c_old_1_is_cross_entropy():
    torch.manual_seed(2)
    z = torch.randn(2, 7, 6, 5, dtype=torch.float64) * 3
    y = torch.randint(0, 7, (2, 6, 5)); y[0, 0, :2] = -100
    tot, ce, kd = unbiased_losses(z, y, None, 1, 0.0)
    assert abs(float(ce) - float(F.cross_entropy(z, y))) < 1e-14 and float(kd) == 0.0 and float(tot) == float(ce)


@pytest.mark.parametrize('K,c_old', [(21, 11), (5, 5), (32, 31), (21, 1)])
def test_closed_form_gradients_equal_autograd(K, c_old):
    torch.manual_seed(4)
    z = (torch.randn(2, K, 6, 8, dtype=torch.float64) * 3).requires_grad_()
    zo = torch.randn(2, c_old + (K > c_old), 6, 8, dtype=torch.float64) * 3
    y = torch.randint(0, K, (2, 6, 8)); y[0, 0, :3] = -100; y[1, 2, 2] = K + 4; y[1, 3, 3] = -7
    tot, ce, kd = unbiased_losses(z, y, zo, c_old, 10.0)
    g_ce, = torch.autograd.grad(ce, z, retain_graph=True)
    g_kd, = torch.autograd.grad(kd, z)
    w_ce, w_kd = closed_form_grads(z.detach(), y, zo, c_old, 10.0)
    e1, e2 = float((g_ce - w_ce).abs().max()), float((g_kd - w_kd).abs().max())
    assert e1 < 1e-12 and e2 < 1e-12, (e1, e2)


def test_kd_gradient_is_zero_right_after_background_growth():
    torch.manual_seed(6)
    m = C.UNet(11, 3, 8).double()
    with torch.no_grad():
        m.last[6].bias.normal_()
    feat = torch.randn(2, 8, 8, 8, dtype=torch.float64) * 2
    zo = F.conv2d(feat, m.last[6].weight, m.last[6].bias).detach()
    m.expand_classes(10)
    z = F.conv2d(feat, m.last[6].weight, m.last[6].bias).detach().requires_grad_()
    y = torch.zeros(2, 8, 8, dtype=torch.int64)
    _, _, kd = unbiased_losses(z, y, zo, 11, 10.0)
    g, = torch.autograd.grad(kd, z)
    assert float(g.abs().max()) < 1e-15, float(g.abs().max())


def test_replace_params_host_logic():
    torch.manual_seed(0)
    m = C.UNet(11, 3, 8)
    opt = C.FusedAdam(m.parameters(), lr=1e-3)
    old = [p.detach().clone() for p in m.parameters()]
    opt.set_l2_anchor(old, 0.1)
    ow, ob, nw, nb = m.expand_classes(10, init='default')
    with pytest.raises(ValueError, match='not a parameter'):
        opt.replace_params({torch.nn.Parameter(torch.zeros(3)): nb})
    with pytest.raises(ValueError, match='not growth along dim 0'):
        opt.replace_params({ow: torch.nn.Parameter(torch.zeros(21, 9, 1, 1))})
    with pytest.raises(ValueError, match='not growth along dim 0'):
        opt.replace_params({ob: torch.nn.Parameter(torch.zeros(11))})
    opt.replace_params({ow: nw, ob: nb})
    params = opt.param_groups[0]['params']
    assert len(params) == 82 and all(a is b for a, b in zip(params, m.parameters())) and opt._table is None
    # the L2 anchor: old rows = the snapshot, new rows = the new rows' initial values (no pull on them)
    assert torch.equal(opt._anchor[-2][:11], old[-2]) and torch.equal(opt._anchor[-2][11:], nw.detach()[11:])
    assert torch.equal(opt._anchor[-1][:11], old[-1]) and torch.equal(opt._anchor[-1][11:], nb.detach()[11:])
    assert len(opt.state_dict()['param_groups'][0]['params']) == 82


def test_consolidation_grow_host_logic():
    torch.manual_seed(0)
    m = C.UNet(11, 3, 8)
    cons = C.Consolidation(m.named_parameters())
    cons.flat.copy_(torch.arange(cons.flat.numel(), dtype=torch.float32))
    imp0 = [w.clone() for w in cons.importance]
    anchor0 = [a.clone() for a in cons.anchor]
    cons.finished = True
    before = {k: {n: t.clone() for n, t in v.items()} if isinstance(v, dict) else v for k, v in cons.state_dict().items()}
    ow, ob, nw, nb = m.expand_classes(10, init='default')
    with pytest.raises(KeyError):
        cons.grow('last.7.weight', nw)
    with pytest.raises(ValueError, match='not growth along dim 0'):
        cons.grow('last.6.weight', ow)
    cons.grow('last.6.weight', nw).grow('last.6.bias', nb)
    assert cons.names == [n for n, _ in m.named_parameters()] and cons.shapes == [tuple(p.shape) for p in m.parameters()]
    assert cons.flat.numel() == sum(p.numel() for p in m.parameters())
    off = 0
    for w, w0, a, a0, p in zip(cons.importance, imp0, cons.anchor, anchor0, m.parameters()):
        assert w.data_ptr() == cons.flat.data_ptr() + 4 * off and w.shape == p.shape
        off += w.numel()
        n0 = w0.shape[0]
        assert torch.equal(w[:n0], w0) and float(w[n0:].abs().sum()) == 0.0
        assert torch.equal(a[:n0], a0) and torch.equal(a[n0:], p.detach()[n0:])
    # round trip of the grown state; a pre-growth state is refused with the shape message
    other = C.Consolidation(m.named_parameters()).load_state_dict(cons.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(other.importance, cons.importance))
    with pytest.raises(ValueError, match='has shape'):
        C.Consolidation(m.named_parameters()).load_state_dict(before)


def test_criterion_refuses_cpu_tensors():
    crit = C.UnbiasedDistillationCrossEntropy(3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        crit(torch.zeros(1, 5, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))
    with pytest.raises(ValueError):
        C.UnbiasedDistillationCrossEntropy(0)


def _gloo_growth_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from continual_learning_amd.unet import _Engine
        torch.manual_seed(0)
        tr = C.Trainer([], C.default_config(num_classes=5, conv_dim=4), device='cpu')
        sync = C.ddp.GradSync(tr.model, tr.optim, min_bucket_bytes=16 << 10)

        def exchange():
            """One backward's worth of stage buckets over a fresh engine of the model's current width -> (sum ok, buckets tile the buffer)."""
            eng = _Engine(tr.model, 2, 32, 32, torch.device('cpu'))
            n = eng.gflat.numel()
            eng.gflat.copy_(torch.arange(n, dtype=torch.float32) * (rank + 1))
            launches, orig = [], sync._launch
            sync._launch = lambda flat: (launches.append((flat.data_ptr(), flat.numel())), orig(flat))[1]
            for st in reversed(eng.stages):
                sync.stage_done(eng, st)
            sync.wait()
            sync._launch = orig
            base = eng.gflat.data_ptr()
            spans = sorted(((p - base) // 4, (p - base) // 4 + k) for p, k in launches)
            tiled = spans[0][0] == 0 and spans[-1][1] == n and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            return torch.equal(eng.gflat, torch.arange(n, dtype=torch.float32) * sum(r + 1 for r in range(world))), tiled, n

        before = exchange()
        torch.manual_seed(100 + rank)                    # 'default' draws the new rows from each rank's own RNG ...
        tr.grow_head(3, init='default')
        w = tr.model.last[6].weight.detach().clone()
        gathered = [torch.zeros_like(w) for _ in range(world)]
        dist.all_gather(gathered, w)                     # ... and grow_head broadcasts rank 0's
        after = exchange()
        params = tr.optim.param_groups[0]['params']
        q.put((rank, before, after, all(torch.equal(gathered[0], t) for t in gathered), sync._lo is None and not sync._pending,
               all(a is b for a, b in zip(params, tr.model.parameters())), tr.cfg.num_classes, sum(p.numel() for p in params)))
    finally:
        dist.destroy_process_group()


def test_gradsync_through_head_growth_gloo_world2():
    """ddp.GradSync keeps no parameter list or sizes of its own: after head growth the rebuilt engine's flat gradient buffer is tiled by the
    stage buckets exactly once and summed over the ranks as before; grow_head broadcasts the new rows, so ranks with different RNG
    states keep identical heads with init='default'."""
    world = 2
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    ps = [ctx.Process(target=_gloo_growth_worker, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = [q.get(timeout=180) for _ in range(world)]
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    for rank, before, after, same_head, idle, params_ok, nc, numel in res:
        assert before[0] and before[1] and after[0] and after[1], (rank, before, after)
        assert after[2] == before[2] + 3 * 4 + 3 == numel, (before[2], after[2], numel)
        assert same_head, 'grow_head did not equalise the new rows across the ranks'
        assert idle and params_ok and nc == 8
