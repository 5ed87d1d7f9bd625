"""Synchronised BatchNorm (nn.SyncBatchNorm.convert_sync_batchnorm) on the GPU.

* the three kernels: fp64 totals of the partial rows, and finalize from all-reduced totals -- bit-identical to clamd_bn_finalize /
  clamd_bn_bwd_finalize when the global totals are the local ones, torch.nn.SyncBatchNorm's formulas when they are not;
* world size 1 (gloo and RCCL): the converted model takes the synchronised path (every train-mode layer all-reduces) and is bit-identical
  to the unconverted model;
* world size 2 (two gloo ranks on the one card, as tests/test_ddp_gpu.py): one image per rank with GradSync reproduces the plain model
  on both images in one process -- logits, running statistics, weights -- where the unconverted model does not; uneven shards, layers
  in eval mode, a stand-alone block and a conversion after the first forward.
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

pytestmark = pytest.mark.gpu

CFG = dict(num_classes=5, conv_dim=8, size=64, steps=3)
FROZEN = ('enc2.block.3', 'dec1.block.5', 'last.2')       # the mixed-mode run: these layers in eval mode


def _C():
    import continual_learning_amd as C
    return C


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# ------------------------------------------------------------------------------------------------ kernels
def _rows(nrows, nk, Cp, seed, two=False):
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(nrows, nk, Cp, generator=g, dtype=torch.float32) * 3 + 0.5
    r[:, 1] = r[:, 1].abs() * 20 + 40            # forward: sum x^2 large enough for a positive variance; backward: any value
    if two:
        r[:, 2:] = float('nan')                  # the two-sum form (include/clamd.h, clamd_bn_bwd_apply_sums)
    return r.cuda()


def _vec(n, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, generator=g) * (hi - lo) + lo).cuda()


def _totals(rows, count):
    """(reduce [2Cp+1], totals [nk][Cp]) from clamd_bn_rows_total."""
    C = _C()
    nrows, nk, Cp = rows.shape
    red = torch.full((2 * Cp + 1,), float('nan'), dtype=torch.float64, device='cuda')
    tot = torch.full((nk, Cp), float('nan'), dtype=torch.float64, device='cuda')
    C._lib.call('clamd_bn_rows_total', rows.data_ptr(), nrows, nk, Cp, float(count), tot.data_ptr(), red.data_ptr(), None)
    return red, tot


@pytest.mark.parametrize('nk,two', [(2, False), (5, False), (5, True)])
def test_rows_total_matches_fp64_sum(nk, two):
    C = _C()
    rows = _rows(37, nk, 64, 1 + nk, two)
    red, tot = _totals(rows, 1234.0)
    torch.cuda.synchronize()
    r = rows.double().cpu().numpy()
    ref, scale = r.sum(0), np.abs(r).sum(0)
    got = tot.cpu().numpy()
    ok = ~np.isnan(ref)
    assert np.all(np.abs(got[ok] - ref[ok]) <= 1e-12 * scale[ok])
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(red[:128].cpu().numpy(), got[:2].reshape(-1), equal_nan=True)      # the k = 0, 1 copy ...
    assert float(red[128]) == 1234.0                                                          # ... and the count slot
    # only one of the two outputs
    red2 = torch.zeros(129, dtype=torch.float64, device='cuda')
    C._lib.call('clamd_bn_rows_total', rows.data_ptr(), 37, nk, 64, 1234.0, None, red2.data_ptr(), None)
    assert torch.equal(red2[:128], red[:128]) and float(red2[128]) == 1234.0


def _fwd_outputs(Cp, C_):
    rm, rv = _vec(C_, 11), _vec(C_, 12, 0.5, 2.0)
    return dict(scale=torch.zeros(Cp, device='cuda'), shift=torch.zeros(Cp, device='cuda'), mean=torch.zeros(Cp, device='cuda'),
                istd=torch.zeros(Cp, device='cuda'), rm=rm, rv=rv, nbt=torch.zeros((), dtype=torch.int64, device='cuda'))


def _finalize_total(red, gamma, beta, o, Cp, C_):
    _C()._lib.call('clamd_bn_finalize_total', red.data_ptr(), gamma.data_ptr(), beta.data_ptr(), o['rm'].data_ptr(), o['rv'].data_ptr(),
                   o['scale'].data_ptr(), o['shift'].data_ptr(), o['mean'].data_ptr(), o['istd'].data_ptr(), Cp, C_, 0.1, 1e-5,
                   o['nbt'].data_ptr(), None)


def test_finalize_total_forward():
    C = _C()
    Cp, C_, n = 64, 50, 37
    rows, other = _rows(n, 2, Cp, 3), _rows(23, 2, Cp, 4)
    gamma, beta = _vec(C_, 5), _vec(C_, 6)
    count, count_o = 1000.0, 600.0
    ref = _fwd_outputs(Cp, C_)
    C._lib.call('clamd_bn_finalize', rows.data_ptr(), n, gamma.data_ptr(), beta.data_ptr(), ref['rm'].data_ptr(), ref['rv'].data_ptr(),
                ref['scale'].data_ptr(), ref['shift'].data_ptr(), ref['mean'].data_ptr(), ref['istd'].data_ptr(), Cp, C_, count, 0.1, 1e-5,
                ref['nbt'].data_ptr(), None)
    red, _ = _totals(rows, count)
    got = _fwd_outputs(Cp, C_)
    _finalize_total(red, gamma, beta, got, Cp, C_)
    torch.cuda.synchronize()
    for k in ref:
        assert torch.equal(got[k], ref[k]), f'{k}: finalize of the local totals is not bit-identical to clamd_bn_finalize'
    assert int(got['nbt']) == 1
    # global != local: the totals of another rank added (and its count): torch.nn.SyncBatchNorm's statistics of the union
    red_o, _ = _totals(other, count_o)
    glob = red + red_o
    got = _fwd_outputs(Cp, C_)
    rm0, rv0 = got['rm'].double().cpu().numpy(), got['rv'].double().cpu().numpy()
    _finalize_total(glob, gamma, beta, got, Cp, C_)
    torch.cuda.synchronize()
    s0 = rows[:, 0].double().sum(0).cpu().numpy() + other[:, 0].double().sum(0).cpu().numpy()
    s1 = rows[:, 1].double().sum(0).cpu().numpy() + other[:, 1].double().sum(0).cpu().numpy()
    N = count + count_o
    mean = s0 / N
    var = np.maximum(s1 / N - mean * mean, 0)
    istd = 1 / np.sqrt(var + 1e-5)
    g = np.zeros(Cp); g[:C_] = gamma.double().cpu().numpy()
    b = np.zeros(Cp); b[:C_] = beta.double().cpu().numpy()
    tol = dict(rtol=2e-6, atol=1e-6)
    np.testing.assert_allclose(got['scale'].cpu().numpy(), g * istd, **tol)
    np.testing.assert_allclose(got['shift'].cpu().numpy(), b - mean * g * istd, **tol)
    np.testing.assert_allclose(got['mean'].cpu().numpy(), mean, **tol)
    np.testing.assert_allclose(got['istd'].cpu().numpy(), istd, **tol)
    np.testing.assert_allclose(got['rm'].cpu().numpy(), 0.9 * rm0 + 0.1 * mean[:C_], **tol)
    np.testing.assert_allclose(got['rv'].cpu().numpy(), 0.9 * rv0 + 0.1 * var[:C_] * N / (N - 1), **tol)     # unbiased, global count
    assert int(got['nbt']) == 1


def _bwd_outputs(Cp, C_):
    return dict(k012=torch.zeros(3, Cp, device='cuda'), dgamma=torch.zeros(C_, device='cuda'), dbeta=torch.zeros(C_, device='cuda'),
                dbias=torch.zeros(C_, device='cuda'))


@pytest.mark.parametrize('two', [False, True])
def test_bwd_finalize_total(two):
    C = _C()
    NS = C._lib.load().clamd_bn_bwd_nsums()
    Cp, C_, n = 64, 56, 29
    rows, other = _rows(n, NS, Cp, 7, two), _rows(31, NS, Cp, 8, two)
    gamma, mu, istd = _vec(C_, 9), _vec(Cp, 10), _vec(Cp, 11, 0.5, 3.0)
    count, count_o = 900.0, 700.0
    P = lambda t: t.data_ptr()          # noqa: E731
    ref = _bwd_outputs(Cp, C_)
    C._lib.call('clamd_bn_bwd_finalize', P(rows), n, P(gamma), P(mu), P(istd), P(ref['k012']), P(ref['dgamma']), P(ref['dbeta']),
                None if two else P(ref['dbias']), Cp, C_, count, None)
    red, tot = _totals(rows, count)

    def total(glob):
        o = _bwd_outputs(Cp, C_)
        C._lib.call('clamd_bn_bwd_finalize_total', P(tot), P(glob), P(gamma), P(mu), P(istd), P(o['k012']), P(o['dgamma']), P(o['dbeta']),
                    None if two else P(o['dbias']), Cp, C_, None)
        torch.cuda.synchronize()
        return o
    got = total(red)
    for k in ref:
        assert torch.equal(got[k], ref[k]), f'{k}: finalize of the local totals is not bit-identical to clamd_bn_bwd_finalize'
    # global != local: k0, k1, k2 from the union's sums and count, the parameter gradients from this rank's sums alone
    red_o, _ = _totals(other, count_o)
    got = total(red + red_o)
    r, o = rows.double().sum(0).cpu().numpy(), other.double().sum(0).cpu().numpy()
    G0, G1, N = r[0] + o[0], r[1] + o[1], count + count_o
    m, s = mu.double().cpu().numpy(), istd.double().cpu().numpy()
    g = np.zeros(Cp); g[:C_] = gamma.double().cpu().numpy()
    # torch: grad_in = (dy - sum_dy / N - (x - mean) * invstd^2 * sum_dy_xmu / N) * invstd * weight, sum_dy_xmu = sum dy (x - mean)
    sum_dy_xmu = G1 - m * G0
    k0 = g * s
    k1 = -k0 * s * s * sum_dy_xmu / N
    k2 = k0 * (m * s * s * sum_dy_xmu / N - G0 / N)
    tol = dict(rtol=2e-6, atol=1e-6)
    np.testing.assert_allclose(got['k012'].cpu().numpy(), np.stack([k0, k1, k2]), **tol)
    np.testing.assert_allclose(got['dgamma'].cpu().numpy(), (s * (r[1] - m * r[0]))[:C_], **tol)       # local sums
    np.testing.assert_allclose(got['dbeta'].cpu().numpy(), r[0][:C_], **tol)
    if not two:       # d conv-bias = sum of this rank's g_z = k0 sum g[y>0] + k1 sum y + k2 sum [y>0]
        np.testing.assert_allclose(got['dbias'].cpu().numpy(), (k0 * r[2] + k1 * r[4] + k2 * r[3])[:C_], **tol)
    else:
        assert not got['dbias'].any()


# ------------------------------------------------------------------------------------------------ training runs
def _data(first, n):
    C = _C()
    s, K = CFG['size'], CFG['num_classes']
    x = torch.from_numpy(C.synth.images(99, n, 3, s, s, first_image=first)).cuda()
    y = torch.from_numpy(C.synth.labels(99, n, s, s, K, first_image=first)).cuda()
    return x, y


def _bn_state(model):
    out = {}
    for n, m in model.named_modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            out[n] = (m.running_mean.detach().cpu().clone(), m.running_var.detach().cpu().clone(), int(m.num_batches_tracked))
    return out


# Two runs that differ by rounding only: Adam's first steps are nearly lr * sign(g), and the gradient of a convolution bias in front of a
# train-mode BatchNorm is zero up to rounding (the ReLU between them keeps it from being exactly zero), so at eps = 1e-8 such elements move by
# +-lr at random and the runs part by ~1e-3 within three steps, whatever the BatchNorm does.  The comparisons against the full batch use the
# reference's learning rate (1e-4) and eps = 1e-6: rounding-level gradients then move nothing, every real gradient still moves by ~lr.
FULL_BATCH_OPT = dict(lr=1e-4, eps=1e-6)


def _train(first, n, dtype='fp32', convert=False, ddp=False, frozen=(), steps=CFG['steps'], opt_kw=None):
    """`steps` train steps (trainer.py:172-176 order) on images first..first+n-1: losses, logits per step, first-step gradients, final
    weights, BatchNorm buffers."""
    C = _C()
    torch.manual_seed(7)
    model = C.UNet(CFG['num_classes'], 3, CFG['conv_dim'], compute_dtype=dtype).cuda().train()
    if convert:
        nn.SyncBatchNorm.convert_sync_batchnorm(model)
    for name in frozen:
        model.get_submodule(name).eval()
    opt = C.FusedAdam(model.parameters(), betas=[0.5, 0.99], **(opt_kw or dict(lr=1e-3)))
    crit = C.CrossEntropyLoss()
    if ddp:
        C.ddp.broadcast_parameters(model)
        C.ddp.GradSync(model, opt, min_bucket_bytes=16 << 10, grad_dtype='fp32')
    x, y = _data(first, n)
    losses, logits, grad0 = [], [], None
    for i in range(steps):
        out = model(x)
        opt.zero_grad()
        loss = crit(out, y)
        loss.backward()
        if i == 0:
            if ddp:
                model.grad_sync.wait()
            grad0 = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu()
        opt.step()
        losses.append(float(loss.detach()))
        logits.append(out.detach().cpu())
    torch.cuda.synchronize()
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu()
    return dict(losses=losses, logits=logits, grad0=grad0, flat=flat, bn=_bn_state(model))


class _CountBN:
    """Wraps torch.distributed.all_reduce: records the BatchNorm sums (fp64 buffers; the gradient buckets are fp32)."""

    def __init__(self):
        self.sizes, self._orig = [], dist.all_reduce

    def __enter__(self):
        def wrapped(t, *a, **kw):
            if t.dtype == torch.float64:
                self.sizes.append(t.numel())
            return self._orig(t, *a, **kw)
        dist.all_reduce = wrapped
        return self

    def __exit__(self, *exc):
        dist.all_reduce = self._orig


def _bn_sizes(model_or_none, frozen=()):
    """2 Cp + 1 per train-mode BatchNorm in forward order (the forward's collectives)."""
    C = _C()
    m = model_or_none or C.UNet(CFG['num_classes'], 3, CFG['conv_dim'])
    return [2 * C.cpad(mod.num_features) + 1 for n, mod in m.named_modules()
            if isinstance(mod, nn.modules.batchnorm._BatchNorm) and n not in frozen]


def _assert_same(a, b, what):
    assert a['losses'] == b['losses'], f'{what}: losses {a["losses"]} vs {b["losses"]}'
    assert torch.equal(a['grad0'], b['grad0']), f'{what}: first-step gradients differ (rel {_rel(a["grad0"], b["grad0"]):.2e})'
    assert torch.equal(a['flat'], b['flat']), f'{what}: weights after {CFG["steps"]} steps differ'
    for k in b['bn']:
        rm, rv, nb = a['bn'][k]
        assert torch.equal(rm, b['bn'][k][0]) and torch.equal(rv, b['bn'][k][1]) and nb == b['bn'][k][2], f'{what}: {k} running statistics'


@pytest.mark.parametrize('backend', ['gloo', 'nccl'])
@pytest.mark.parametrize('dtype', ['fp32', 'bf16', 'bf16x3'])
def test_world1_converted_model_is_bit_identical(backend, dtype):
    ref = _train(0, 2, dtype)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_free_port()), RANK='0', WORLD_SIZE='1')
    kw = dict(device_id=torch.device('cuda', 0)) if backend == 'nccl' else {}
    dist.init_process_group(backend, rank=0, world_size=1, **kw)
    try:
        with _CountBN() as cnt:
            got = _train(0, 2, dtype, convert=True)
    finally:
        dist.destroy_process_group()
    fwd = _bn_sizes(None)
    assert len(cnt.sizes) == CFG['steps'] * 2 * 18, 'the converted model did not take the synchronised path'
    assert cnt.sizes[:18] == fwd and sorted(cnt.sizes[18:36]) == sorted(fwd)
    _assert_same(got, ref, f'{backend} world 1 {dtype}')
    assert all(v[2] == CFG['steps'] for v in got['bn'].values())


def test_capture_of_a_synchronised_step_raises(tmp_path, monkeypatch):
    C = _C()
    dist.init_process_group('gloo', init_method=f'file://{tmp_path}/pg', rank=0, world_size=1)
    try:
        model = nn.SyncBatchNorm.convert_sync_batchnorm(C.UNet(CFG['num_classes'], 3, CFG['conv_dim']).cuda().train())
        x, _ = _data(0, 2)
        model(x)
        monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)      # what a capture would report; no capture is made
        with pytest.raises(RuntimeError, match='SyncBatchNorm'):
            model(x)
        model.eval()
        monkeypatch.undo()
        model(x)                        # eval mode: no collective, nothing to refuse
    finally:
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------ two ranks
def _host(obj):
    if torch.is_tensor(obj):
        return obj.detach().cpu().numpy()
    if isinstance(obj, dict):
        return {k: _host(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_host(v) for v in obj)
    return obj


def _worker(rank, world, port, job, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        with _CountBN() as cnt:
            res = _JOBS[job['kind']](rank, job)
        res['bn_sizes'] = cnt.sizes
        q.put((rank, _host(res)))      # numpy: torch tensors would travel as file descriptors of this process, which ends next
    except BaseException as e:          # report, so the parent fails with the reason instead of a queue timeout
        q.put((rank, {'error': repr(e)}))
        raise
    finally:
        dist.destroy_process_group()


def _job_train(rank, job):
    first, n = job['shards'][rank]
    return _train(first, n, convert=job['convert'], ddp=True, frozen=job.get('frozen', ()), opt_kw=FULL_BATCH_OPT)


def _job_forward(rank, job):
    """One train-mode forward on an uneven shard."""
    C = _C()
    first, n = job['shards'][rank]
    torch.manual_seed(7)
    model = nn.SyncBatchNorm.convert_sync_batchnorm(C.UNet(CFG['num_classes'], 3, CFG['conv_dim']).cuda().train())
    x, _ = _data(first, n)
    out = model(x).detach().cpu()
    torch.cuda.synchronize()
    return dict(logits=out, bn=_bn_state(model))


def _job_late(rank, job):
    """Forward, convert, forward: the second forward uses the global statistics."""
    C = _C()
    first, n = job['shards'][rank]
    torch.manual_seed(7)
    model = C.UNet(CFG['num_classes'], 3, CFG['conv_dim']).cuda().train()
    x, _ = _data(first, n)
    before = model(x).detach().cpu()
    nn.SyncBatchNorm.convert_sync_batchnorm(model)
    after = model(x).detach().cpu()
    torch.cuda.synchronize()
    return dict(before=before, after=after, bn=_bn_state(model))


def _block_input(first, n):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, CFG['conv_dim'], 32, 32, generator=g)[first:first + n]
    w = torch.randn(3, 2 * CFG['conv_dim'], 16, 16, generator=g)[first:first + n]
    return x.cuda().requires_grad_(True), w.cuda()


def _block_run(model, first, n):
    x, w = _block_input(first, n)
    out = model.enc2(x)
    (out * w).sum().backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone() for k, p in model.enc2.named_parameters()}
    return out.detach().cpu(), x.grad.detach().cpu(), grads, _bn_state(model.enc2)


def _job_block(rank, job):
    """model.enc2(x) on one image per rank; the parameter gradients summed over the ranks."""
    C = _C()
    first, n = job['shards'][rank]
    torch.manual_seed(7)
    model = nn.SyncBatchNorm.convert_sync_batchnorm(C.UNet(CFG['num_classes'], 3, CFG['conv_dim']).cuda().train())
    out, gx, grads, bn = _block_run(model, first, n)
    for g in grads.values():
        dist.all_reduce(g)
    return dict(out=out, gx=gx, grads={k: g.cpu() for k, g in grads.items()}, bn=bn)


_JOBS = dict(train=_job_train, forward=_job_forward, late=_job_late, block=_job_block)


def _run_world2(job):
    world, port = 2, _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, world, port, job, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = sorted((q.get(timeout=300) for _ in range(world)), key=lambda r: r[0])
    for p in ps:
        p.join(60)
    for rank, r in res:
        assert 'error' not in r, f'rank {rank}: {r["error"]}'
    assert all(p.exitcode == 0 for p in ps)
    return [r for _, r in res]


def _stats_err(a, b):
    """Largest rel-L2 error of running mean / var over the layers, and whether num_batches_tracked agree."""
    e = max(max(_rel(a[k][0], b[k][0]), _rel(a[k][1], b[k][1])) for k in b)
    return e, all(a[k][2] == b[k][2] for k in b)


# Measured on the MI355X (fp32, conv_dim 8, 64 x 64, 2 ranks x 1 image against 2 images in one process, three steps): logits 0 at the
# first step and up to 2.7e-6 rel-L2 after it, first-step gradient 4.6e-7, running statistics 9.6e-7, weights 3.8e-6 (mixed modes; 1e-7 all
# train).  The bounds are about twice that (the issue's caps: logits 1e-4, running statistics 1e-5).  The forward-only runs (uneven shards,
# stand-alone block, late conversion) matched bit for bit; their bounds are the same.
TOL_LOGITS, TOL_STATS, TOL_W, TOL_GRAD = 6e-6, 2e-6, 8e-6, 1e-6


def _check_vs_full(got, full, n_each, frozen=()):
    for rank, r in enumerate(got):
        es_ = [_rel(lr, lf[rank * n_each:(rank + 1) * n_each]) for lr, lf in zip(r['logits'], full['logits'])]
        e = max(es_)
        es, same_nbt = _stats_err(r['bn'], full['bn'])
        ew = _rel(r['flat'], full['flat'])
        eg = _rel(r['grad0'] / 2, full['grad0'])          # GradSync's sum over the two ranks; the 1/world factor lives in Adam
        print(f'rank {rank}: logits rel {" ".join(f"{v:.2e}" for v in es_)}, first-step gradient rel {eg:.2e}, running stats rel {es:.2e}, '
              f'weights rel {ew:.2e}')
        assert e <= TOL_LOGITS, f'rank {rank}: logits miss the full batch by {e:.2e}'
        assert eg <= TOL_GRAD, f'rank {rank}: first-step gradient misses the full batch by {eg:.2e}'
        assert es <= TOL_STATS and same_nbt, f'rank {rank}: running statistics miss the full batch by {es:.2e}'
        assert ew <= TOL_W, f'rank {rank}: weights miss the full batch by {ew:.2e}'
    a, b = got
    assert np.array_equal(a['flat'], b['flat']), 'replicas diverged'
    for k in a['bn']:
        assert np.array_equal(a['bn'][k][0], b['bn'][k][0]) and np.array_equal(a['bn'][k][1], b['bn'][k][1]), f'{k}: ranks disagree'
    fwd = _bn_sizes(None, frozen)
    assert a['bn_sizes'][:len(fwd)] == fwd
    assert len(a['bn_sizes']) == CFG['steps'] * 2 * len(fwd), 'frozen layers must take part in no collective'


def test_world2_matches_the_full_batch():
    full = _train(0, 2, opt_kw=FULL_BATCH_OPT)
    got = _run_world2(dict(kind='train', shards=[(0, 1), (1, 1)], convert=True))
    _check_vs_full(got, full, 1)
    # control: without the conversion every rank normalises with its own image's statistics
    plain = _run_world2(dict(kind='train', shards=[(0, 1), (1, 1)], convert=False))
    for rank, r in enumerate(plain):
        e = _rel(r['logits'][0], full['logits'][0][rank:rank + 1])
        print(f'unconverted rank {rank}: logits rel {e:.2e}')
        assert e > 1e-2
        assert r['bn_sizes'] == []


def test_world2_mixed_modes_match_the_equally_frozen_full_batch():
    full = _train(0, 2, frozen=FROZEN, opt_kw=FULL_BATCH_OPT)
    got = _run_world2(dict(kind='train', shards=[(0, 1), (1, 1)], convert=True, frozen=FROZEN))
    _check_vs_full(got, full, 1, frozen=FROZEN)
    for k in FROZEN:
        assert got[0]['bn'][k][2] == 0


def test_world2_uneven_shards():
    C = _C()
    torch.manual_seed(7)
    model = C.UNet(CFG['num_classes'], 3, CFG['conv_dim']).cuda().train()
    x, _ = _data(0, 3)
    full = model(x).detach().cpu()
    full_bn = _bn_state(model)
    got = _run_world2(dict(kind='forward', shards=[(0, 2), (2, 1)]))
    for rank, (r, sl) in enumerate(zip(got, [slice(0, 2), slice(2, 3)])):
        e = _rel(r['logits'], full[sl])
        es, same_nbt = _stats_err(r['bn'], full_bn)
        print(f'uneven rank {rank}: logits rel {e:.2e}, running stats rel {es:.2e}')
        assert e <= TOL_LOGITS and es <= TOL_STATS and same_nbt


def test_world2_standalone_block():
    C = _C()
    torch.manual_seed(7)
    model = C.UNet(CFG['num_classes'], 3, CFG['conv_dim']).cuda().train()
    out, gx, grads, bn = _block_run(model, 0, 2)
    got = _run_world2(dict(kind='block', shards=[(0, 1), (1, 1)]))
    for rank, r in enumerate(got):
        e, eg = _rel(r['out'], out[rank:rank + 1]), _rel(r['gx'], gx[rank:rank + 1])
        ep = max(_rel(r['grads'][k], grads[k].cpu()) for k in grads)
        es, same_nbt = _stats_err(r['bn'], bn)
        print(f'block rank {rank}: out rel {e:.2e}, input grad rel {eg:.2e}, parameter grads rel {ep:.2e}, running stats rel {es:.2e}')
        assert e <= TOL_LOGITS and es <= TOL_STATS and same_nbt
        assert eg <= TOL_GRAD and ep <= 2e-7          # measured: 0 and 7.8e-8 (the sum over the ranks against the full batch's sum)
    assert got[0]['bn_sizes'] == [2 * C.cpad(2 * CFG['conv_dim']) + 1] * 4          # two layers, forward and backward


def test_world2_conversion_after_the_first_forward():
    C = _C()
    torch.manual_seed(7)
    model = C.UNet(CFG['num_classes'], 3, CFG['conv_dim']).cuda().train()
    x, _ = _data(0, 2)
    full = model(x).detach().cpu()
    got = _run_world2(dict(kind='late', shards=[(0, 1), (1, 1)]))
    for rank, r in enumerate(got):
        e0, e1 = _rel(r['before'], full[rank:rank + 1]), _rel(r['after'], full[rank:rank + 1])
        print(f'late rank {rank}: before conversion rel {e0:.2e}, after {e1:.2e}')
        assert e0 > 1e-2 and e1 <= TOL_LOGITS
        assert r['bn_sizes'] == _bn_sizes(None)
        assert all(v[2] == 2 for v in r['bn'].values())
