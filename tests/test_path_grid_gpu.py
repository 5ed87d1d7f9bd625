"""GPU: the tracked instantiations of the fused Adam and SGD kernels and the boundary pass of Synaptic Intelligence (csrc/optim.hip) per
tensor and per element across the grid of test_adam_grid_gpu.py -- sizes below, at and above one chunk in one launch, every buffer (the
path integral included) at its own element phase inside a poisoned buffer with guard bands, the anchor terms none / l2 / ewc / both, two
gradient scales, zero and given starting state; for SGD also the momentum variants and weight decay with one undecayed row.

Step kernels: p, m, v / buf and the two penalty sums against the float64 restatement (tests/path_ref.py) at the bounds of the existing
grid tests; omega per element against its definition evaluated in float64 on the kernel's OWN fp32 input and output parameters; the buffers
that are only read bit-unchanged; two launches from the same state bit-identical; and, where the compiler cannot contract differently
(grad_scale 1, no anchor, no weight decay), p, m, v / buf bit-identical to the untracked entry point."""
import numpy as np
import pytest
import torch

import path_ref
from conftest import rel_l2
from grid_util import Banded, DEV, POISON
from test_adam_grid_gpu import ADAM_ROW, BETA1, BETA2, EPS, L2, LAM, LR, PHASES, SIZES, _inputs as adam_inputs, f32
from test_ewc_gpu import _check_importance
from test_sgd_gpu import NO_DECAY

pytestmark = pytest.mark.gpu

PATH_PHASES = (3, 2, 1, 0, 1, 2)               # the path integral at every 4-byte phase of a 16-byte line
SGD_PHASES = {'p': (0, 0, 0, 1, 0, 0), 'g': (0, 1, 2, 3, 1, 2), 'buf': (0, 3, 0, 0, 2, 1), 'old': (1, 2, 0, 3, 0, 3),
              'omega': (2, 0, 1, 0, 0, 3)}     # those of test_sgd_gpu.py
PATH_ROW = np.dtype([('importance', 'u8'), ('path', 'u8'), ('p', 'u8'), ('start', 'u8'), ('n', 'i8')])
assert set(PATH_PHASES) == {0, 1, 2, 3}


@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    C._lib.load()
    return C


_PATH0 = {}


def _path0(given):
    """The starting path integral: zero, or (given) normal values of the size of one step's term, 5 % exact zeros.  Generated once."""
    if not _PATH0:
        rng = np.random.default_rng(31)
        vals = []
        for n in SIZES:
            a = (rng.standard_normal(n) * 0.01).astype(np.float32)
            a[rng.random(n) < 0.05] = 0.0
            vals.append(torch.from_numpy(a))
        _PATH0[True] = vals
        _PATH0[False] = [torch.zeros(n) for n in SIZES]
    return _PATH0[given]


def _jobs(C, rows, dtype):
    chunk = C._lib.load().clamd_adam_chunk_elems()
    t = np.zeros(len(SIZES), dtype=dtype)
    chunks = []
    for i, n in enumerate(SIZES):
        t[i] = rows[i]
        chunks += [(i, c) for c in range((n + chunk - 1) // chunk)]
    assert len(chunks) == 8                    # 8195 elements: three chunks
    return torch.from_numpy(t.view(np.uint8).copy()).to(DEV), torch.tensor(chunks, dtype=torch.int32, device=DEV), len(chunks)


def _ptrs(views):
    return torch.tensor([w.data_ptr() for w in views], dtype=torch.int64).to(DEV)


def _unchanged(b):
    return torch.equal(b.flat.view(torch.int32), b.before.view(torch.int32))


def _check_omega(what, A, i, omega0, g, gs, p0, p1):
    """omega of tensor i per element (path_ref.omega_from_kernel_values); elements with a zero gradient keep omega's bits."""
    got = A.views[i].cpu()
    want, bound = path_ref.omega_from_kernel_values(omega0.numpy(), g.numpy(), gs, p0.numpy(), p1.numpy())
    err = np.abs(got.numpy().astype(np.float64) - want)
    worst = float((err / bound).max())
    print(f'{what} omega[{i}] n={SIZES[i]}: worst error / bound {worst:.3f}')
    assert worst <= 1.0, (what, i, int((err / bound).argmax()), worst)
    zero = g == 0
    assert zero.any() or SIZES[i] < 1000
    assert torch.equal(got[zero].view(torch.int32), omega0[zero].view(torch.int32)), f'{what}: omega[{i}] moved under a zero gradient'


# ------------------------------------------------------------------------------------------------------------------------------ Adam
class AdamState:
    def __init__(self, given):
        inp = adam_inputs()
        zeros = [torch.zeros(n) for n in SIZES]
        self.step0 = 3 if given else 0
        self.P = Banded(SIZES, PHASES['p'], inp['p'])
        self.G = Banded(SIZES, PHASES['g'], inp['g'])
        self.M = Banded(SIZES, PHASES['m'], inp['m'] if given else zeros)
        self.V = Banded(SIZES, PHASES['v'], inp['v'] if given else zeros)
        self.OLD = Banded(SIZES, PHASES['old'], inp['old'])
        self.OM = Banded(SIZES, PHASES['omega'], inp['omega'])
        self.A = Banded(SIZES, PATH_PHASES, _path0(given))
        self.step = torch.full((1,), self.step0, dtype=torch.int32, device=DEV)
        self.written = (self.P, self.M, self.V, self.A)

    def restore(self):
        for b in self.written:
            b.restore()
        self.step.fill_(self.step0)

    def bits(self):
        return [b.flat.view(torch.int32).clone() for b in self.written]


def _adam_launch(C, S, tracked, anchored, consolidated, l2_on, gs, l2_lam, ewc_lam):
    rows = [(S.P.views[i].data_ptr(), S.G.views[i].data_ptr(), S.M.views[i].data_ptr(), S.V.views[i].data_ptr(),
             S.OLD.views[i].data_ptr() if anchored else 0, n) for i, n in enumerate(SIZES)]
    assert C._lib.load().clamd_sizeof_adam_tensor() == ADAM_ROW.itemsize
    tensors, chunks, nch = _jobs(C, rows, ADAM_ROW)
    hyper = torch.tensor([LR, BETA1, BETA2, EPS, gs, l2_lam, ewc_lam, 0.0], dtype=torch.float32, device=DEV)
    derived = torch.zeros(2, dtype=torch.float32, device=DEV)
    l2 = torch.full((1 + nch,), POISON, device=DEV) if l2_on else None
    ewc = torch.full((1 + nch,), POISON, device=DEV) if consolidated else None
    imp = _ptrs(S.OM.views) if consolidated else None
    ptr, call = C._lib.ptr, C._lib.call
    if tracked:
        path = _ptrs(S.A.views)
        call('clamd_adam_step_tracked', ptr(tensors), ptr(imp), ptr(path), ptr(chunks), nch, ptr(hyper), ptr(S.step), ptr(derived), ptr(ewc),
             ptr(l2), C._lib.stream_ptr())
    elif consolidated:
        call('clamd_adam_step_consolidated', ptr(tensors), ptr(imp), ptr(chunks), nch, ptr(hyper), ptr(S.step), ptr(derived), ptr(ewc), ptr(l2),
             C._lib.stream_ptr())
    else:
        call('clamd_adam_step', ptr(tensors), ptr(chunks), nch, ptr(hyper), ptr(S.step), ptr(derived), ptr(l2), C._lib.stream_ptr())
    torch.cuda.synchronize()
    return ewc, l2


@pytest.mark.parametrize('given', [False, True], ids=['zero_state', 'given_state'])
@pytest.mark.parametrize('gs', [1.0, 0.375])
@pytest.mark.parametrize('terms', ['none', 'l2', 'ewc', 'both'])
def test_tracked_adam_step(C, terms, gs, given):
    """clamd_adam_step_tracked, without and with an importance table.  rel_l2 < 1e-6 per tensor for p, m, v and 2e-6 on the sums, as
    test_adam_step_per_tensor; omega per element."""
    inp = adam_inputs()
    l2_lam = L2 if terms in ('l2', 'both') else 0.0
    ewc_lam = LAM if terms in ('ewc', 'both') else 0.0
    anchored, consolidated = terms != 'none', terms in ('ewc', 'both')
    S = AdamState(given)
    ewc, l2 = _adam_launch(C, S, True, anchored, consolidated, l2_lam > 0, gs, l2_lam, ewc_lam)
    got = S.bits()
    for name, b in (('p', S.P), ('m', S.M), ('v', S.V), ('path', S.A)):
        assert b.guards_intact(), f'{name}: a store outside [0, n) of a tensor'
    for name, b in (('g', S.G), ('old', S.OLD), ('importance', S.OM)):
        assert _unchanged(b), f'{name} was written'
    assert int(S.step) == S.step0 + 1
    what = f'adam {terms} gs={gs} step0={S.step0}'
    zeros = [np.zeros(n) for n in SIZES]
    l2_ref = ewc_ref = 0.0
    for i, n in enumerate(SIZES):
        ref = path_ref.adam_step_tracked(inp['p'][i].numpy(), inp['g'][i].numpy(), inp['m'][i].numpy() if given else zeros[i],
                                         inp['v'][i].numpy() if given else zeros[i], _path0(given)[i].numpy(), S.step0 + 1,
                                         inp['old'][i].numpy() if anchored else None, inp['omega'][i].numpy() if consolidated else None,
                                         lr=f32(LR), beta1=f32(BETA1), beta2=f32(BETA2), eps=f32(EPS), grad_scale=f32(gs),
                                         l2_lambda=f32(l2_lam), ewc_lambda=f32(ewc_lam))
        l2_ref += ref['l2']
        ewc_ref += ref['ewc']
        for name, b in (('p', S.P), ('m', S.M), ('v', S.V)):
            err = rel_l2(b.views[i].cpu().numpy(), ref[name])
            print(f'{what} {name}[{i}] n={n}: rel_l2 {err:.2e}')
            assert err < 1e-6, (terms, gs, given, name, i, n, err)
        _check_omega(what, S.A, i, _path0(given)[i], inp['g'][i], gs, inp['p'][i], S.P.views[i].cpu())
    if l2 is not None:
        assert abs(float(l2[0]) - l2_ref) <= 2e-6 * l2_ref
    if ewc is not None:
        assert abs(float(ewc[0]) - ewc_ref) <= 2e-6 * ewc_ref
    # the same launch from the same state: the same bits
    S.restore()
    ewc2, l22 = _adam_launch(C, S, True, anchored, consolidated, l2_lam > 0, gs, l2_lam, ewc_lam)
    for a, b in zip(got, S.bits()):
        assert torch.equal(a, b)
    assert ewc is None or torch.equal(ewc.view(torch.int32), ewc2.view(torch.int32))
    assert l2 is None or torch.equal(l2.view(torch.int32), l22.view(torch.int32))
    if gs == 1.0 and terms == 'none':
        # tracking must not change the step: the scaled gradient is exact and no other expression gains a second use
        U = AdamState(given)
        _adam_launch(C, U, False, False, False, False, gs, 0.0, 0.0)
        for name, a, b in (('p', S.P, U.P), ('m', S.M, U.M), ('v', S.V, U.V)):
            assert torch.equal(a.flat.view(torch.int32), b.flat.view(torch.int32)), f'{name}: the tracked step differs from the untracked one'
        assert _unchanged(U.A), 'the untracked step touched the path integral'


# ------------------------------------------------------------------------------------------------------------------------------- SGD
_BUF0 = []


def _buf0(given):
    """The momentum buffers of the given state: standard normal, generated once.  p, g, old and the importance of the SGD cases are the
    Adam grid's.  test_sgd_gpu's own inputs do not serve the rel_l2 bound asked for here: its one-element tensor is ill-conditioned (the
    parameter and its update nearly cancel), and a plain fp32 NumPy evaluation of the formula is already 2.0e-6 away from the float64
    restatement there.  With these inputs that evaluation stays within 1.9e-7 for every tensor and setting of the grid below (the same
    consideration test_adam_grid_gpu._inputs records), so the 1e-6 bound measures the kernel and not the inputs."""
    if not _BUF0:
        rng = np.random.default_rng(33)
        _BUF0.extend(torch.from_numpy(rng.standard_normal(n).astype(np.float32)) for n in SIZES)
    return _BUF0 if given else [torch.zeros(n) for n in SIZES]


class SgdState:
    def __init__(self, given, with_buf):
        inp = adam_inputs()
        self.buf0 = _buf0(given)
        self.P = Banded(SIZES, SGD_PHASES['p'], inp['p'])
        self.G = Banded(SIZES, SGD_PHASES['g'], inp['g'])
        self.B = Banded(SIZES, SGD_PHASES['buf'], self.buf0) if with_buf else None
        self.OLD = Banded(SIZES, SGD_PHASES['old'], inp['old'])
        self.OM = Banded(SIZES, SGD_PHASES['omega'], inp['omega'])
        self.A = Banded(SIZES, PATH_PHASES, _path0(given))
        self.written = [b for b in (self.P, self.B, self.A) if b is not None]

    def restore(self):
        for b in self.written:
            b.restore()

    def bits(self):
        return [b.flat.view(torch.int32).clone() for b in self.written]


def _sgd_launch(C, S, tracked, anchored, consolidated, l2_on, hyper):
    from continual_learning_amd.optim import _SGD_TENSOR_DT
    rows = [(S.P.views[i].data_ptr(), S.G.views[i].data_ptr(), S.B.views[i].data_ptr() if S.B is not None else 0,
             S.OLD.views[i].data_ptr() if anchored else 0, n, 0.0 if i == NO_DECAY else 1.0, 0.0) for i, n in enumerate(SIZES)]
    tensors, chunks, nch = _jobs(C, rows, _SGD_TENSOR_DT)
    hyper_dev = torch.tensor(hyper, dtype=torch.float32, device=DEV)
    imp = _ptrs(S.OM.views) if consolidated else None
    ewc = torch.full((1 + nch,), POISON, device=DEV) if consolidated else None
    l2 = torch.full((1 + nch,), POISON, device=DEV) if l2_on else None
    ptr, call = C._lib.ptr, C._lib.call
    if tracked:
        path = _ptrs(S.A.views)
        call('clamd_sgd_step_tracked', ptr(tensors), ptr(imp), ptr(path), ptr(chunks), nch, ptr(hyper_dev), ptr(ewc), ptr(l2), C._lib.stream_ptr())
    else:
        call('clamd_sgd_step', ptr(tensors), ptr(imp), ptr(chunks), nch, ptr(hyper_dev), ptr(ewc), ptr(l2), C._lib.stream_ptr())
    torch.cuda.synchronize()
    return ewc, l2


@pytest.mark.parametrize('given', [False, True], ids=['zero_state', 'given_state'])
@pytest.mark.parametrize('gs', [1.0, 0.375])
@pytest.mark.parametrize('terms', ['none', 'l2', 'ewc', 'both'])
@pytest.mark.parametrize('wd', [0.0, 0.05])
@pytest.mark.parametrize('mu,nesterov', [(0.0, False), (0.9, False), (0.9, True)])
def test_tracked_sgd_step(C, mu, nesterov, wd, terms, gs, given):
    """clamd_sgd_step_tracked: momentum with and without Nesterov, no momentum buffer, weight decay with decay_mult 0 on row NO_DECAY.
    rel_l2 < 1e-6 per tensor for p and buf and 2e-6 on the sums; omega per element."""
    inp = adam_inputs()
    lr = 0.1
    l2_lam = 0.3 if terms in ('l2', 'both') else 0.0
    ewc_lam = 0.7 if terms in ('ewc', 'both') else 0.0
    anchored, consolidated = terms != 'none', terms in ('ewc', 'both')
    hyper = [lr, mu, wd, 1.0 if nesterov else 0.0, gs, l2_lam, ewc_lam, 0.0]
    S = SgdState(given, mu > 0)
    ewc, l2 = _sgd_launch(C, S, True, anchored, consolidated, l2_lam > 0, hyper)
    got = S.bits()
    for b in S.written:
        assert b.guards_intact(), 'a store outside [0, n) of a tensor'
    for name, b in (('g', S.G), ('old', S.OLD), ('importance', S.OM)):
        assert _unchanged(b), f'{name} was written'
    what = f'sgd mu={mu} nesterov={nesterov} wd={wd} {terms} gs={gs} given={given}'
    l2_ref = ewc_ref = 0.0
    for i, n in enumerate(SIZES):
        ref = path_ref.sgd_step_tracked(inp['p'][i].numpy(), inp['g'][i].numpy(), S.buf0[i].numpy() if mu > 0 else None, _path0(given)[i].numpy(),
                                        inp['old'][i].numpy() if anchored else None, inp['omega'][i].numpy() if consolidated else None,
                                        lr=f32(lr), momentum=f32(mu), weight_decay=f32(wd), nesterov=nesterov, grad_scale=f32(gs),
                                        decay_mult=0.0 if i == NO_DECAY else 1.0, l2_lambda=f32(l2_lam), ewc_lambda=f32(ewc_lam))
        l2_ref += ref['l2']
        ewc_ref += ref['ewc']
        for name, b in (('p', S.P), ('buf', S.B)):
            if b is None:
                continue
            err = rel_l2(b.views[i].cpu().numpy(), ref[name])
            print(f'{what} {name}[{i}] n={n}: rel_l2 {err:.2e}')
            assert err < 1e-6, (what, name, i, n, err)
        _check_omega(what, S.A, i, _path0(given)[i], inp['g'][i], gs, inp['p'][i], S.P.views[i].cpu())
    if l2 is not None:
        assert abs(float(l2[0]) - l2_ref) <= 2e-6 * l2_ref
    if ewc is not None:
        assert abs(float(ewc[0]) - ewc_ref) <= 2e-6 * ewc_ref
    S.restore()
    ewc2, l22 = _sgd_launch(C, S, True, anchored, consolidated, l2_lam > 0, hyper)
    for a, b in zip(got, S.bits()):
        assert torch.equal(a, b)
    assert ewc is None or torch.equal(ewc.view(torch.int32), ewc2.view(torch.int32))
    assert l2 is None or torch.equal(l2.view(torch.int32), l22.view(torch.int32))
    if gs == 1.0 and terms == 'none' and wd == 0.0:
        U = SgdState(given, mu > 0)
        _sgd_launch(C, U, False, False, False, False, hyper)
        for a, b in zip(S.written[:-1], U.written[:-1]):
            assert torch.equal(a.flat.view(torch.int32), b.flat.view(torch.int32)), 'the tracked step differs from the untracked one'
        assert _unchanged(U.A), 'the untracked step touched the path integral'


# -------------------------------------------------------------------------------------------------------------------------- boundary
_BOUNDARY = {}


def _boundary_inputs():
    """importance in [0, 2); the path normal with negative, exactly zero (10 %) and positive entries; p normal; start = p exactly on a
    quarter of the elements (the denominator is xi there), normal elsewhere."""
    if not _BOUNDARY:
        rng = np.random.default_rng(32)
        imp, path, p, start = [], [], [], []
        for n in SIZES:
            imp.append(torch.from_numpy((rng.random(n) * 2).astype(np.float32)))
            a = rng.standard_normal(n).astype(np.float32)
            a[rng.random(n) < 0.1] = 0.0
            path.append(torch.from_numpy(a))
            w = rng.standard_normal(n).astype(np.float32)
            s = rng.standard_normal(n).astype(np.float32)
            same = rng.random(n) < 0.25
            s[same] = w[same]
            p.append(torch.from_numpy(w))
            start.append(torch.from_numpy(s))
        path[0][0], path[1][:] = 0.5, torch.tensor([-1.0, 0.0, 2.0])      # the one- and three-element tensors: every kind is present
        start[1][2] = p[1][2]
        _BOUNDARY.update(importance=imp, path=path, p=p, start=start)
    return _BOUNDARY


@pytest.mark.parametrize('xi', [0.1, 1e-3])
@pytest.mark.parametrize('decay', [0.7, 1.0])
def test_path_importance_per_element(C, decay, xi):
    """clamd_path_importance on the same sizes, every buffer at its own phase: _check_importance's bound (1e-6 relative per element in the
    normal range: a handful of fp32 roundings, all terms >= 0) against the float64 formula; exactly fl(decay * importance) where the path
    is <= 0; path, p and start bit-unchanged; guards intact; two runs bit-identical."""
    inp = _boundary_inputs()
    W = Banded(SIZES, PATH_PHASES, inp['importance'])
    A = Banded(SIZES, (0, 1, 2, 3, 1, 2), inp['path'])
    P = Banded(SIZES, (1, 0, 3, 0, 2, 1), inp['p'])
    S = Banded(SIZES, (2, 3, 0, 1, 0, 3), inp['start'])
    assert C._lib.load().clamd_sizeof_path_tensor() == PATH_ROW.itemsize == 40
    rows = [(W.views[i].data_ptr(), A.views[i].data_ptr(), P.views[i].data_ptr(), S.views[i].data_ptr(), n) for i, n in enumerate(SIZES)]
    tensors, chunks, nch = _jobs(C, rows, PATH_ROW)
    ptr = C._lib.ptr
    outs = []
    for _ in range(2):
        W.restore()
        C._lib.call('clamd_path_importance', ptr(tensors), ptr(chunks), nch, decay, xi, C._lib.stream_ptr())
        torch.cuda.synchronize()
        outs.append(W.flat.view(torch.int32).clone())
    assert torch.equal(outs[0], outs[1]), 'two runs differ'
    assert W.guards_intact(), 'a store outside [0, n) of a tensor'
    for name, b in (('path', A), ('p', P), ('start', S)):
        assert _unchanged(b), f'{name} was written'
    kinds = set()
    for i, n in enumerate(SIZES):
        got = W.views[i].cpu().numpy()
        want = path_ref.path_importance(inp['importance'][i].numpy(), inp['path'][i].numpy(), inp['p'][i].numpy(), inp['start'][i].numpy(),
                                        decay=f32(decay), xi=f32(xi))
        e = _check_importance(got, want, f'path importance decay={decay} xi={xi} tensor {i} n={n}')
        print(f'path importance decay={decay} xi={xi} [{i}] n={n}: max relative error {e:.2e}')
        off = inp['path'][i].numpy() <= 0
        exact = np.float32(decay) * inp['importance'][i].numpy()
        assert np.array_equal(got[off].view(np.int32), exact[off].view(np.int32)), f'tensor {i}: path <= 0 must leave fl(decay * importance)'
        assert np.all(got[~off] >= exact[~off])
        same = (inp['p'][i] == inp['start'][i]).numpy()
        kinds |= {('neg', bool((inp['path'][i] < 0).any())), ('zero', bool((inp['path'][i] == 0).any())), ('same', bool((same & ~off).any()))}
    assert {('neg', True), ('zero', True), ('same', True)} <= kinds
