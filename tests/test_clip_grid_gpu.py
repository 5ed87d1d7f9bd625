"""GPU: clamd_grad_norm_clip (csrc/optim.hip) through tables built here -- the norm pass and the finalize kernel across the sizes of
test_adam_grid_gpu.py (below, at and above one chunk, every gradient phase of a 16-byte line, inside a poisoned buffer with guard bands),
one tensor of 301 chunks (past any 64- or 256-wide stride of the finalize) and a table of 300 tiny tensors (more tensors than finalize
lanes or waves).  Norm, per-tensor norms and coefficient against float64 (tests/clip_ref.py); hyper_eff bit for bit; the exact, zero and
non-finite cases; the gradients bit-unchanged; two launches bit-identical; and the unchanged Adam and SGD step kernels launched on
hyper_eff bit-identical to the same launch on a host-built hyper buffer, and right against their float64 references."""
import math

import numpy as np
import pytest
import torch

import clip_ref
import sgd_ref
from conftest import rel_l2
from grid_util import Banded, DEV, POISON, RATIOS, Rows, _per_element
from oracle import np_unet
from test_adam_grid_gpu import ADAM_ROW, BETA1, BETA2, EPS, LR, PHASES, SIZES, State, _inputs as adam_inputs, f32
from test_path_grid_gpu import SgdState

pytestmark = pytest.mark.gpu

GRAD_ROW = np.dtype([('g', 'u8'), ('n', 'i8'), ('first_chunk', 'i4'), ('nchunks', 'i4')])
BIG = 300 * 4096 + 5                           # 301 partials for one tensor
REL = 1e-6                                     # relative bound on norm, per-tensor norms and coefficient: a NumPy emulation of a blocked
#                                                fp32 sum of squares (16 elements per lane, 256-lane tree, fp64 over the partials) of these
#                                                inputs stays within 2.6e-8 of float64, so the bound measures the kernel, not the inputs
HYPER = [LR, BETA1, BETA2, EPS, None, 0.3, 0.7, 0.0]


@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    C._lib.load()
    return C


_TABLES = {}


def _tables():
    """Host values, generated once.  'grid': the six gradients of test_adam_grid_gpu._inputs (seed 12, 5 % exact zeros) at its gradient
    phases and one tensor of BIG elements at phase 3, generated the same way.  'many': 300 tensors of 1..7 elements, phases cycling."""
    if not _TABLES:
        rng = np.random.default_rng(12012)
        big = rng.standard_normal(BIG).astype(np.float32)
        big[rng.random(BIG) < 0.05] = 0.0
        _TABLES['grid'] = (SIZES + (BIG,), PHASES['g'] + (3,), list(adam_inputs()['g']) + [torch.from_numpy(big)])
        sizes = tuple(1 + i % 7 for i in range(300))
        vals = []
        for n in sizes:
            a = rng.standard_normal(n).astype(np.float32)
            a[rng.random(n) < 0.05] = 0.0
            vals.append(torch.from_numpy(a))
        _TABLES['many'] = (sizes, tuple((i * 3) % 4 for i in range(300)), vals)
    return _TABLES


class Clip:
    """One table's gradients in a Banded buffer, the device tables, and poisoned outputs with guard bands."""

    def __init__(self, C, sizes, phases, values):
        self.C, self.sizes = C, sizes
        lib = C._lib.load()
        assert lib.clamd_sizeof_grad_tensor() == GRAD_ROW.itemsize == 24
        chunk = lib.clamd_adam_chunk_elems()
        self.G = Banded(sizes, phases, values)
        t = np.zeros(len(sizes), dtype=GRAD_ROW)
        chunks = []
        for i, n in enumerate(sizes):
            k = (n + chunk - 1) // chunk
            t[i] = (self.G.views[i].data_ptr(), n, len(chunks), k)
            chunks += [(i, c) for c in range(k)]
        self.nchunks = len(chunks)
        self.tensors = torch.from_numpy(t.view(np.uint8).copy()).to(DEV)
        self.chunks = torch.tensor(chunks, dtype=torch.int32, device=DEV)

    def launch(self, gs, max_norm, with_tensor_norms=True):
        """-> (partials, clip_out, tensor_norms, hyper_eff, hyper) after a synchronise; the outputs are fresh poisoned Rows."""
        C, ptr = self.C, self.C._lib.ptr
        hyper = torch.tensor([gs if v is None else v for v in HYPER], dtype=torch.float32, device=DEV)
        part, out, eff = Rows(self.nchunks, fill=POISON), Rows(4, fill=POISON), Rows(8, fill=POISON)
        norms = Rows(len(self.sizes), fill=POISON) if with_tensor_norms else None
        C._lib.call('clamd_grad_norm_clip', ptr(self.tensors), len(self.sizes), ptr(self.chunks), self.nchunks, ptr(hyper), float(max_norm),
                    part.ptr, out.ptr, norms.ptr if norms is not None else None, eff.ptr, C._lib.stream_ptr())
        torch.cuda.synchronize()
        return part, out, norms, eff, hyper

    def unchanged(self):
        return torch.equal(self.G.flat.view(torch.int32), self.G.before.view(torch.int32))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ratio(what, got, want):
    """|got - want| / (REL * |want|); an exact zero must be returned as zero."""
    if want == 0.0:
        assert got == 0.0, (what, got)
        return 0.0
    r = abs(got - want) / (REL * abs(want))
    RATIOS['clip'] = max(RATIOS.get('clip', 0.0), r)
    assert r <= 1.0, f'{what}: got {got!r}, float64 {want!r}, error / bound {r:.3f}'
    return r


@pytest.mark.parametrize('where', ['half', 'double', 'inf'])
@pytest.mark.parametrize('gs', [1.0, 0.5, -0.25])
@pytest.mark.parametrize('table', ['grid', 'many'])
def test_norm_and_coefficient_against_float64(C, table, gs, where):
    sizes, phases, values = _tables()[table]
    ref1 = clip_ref.clip([v.numpy() for v in values], math.inf, gs)
    max_norm = {'half': 0.5 * ref1['norm'], 'double': 2.0 * ref1['norm'], 'inf': math.inf}[where]
    ref = clip_ref.clip([v.numpy() for v in values], max_norm, gs)
    K = Clip(C, sizes, phases, values)
    part, out, norms, eff, hyper = K.launch(gs, max_norm)
    for name, r in (('partials', part), ('clip_out', out), ('tensor_norms', norms), ('hyper_eff', eff)):
        assert r.guards_intact(), f'{name}: a store outside the buffer'
    assert K.unchanged() and K.G.guards_intact(), 'the gradients were written'
    got = out.view.cpu().double().numpy()
    worst = _ratio('norm', got[0], ref['norm'])
    worst = max(worst, _ratio('coef', got[1], ref['coef']))
    tn = norms.view.cpu().double().numpy()
    for i, n in enumerate(sizes):
        worst = max(worst, _ratio(f'tensor_norms[{i}] n={n}', tn[i], ref['tensor_norms'][i]))
    print(f'clip {table} gs={gs} max_norm={where}: norm {got[0]:.7g} coef {got[1]:.7g}; worst error / bound {worst:.4f} '
          f"(largest so far {RATIOS.get('clip', 0.0):.4f})")
    assert got[3] == 0.0
    if where == 'half':
        assert got[1] < 1.0
    else:
        assert got[1] == 1.0                            # exactly: nothing may move an unclipped step
    # the partials add up to the tensors' sums (float64 over fp32 partials), and every one of them was written
    p64 = part.view.cpu().double().numpy().reshape(-1)
    assert not np.any(p64 == POISON) and np.all(p64 >= 0)
    _ratio('sum of partials', math.sqrt(p64.sum()) * abs(gs), ref1['norm'])
    # hyper_eff: hyper bit for bit except slot 4 = fp32(gs) * coef, one fp32 product of the read-back coefficient
    coef32, eff32 = out.view.cpu().numpy().reshape(-1)[1], out.view.cpu().numpy().reshape(-1)[2]
    assert eff32.view(np.int32) == (np.float32(gs) * coef32).view(np.int32)
    want = hyper.clone()
    want[4] = float(eff32)
    assert torch.equal(_bits(eff.view.reshape(-1)), _bits(want))
    # without the optional per-tensor output, and a second time: the same bits everywhere
    part2, out2, none, eff2, _ = K.launch(gs, max_norm, with_tensor_norms=False)
    assert none is None
    part3, out3, norms3, eff3, _ = K.launch(gs, max_norm)
    for a, b in ((part, part2), (out, out2), (eff, eff2), (part, part3), (out, out3), (norms, norms3), (eff, eff3)):
        assert torch.equal(_bits(a.buf), _bits(b.buf)), 'two launches differ'


def test_zero_gradient(C):
    sizes, phases, _ = _tables()['grid']
    K = Clip(C, sizes[:6], phases[:6], [torch.zeros(n) for n in sizes[:6]])
    _, out, norms, eff, _ = K.launch(0.5, 1.0)
    got = out.view.cpu().numpy().reshape(-1)
    assert got[0] == 0.0 and got[1] == 1.0 and got[2] == 0.5 and got[3] == 0.0
    assert not norms.view.any() and float(eff.view.reshape(-1)[4]) == 0.5


@pytest.mark.parametrize('bad', [math.nan, math.inf, -math.inf])
@pytest.mark.parametrize('where', [(3, 4094), (6, BIG - 1), (0, 0)], ids=['tail', 'last_of_big', 'single'])
def test_non_finite_gradient(C, where, bad):
    """One NaN element: NaN norm, NaN coefficient, NaN effective scale, flag 1 (torch with error_if_nonfinite=False).  One infinite element:
    an infinite norm, coefficient 0, flag 1.  Only the tensor that holds it reports it."""
    sizes, phases, values = _tables()['grid']
    i, j = where
    values = [v.clone() for v in values]
    values[i][j] = bad
    K = Clip(C, sizes, phases, values)
    _, out, norms, eff, _ = K.launch(1.0, 1.0)
    got = out.view.cpu().numpy().reshape(-1)
    tn = norms.view.cpu().numpy().reshape(-1)
    assert got[3] == 1.0
    if math.isnan(bad):
        assert np.isnan(got[0]) and np.isnan(got[1]) and np.isnan(got[2]) and np.isnan(tn[i])
        assert math.isnan(float(eff.view.reshape(-1)[4]))
    else:
        assert got[0] == np.inf and got[1] == 0.0 and got[2] == 0.0 and tn[i] == np.inf
    assert np.isfinite(np.delete(tn, i)).all()
    assert K.unchanged()


def _grad_table(C, views, sizes):
    chunk = C._lib.load().clamd_adam_chunk_elems()
    t = np.zeros(len(sizes), dtype=GRAD_ROW)
    first = 0
    for i, n in enumerate(sizes):
        k = (n + chunk - 1) // chunk
        t[i] = (views[i].data_ptr(), n, first, k)
        first += k
    return torch.from_numpy(t.view(np.uint8).copy()).to(DEV), first


def _step_tables(C, rows, dtype):
    chunk = C._lib.load().clamd_adam_chunk_elems()
    t = np.zeros(len(SIZES), dtype=dtype)
    chunks = []
    for i, n in enumerate(SIZES):
        t[i] = rows[i]
        chunks += [(i, c) for c in range((n + chunk - 1) // chunk)]
    return torch.from_numpy(t.view(np.uint8).copy()).to(DEV), torch.tensor(chunks, dtype=torch.int32, device=DEV), len(chunks)


def _clip_into(C, G, hyper, max_norm, chunks, nch):
    """The norm pass over the step's own job list -> (clip_out, hyper_eff) device tensors."""
    ptr = C._lib.ptr
    gt, first = _grad_table(C, G.views, SIZES)
    assert first == nch
    part = torch.full((nch,), POISON, device=DEV)
    out, eff = torch.full((4,), POISON, device=DEV), torch.full((8,), POISON, device=DEV)
    C._lib.call('clamd_grad_norm_clip', ptr(gt), len(SIZES), ptr(chunks), nch, ptr(hyper), float(max_norm), ptr(part), ptr(out), None, ptr(eff),
                C._lib.stream_ptr())
    return out, eff


def test_adam_step_on_hyper_eff(C):
    """clamd_adam_step launched on hyper_eff leaves the bits of p, m and v that the same launch on a host-built hyper buffer whose slot 4 is
    the read-back clip_out[2] leaves: the step kernel is untouched and the coefficient reaches it.  And the result is right: p, m, v against
    oracle.np_unet.adam_step with grad_scale = clip_out[2] at test_adam_step_per_tensor's bound."""
    inp = adam_inputs()
    gs = 0.5
    ptr, call = C._lib.ptr, C._lib.call
    max_norm = 0.5 * clip_ref.clip([g.numpy() for g in inp['g']], math.inf, gs)['norm']
    runs = []
    eff_scale = None
    for on_eff in (True, False):
        S = State(True)
        rows = [(S.P.views[i].data_ptr(), S.G.views[i].data_ptr(), S.M.views[i].data_ptr(), S.V.views[i].data_ptr(), 0, n) for i, n in enumerate(SIZES)]
        tensors, chunks, nch = _step_tables(C, rows, ADAM_ROW)
        hyper = torch.tensor([LR, BETA1, BETA2, EPS, gs, 0.0, 0.0, 0.0], dtype=torch.float32, device=DEV)
        derived = torch.zeros(2, dtype=torch.float32, device=DEV)
        if on_eff:
            out, step_hyper = _clip_into(C, S.G, hyper, max_norm, chunks, nch)
        else:
            step_hyper = torch.tensor([LR, BETA1, BETA2, EPS, eff_scale, 0.0, 0.0, 0.0], dtype=torch.float32, device=DEV)
        call('clamd_adam_step', ptr(tensors), ptr(chunks), nch, ptr(step_hyper), ptr(S.step), ptr(derived), None, C._lib.stream_ptr())
        torch.cuda.synchronize()
        if on_eff:
            eff_scale = float(out[2])
            assert 0 < float(out[1]) < 1 and eff_scale == float(np.float32(gs) * out.cpu().numpy()[1])
        for b in (S.P, S.M, S.V):
            assert b.guards_intact()
        assert torch.equal(S.G.flat.view(torch.int32), S.G.before.view(torch.int32))
        runs.append(S)
    a, b = runs
    for x, y in zip(a.bits(), b.bits()):
        assert torch.equal(x, y), 'the step on hyper_eff differs from the step on the host-built hyper buffer'
    for i, n in enumerate(SIZES):
        p, g, m, v = (inp[k][i].numpy().astype(np.float64) for k in ('p', 'g', 'm', 'v'))
        rp, rm, rv = np_unet.adam_step(p, g * eff_scale, m, v, 4, f32(LR), f32(BETA1), f32(BETA2), f32(EPS))
        for name, buf, ref in (('p', a.P, rp), ('m', a.M, rm), ('v', a.V, rv)):
            err = rel_l2(buf.views[i].cpu().numpy(), ref)
            print(f'clipped adam {name}[{i}] n={n}: rel_l2 {err:.2e}')
            assert err < 1e-6, (name, i, n, err)


@pytest.mark.parametrize('tracked', [False, True], ids=['sgd_step', 'sgd_step_tracked'])
def test_sgd_step_on_hyper_eff(C, tracked):
    """The same for clamd_sgd_step and clamd_sgd_step_tracked (momentum 0.9, Nesterov, weight decay): bit-identical to the launch on the
    host-built hyper buffer; p and buf per element against tests/sgd_ref.py with grad_scale = clip_out[2] within sgd_ref.bounds."""
    from continual_learning_amd.optim import _SGD_TENSOR_DT
    inp = adam_inputs()
    gs, lr, mu, wd = -0.25, 0.1, 0.9, 0.05
    ptr, call = C._lib.ptr, C._lib.call
    max_norm = 0.5 * clip_ref.clip([g.numpy() for g in inp['g']], math.inf, gs)['norm']
    runs = []
    eff_scale = None
    for on_eff in (True, False):
        S = SgdState(True, True)
        rows = [(S.P.views[i].data_ptr(), S.G.views[i].data_ptr(), S.B.views[i].data_ptr(), 0, n, 1.0, 0.0) for i, n in enumerate(SIZES)]
        tensors, chunks, nch = _step_tables(C, rows, _SGD_TENSOR_DT)
        hyper = torch.tensor([lr, mu, wd, 1.0, gs, 0.0, 0.0, 0.0], dtype=torch.float32, device=DEV)
        if on_eff:
            out, step_hyper = _clip_into(C, S.G, hyper, max_norm, chunks, nch)
        else:
            step_hyper = torch.tensor([lr, mu, wd, 1.0, eff_scale, 0.0, 0.0, 0.0], dtype=torch.float32, device=DEV)
        if tracked:
            path = torch.tensor([w.data_ptr() for w in S.A.views], dtype=torch.int64).to(DEV)
            call('clamd_sgd_step_tracked', ptr(tensors), None, ptr(path), ptr(chunks), nch, ptr(step_hyper), None, None, C._lib.stream_ptr())
        else:
            call('clamd_sgd_step', ptr(tensors), None, ptr(chunks), nch, ptr(step_hyper), None, None, C._lib.stream_ptr())
        torch.cuda.synchronize()
        if on_eff:
            eff_scale = float(out[2])
            assert 0 < float(out[1]) < 1 and eff_scale < 0
        for b in S.written:
            assert b.guards_intact()
        assert torch.equal(S.G.flat.view(torch.int32), S.G.before.view(torch.int32))
        runs.append(S)
    a, b = runs
    for x, y in zip(a.bits(), b.bits()):
        assert torch.equal(x, y), 'the step on hyper_eff differs from the step on the host-built hyper buffer'
    assert tracked or torch.equal(a.A.flat.view(torch.int32), a.A.before.view(torch.int32))
    for i, n in enumerate(SIZES):
        ref = sgd_ref.sgd_step(inp['p'][i].numpy(), inp['g'][i].numpy(), a.buf0[i].numpy(), lr=f32(lr), momentum=f32(mu), weight_decay=f32(wd),
                               nesterov=True, grad_scale=eff_scale)
        bb, pb = sgd_ref.bounds(inp['p'][i].numpy(), ref, lr=f32(lr), momentum=f32(mu))
        _per_element(f'clipped sgd p[{i}] n={n}', ('clip_sgd', tracked), a.P.views[i].cpu(), torch.from_numpy(ref['p']), torch.from_numpy(pb))
        _per_element(f'clipped sgd buf[{i}] n={n}', ('clip_sgd', tracked), a.B.views[i].cpu(), torch.from_numpy(ref['buf']), torch.from_numpy(bb))
