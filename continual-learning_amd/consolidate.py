"""Elastic weight consolidation: the per-parameter importance of a finished task (build-defined, SURVEY.md §0.1 / §8a A12 -- the reference
has no continual-learning code, so parity is unpinned).

    importance  Omega = (1/N) sum_b g_b * g_b,   g_b = gradient of the loss on batch b, model in eval mode
    penalty     P = (lam/2) sum_i Omega_i (theta_i - theta*_i)^2        (optim.FusedAdam.set_consolidation adds its gradient)
    online EWC  Omega <- gamma * Omega_prev + Omega_new, anchor theta* replaced by the current weights

``Consolidation`` owns ONE flat fp32 importance buffer (per-parameter views into it), a clone of the weights it was created on (the
anchor), the batch count and the device tables of ``clamd_importance_accum``.  All arithmetic is that one element-wise kernel: one launch
per ``accumulate`` for all parameter tensors, deterministic, no CPU fallback.

Per image or per batch: ``accumulate`` squares whatever gradient the last backward left in ``p.grad``.  Fed from a loader of batch size 1 the
result is the per-image empirical Fisher diagonal; with larger batches it is the square of the batch-MEAN gradient (the criterion averages
over the pixels of the whole batch), the variant many implementations use -- smaller by roughly the batch size where per-image gradients
are uncorrelated.  Labels sampled from the model's own softmax ("true" Fisher) and MAS are not provided.

Synaptic Intelligence (Zenke et al. 2017, the "PI" baseline; build-defined as well): the other importance estimate, gathered while the task
trains instead of after it.

    per step    omega_i += -g_i * (theta_i(t+1) - theta_i(t)),   g = the task-loss gradient the optimiser is handed, inside its kernel
    boundary    Omega_i <- decay * Omega_i + max(0, omega_i) / ((theta_i - theta_start_i)^2 + xi);  theta* <- theta;  omega <- 0;
                theta_start <- theta
    penalty     c * sum_i Omega_i (theta_i - theta*_i)^2  =  the consolidation term above with lam = 2 c

``PathIntegral`` owns ONE flat fp32 omega buffer (per-parameter views, installed with ``optim.set_path_integral``) and a clone of the
weights at the start of the current task; ``consolidate`` runs ``clamd_path_importance`` once over all tensors and hands back a finished
``Consolidation``.
"""
import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from ._lib import ptr

_ROW_DT = np.dtype([('dst', 'u8'), ('src', 'u8'), ('n', 'i8')])


def _flat_views(shapes, device):
    """One flat fp32 buffer of zeros and the per-parameter views into it."""
    flat = torch.zeros(sum(int(np.prod(sh)) for sh in shapes), dtype=torch.float32, device=device)
    views, off = [], 0
    for shape in shapes:
        k = int(np.prod(shape))
        views.append(flat[off:off + k].view(shape))
        off += k
    return flat, views


def _grown(who, names, shapes, views, kept, name, new_param):
    """Class-incremental head growth of a flat per-parameter buffer and of one per-parameter clone of the weights, for Consolidation.grow
    and PathIntegral.grow: parameter `name` now has more rows along dim 0 (anything else: ValueError).  The flat buffer is laid out again
    once -- every tensor keeps its values, the new rows are zero -- and that parameter's entry of `kept` (per-parameter clones of the
    weights) keeps its old rows and takes new_param's current value in the new ones.  Returns (flat, views, shapes, kept)."""
    if name not in names:
        raise KeyError(f'{who}.grow: no parameter {name!r}')
    i = names.index(name)
    old, new = shapes[i], tuple(new_param.shape)
    if len(new) != len(old) or len(old) < 1 or new[0] <= old[0] or new[1:] != old[1:]:
        raise ValueError(f'{who}.grow: {name}: {old} -> {new} is not growth along dim 0')
    shapes = list(shapes)
    shapes[i] = new
    flat, grown = _flat_views(shapes, views[i].device)
    for j, (w, v) in enumerate(zip(grown, views)):
        (w[:old[0]] if j == i else w).copy_(v)
    clone = new_param.detach().clone().float().contiguous().to(views[i].device)
    clone[:old[0]].copy_(kept[i])
    kept = list(kept)
    kept[i] = clone
    return flat, grown, shapes, kept


class Consolidation:
    def __init__(self, named_params, gamma=1.0):
        """named_params: iterable of (name, tensor), e.g. ``model.named_parameters()``; their current values become the anchor."""
        named = [(n, p.detach()) for n, p in named_params]
        if not named:
            raise ValueError('Consolidation: no parameters')
        self.names = [n for n, _ in named]
        self.shapes = [tuple(p.shape) for _, p in named]
        self.device = named[0][1].device
        self.anchor = [p.clone().float().contiguous() for _, p in named]
        self.flat, self.importance = _flat_views(self.shapes, self.device)
        self.n_batches = 0
        self.gamma = float(gamma)
        self.finished = False
        self._tables = {}             # tuple of source pointers -> (rows, chunks, nchunks) on the device

    # ---- device tables ------------------------------------------------------------------------------------------
    def _table(self, srcs):
        """(rows, chunks, nchunks) of one clamd_importance_accum launch that reads `srcs` (aligned with the importance views)."""
        for n, w, s in zip(self.names, self.importance, srcs):
            if not (w.is_cuda and s.is_cuda and s.device == w.device and s.dtype == torch.float32 and s.is_contiguous() and s.shape == w.shape):
                raise RuntimeError(f'Consolidation: {n} needs a contiguous fp32 GPU tensor of shape {tuple(w.shape)} on {w.device}: '
                                   f'there is no CPU fallback')
        key = tuple(s.data_ptr() for s in srcs)
        tab = self._tables.get(key)
        if tab is None:
            rows = [(w.data_ptr(), s.data_ptr(), w.numel()) for w, s in zip(self.importance, srcs)]
            if len(self._tables) >= 4:          # gradients that move every step: do not pile tables up
                self._tables.clear()
            tab = self._tables[key] = _lib.job_table(_ROW_DT, rows, [w.numel() for w in self.importance], self.device,
                                                     'clamd_sizeof_importance_tensor')
        return tab

    def _launch(self, srcs, decay, scale, power):
        from . import unet as U
        rows, chunks, nchunks = self._table(srcs)
        U._hbm('importance', 12 * self.flat.numel(),        # dst and src read, dst written
               'clamd_importance_accum', ptr(rows), ptr(chunks), nchunks, float(decay), float(scale), int(power), _lib.stream_ptr())

    # ---- the estimate ---------------------------------------------------------------------------------------------
    def accumulate(self, params):
        """importance += p.grad ** 2 for every parameter, in one launch; counts one batch.  Enqueue only."""
        if self.finished:
            raise RuntimeError('Consolidation.accumulate after finish()')
        params = list(params)
        if len(params) != len(self.importance):
            raise ValueError(f'Consolidation.accumulate: {len(params)} parameters, {len(self.importance)} expected')
        grads = []
        for n, p in zip(self.names, params):
            if p.grad is None:
                raise RuntimeError(f'Consolidation.accumulate: {n} has no gradient')
            grads.append(p.grad)
        self._launch(grads, 1.0, 1.0, 2)
        self.n_batches += 1

    def finish(self, group=None):
        """Sum of squares -> mean of squares.  Under an initialised process group the flat sums and the batch counts are all-reduced first:
        every rank ends with the mean over all ranks' batches (bit-identical across ranks).  Synchronises when a group is initialised."""
        if self.finished:
            raise RuntimeError('Consolidation.finish called twice')
        n = self.n_batches
        if dist.is_available() and dist.is_initialized():
            count = torch.tensor([float(n)], dtype=torch.float64, device=self.device)
            dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=group)
            dist.all_reduce(count, op=dist.ReduceOp.SUM, group=group)
            n = int(round(float(count)))
        if n <= 0:
            raise RuntimeError('Consolidation.finish: no batch was accumulated')
        self.n_batches = n
        self._launch(self.importance, 1.0 / n, 0.0, 1)
        self._tables.clear()
        self.finished = True
        return self

    def merge_from(self, previous, gamma=None):
        """Online EWC: importance <- gamma * previous.importance + importance (this object keeps its own, newer anchor)."""
        gamma = self.gamma if gamma is None else float(gamma)
        if not (self.finished and previous.finished):
            raise RuntimeError('Consolidation.merge_from needs two finished estimates')
        if previous.names != self.names or previous.shapes != self.shapes:
            raise ValueError('Consolidation.merge_from: the two estimates cover different parameters')
        self._launch(previous.importance, 1.0, gamma, 1)
        self._tables.clear()
        self.gamma = gamma
        return self

    @torch.no_grad()
    def grow(self, name, new_param):
        """Class-incremental head growth: parameter `name` now has more rows along dim 0 (UNet.expand_classes).  The flat importance buffer
        is laid out again once: old rows keep their importance, the new rows get zero, and their anchor is new_param's current (initial)
        value -- no pull on classes the finished task never had.  Anything but growth along dim 0 is a ValueError."""
        self.flat, self.importance, self.shapes, self.anchor = _grown('Consolidation', self.names, self.shapes, self.importance, self.anchor,
                                                                      name, new_param)
        self._tables.clear()
        return self

    # ---- checkpoints ------------------------------------------------------------------------------------------------
    def state_dict(self):
        """Tensors by parameter NAME (views of this object's buffers: clone or copy them to keep them)."""
        return {'importance': dict(zip(self.names, self.importance)), 'anchor': dict(zip(self.names, self.anchor)),
                'n_batches': self.n_batches, 'gamma': self.gamma}

    def load_state_dict(self, state):
        for kind in ('importance', 'anchor'):
            if set(state[kind]) != set(self.names):
                missing, extra = sorted(set(self.names) - set(state[kind])), sorted(set(state[kind]) - set(self.names))
                raise KeyError(f'Consolidation.load_state_dict: {kind}: missing {missing}, unexpected {extra}')
        for n, w, a in zip(self.names, self.importance, self.anchor):
            for kind, dst in (('importance', w), ('anchor', a)):
                src = state[kind][n]
                if tuple(src.shape) != tuple(dst.shape):
                    raise ValueError(f'Consolidation.load_state_dict: {kind} of {n} has shape {tuple(src.shape)}, expected {tuple(dst.shape)}')
                dst.copy_(src)
        self.n_batches = int(state['n_batches'])
        self.gamma = float(state['gamma'])
        self.finished = True
        return self


_PATH_ROW_DT = np.dtype([('importance', 'u8'), ('path', 'u8'), ('p', 'u8'), ('start', 'u8'), ('n', 'i8')])


class PathIntegral:
    """Synaptic Intelligence's running path integral over the current task: ``omega`` (per-parameter views of ONE flat fp32 buffer, which
    the optimiser's tracked step accumulates into once ``optim.set_path_integral(self.omega)`` installed them) and ``start``, a clone of
    the weights at the start of the task."""

    def __init__(self, named_params, xi=0.1):
        """named_params: iterable of (name, tensor), e.g. ``model.named_parameters()``; their current values become ``start``.
        xi: the damping of the boundary formula, finite and > 0."""
        named = [(n, p.detach()) for n, p in named_params]
        if not named:
            raise ValueError('PathIntegral: no parameters')
        xi = float(xi)
        if not (xi > 0.0 and xi < float('inf')):
            raise ValueError('PathIntegral: xi must be finite and > 0')
        self.xi = xi
        self.names = [n for n, _ in named]
        self.shapes = [tuple(p.shape) for _, p in named]
        self.device = named[0][1].device
        self.start = [p.clone().float().contiguous() for _, p in named]
        self.flat, self.omega = _flat_views(self.shapes, self.device)

    def _check_names(self, who, names):
        if list(names) != self.names:
            raise ValueError(f'PathIntegral.{who}: the parameters are not the ones this path integral was created on')

    @torch.no_grad()
    def consolidate(self, named_params, previous=None, decay=1.0):
        """The task boundary, in ONE launch of clamd_path_importance over all tensors: returns a finished Consolidation whose importance is
        decay * previous.importance (zero without `previous`) + max(0, omega) / ((theta - start)^2 + xi) and whose anchor is a clone of the
        current weights.  omega and start are left as they are: ``restart`` begins the next task.  Enqueue only, no CPU fallback."""
        from . import unet as U
        named = [(n, p.detach()) for n, p in named_params]
        self._check_names('consolidate', [n for n, _ in named])
        cons = Consolidation(named, gamma=decay)
        if previous is not None:
            if previous.names != self.names or previous.shapes != self.shapes:
                raise ValueError('PathIntegral.consolidate: the previous consolidation covers different parameters')
            cons.flat.copy_(previous.flat)
        rows = []
        for n, w, a, (_, p), s in zip(self.names, cons.importance, self.omega, named, self.start):
            if not (p.is_cuda and p.device == a.device and p.dtype == torch.float32 and p.is_contiguous() and tuple(p.shape) == tuple(a.shape)):
                raise RuntimeError(f'PathIntegral: {n} needs a contiguous fp32 GPU tensor of shape {tuple(a.shape)} on {a.device}: '
                                   f'there is no CPU fallback')
            rows.append((w.data_ptr(), a.data_ptr(), p.data_ptr(), s.data_ptr(), a.numel()))
        tab, chunks, nchunks = _lib.job_table(_PATH_ROW_DT, rows, [a.numel() for a in self.omega], self.device, 'clamd_sizeof_path_tensor')
        U._hbm('importance', 20 * self.flat.numel(),        # importance read and written; omega, the weights and their start read
               'clamd_path_importance', ptr(tab), ptr(chunks), nchunks, float(decay), self.xi, _lib.stream_ptr())
        cons.finished = True
        return cons

    @torch.no_grad()
    def restart(self, params):
        """omega <- 0 and start <- the current weights: the next task begins here."""
        params = list(params)
        if len(params) != len(self.start):
            raise ValueError(f'PathIntegral.restart: {len(params)} parameters, {len(self.start)} expected')
        self.flat.zero_()
        for s, p in zip(self.start, params):
            s.copy_(p.detach())
        return self

    @torch.no_grad()
    def grow(self, name, new_param, old_param=None):
        """Class-incremental head growth, as Consolidation.grow: parameter `name` now has more rows along dim 0.  The flat omega buffer is
        laid out again once: old rows of omega and start are kept, the new rows get zero omega and new_param's current (initial) value as
        their start.  Anything but growth along dim 0 is a ValueError.  old_param (the parameter as it was): where the growth rewrote an
        old row (UNet.expand_classes with init='background' moves the background row), start moves by the same amount, so the tracked
        steps still telescope to theta - start at the next boundary; rows the growth left alone get an exact zero."""
        if name not in self.names:
            raise KeyError(f'PathIntegral.grow: no parameter {name!r}')
        i = self.names.index(name)
        if old_param is not None and tuple(old_param.shape) != self.shapes[i]:
            raise ValueError(f'PathIntegral.grow: {name}: old_param has shape {tuple(old_param.shape)}, expected {self.shapes[i]}')
        self.flat, self.omega, self.shapes, self.start = _grown('PathIntegral', self.names, self.shapes, self.omega, self.start, name, new_param)
        if old_param is not None:      # what the growth itself did to the old rows is no step of the path: start moves with them
            rows = old_param.shape[0]
            self.start[i][:rows] += new_param.detach()[:rows].float() - old_param.detach().float()
        return self

    # ---- checkpoints ------------------------------------------------------------------------------------------------
    def state_dict(self):
        """Tensors by parameter NAME (views of this object's buffers: clone or copy them to keep them), and xi."""
        return {'omega': dict(zip(self.names, self.omega)), 'start': dict(zip(self.names, self.start)), 'xi': self.xi}

    @torch.no_grad()
    def load_state_dict(self, state):
        for kind in ('omega', 'start'):
            if set(state[kind]) != set(self.names):
                missing, extra = sorted(set(self.names) - set(state[kind])), sorted(set(state[kind]) - set(self.names))
                raise KeyError(f'PathIntegral.load_state_dict: {kind}: missing {missing}, unexpected {extra}')
        for n, w, s in zip(self.names, self.omega, self.start):
            for kind, dst in (('omega', w), ('start', s)):
                if tuple(state[kind][n].shape) != tuple(dst.shape):
                    raise ValueError(f'PathIntegral.load_state_dict: {kind} of {n} has shape {tuple(state[kind][n].shape)}, '
                                     f'expected {tuple(dst.shape)}')
        for n, w, s in zip(self.names, self.omega, self.start):
            w.copy_(state['omega'][n])
            s.copy_(state['start'][n])
        self.xi = float(state['xi'])
        return self
