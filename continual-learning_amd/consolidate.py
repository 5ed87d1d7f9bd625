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
are uncorrelated.  Labels sampled from the model's own softmax ("true" Fisher), MAS and Synaptic Intelligence are not provided.
"""
import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from ._lib import ptr

_ROW_DT = np.dtype([('dst', 'u8'), ('src', 'u8'), ('n', 'i8')])


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
        sizes = [p.numel() for _, p in named]
        self.flat = torch.zeros(sum(sizes), dtype=torch.float32, device=self.device)
        self.importance, off = [], 0
        for k, shape in zip(sizes, self.shapes):
            self.importance.append(self.flat[off:off + k].view(shape))
            off += k
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
        if name not in self.names:
            raise KeyError(f'Consolidation.grow: no parameter {name!r}')
        i = self.names.index(name)
        old, new = self.shapes[i], tuple(new_param.shape)
        if len(new) != len(old) or len(old) < 1 or new[0] <= old[0] or new[1:] != old[1:]:
            raise ValueError(f'Consolidation.grow: {name}: {old} -> {new} is not growth along dim 0')
        shapes = list(self.shapes)
        shapes[i] = new
        sizes = [int(np.prod(sh)) for sh in shapes]
        flat = torch.zeros(sum(sizes), dtype=torch.float32, device=self.device)
        views, off = [], 0
        for j, (k, shape) in enumerate(zip(sizes, shapes)):
            w = flat[off:off + k].view(shape)
            w[:self.shapes[j][0]].copy_(self.importance[j])
            views.append(w)
            off += k
        anchor = new_param.detach().clone().float().contiguous().to(self.device)
        anchor[:old[0]].copy_(self.anchor[i])
        self.flat, self.importance, self.shapes = flat, views, shapes
        self.anchor[i] = anchor
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
