"""Fused multi-tensor optimisers on libclamd (csrc/optim.hip): one launch for all 82 parameter tensors.

``FusedAdam(params, lr, betas)`` mirrors ``torch.optim.Adam`` as the reference constructs it (trainer.py:108-110:
weight_decay 0, amsgrad off, eps 1e-8) including the ``state_dict()`` layout ('step', 'exp_avg', 'exp_avg_sq' per
parameter, positional param ids), so optimiser checkpoints are interchangeable (trainer.py:76,95).
Hyper-parameters, the step counter and the bias corrections live in device memory: a captured HIP graph of the step
can be replayed while a scheduler (trainer.py:111-112,147) changes ``param_groups[0]['lr']``.

Optional L2-to-old-weights regulariser (build-defined): ``set_l2_anchor(old_params, lam)`` adds
2*lam*(theta - theta_old) to every gradient inside the same kernel.

Optional elastic weight consolidation (build-defined as well): ``set_consolidation(old_params, importance, lam)`` adds
lam*omega*(theta - theta_old); such a step runs ``clamd_adam_step_consolidated`` (36 B / parameter), every other step
``clamd_adam_step``.

Optional path integral of Synaptic Intelligence (build-defined too): ``set_path_integral(omega)`` makes every step also accumulate
omega += -(grad * grad_scale) * (theta_new - theta_old) inside the same kernel (``clamd_adam_step_tracked`` / ``clamd_sgd_step_tracked``,
+8 B / parameter); without it the step launches what it always did.

Optional clipping by the global gradient norm: ``set_grad_clip(max_norm)`` puts one norm pass (``clamd_grad_norm_clip``, 4 B / parameter) in
front of the step and hands the coefficient to the unchanged step kernel through the gradient scale; nothing is read back.

``FusedSGD`` is the second optimiser: torch.optim.SGD with momentum, Nesterov and weight decay in one launch of ``clamd_sgd_step``.  Both
are a ``_FusedOptimizer``, which owns everything they do alike: the step protocol, the device tables, the two anchor terms, head growth
and checkpoints.  A subclass says how one table row is filled, which eight hyper-parameters it uploads, how its state is laid out in flat
buffers and grows, and which entry point it launches.
"""
import numpy as np
import torch

from . import _lib
from ._lib import ptr


_GRAD_TENSOR_DT = np.dtype([('g', 'u8'), ('n', 'i8'), ('first_chunk', 'i4'), ('nchunks', 'i4')])      # clamd_grad_norm_clip's rows


class _FusedOptimizer(torch.optim.Optimizer):
    """One parameter group of contiguous fp32 GPU tensors behind one device table (rows of _ROW_DT, checked against the library's
    _SIZEOF()).  The two build-defined pulls towards an anchor (one anchor pointer per tensor serves both) live here: the L2-to-old-weights
    term and elastic weight consolidation."""

    def __init__(self, params, defaults, grad_scale):
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError(f'{self._NAME} supports a single parameter group ({self._ONE_GROUP})')
        self.grad_scale = grad_scale
        self.pre_step_hooks = []      # e.g. ddp.GradSync.wait
        self._table = None
        self._hyper_host = None
        self._state_dev = None        # device of the flat state buffers; None: they are laid out (again) at the next step
        self._l2_lambda = 0.0
        self._anchor = None
        self._l2_on = False           # the anchor serves the L2 term, the consolidation term, or both
        self._l2acc = None            # [0] = sum ||theta - theta_old||^2 of the last step, [1..] = per-workgroup partials
        self._importance = None
        self._ewc_lambda = 0.0
        self._ewcacc = None
        self._path = None             # per-parameter path integrals (Synaptic Intelligence): the step launches the tracked entry point
        self._path_dev = None
        self._clip = None             # max_norm of clipping by the global gradient norm; None: off, nothing below is allocated
        self._clip_tab = self._clip_part = self._clip_out = self._hyper_eff = self._tensor_norms = None

    # -- the step ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        for h in self.pre_step_hooks:
            h()
        params = self.param_groups[0]['params']
        key = []
        for p in params:
            gr = p.grad
            if gr is None:
                raise RuntimeError(f'{self._NAME}: every parameter must have a gradient (the UNet backward produces all of them)')
            key.append((p.data_ptr(), gr.data_ptr()))
        if self._table != key:       # first step, or parameters / gradients moved: validate and rebuild the device table
            for p in params:
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() or not p.grad.is_contiguous():
                    raise RuntimeError(f'{self._NAME} needs contiguous fp32 GPU parameters and gradients: there is no CPU fallback')
            dev = params[0].device
            if self._state_dev != dev:
                self._hyper = torch.zeros(8, dtype=torch.float32, device=dev)
                self._hyper_host = None       # a new device buffer: sync_hyper uploads again
                self._init_state(params, dev)
                self._state_dev = dev
            self._build_table(params, dev)
            self._table = key
        self.sync_hyper()
        if self._clip is not None:
            from . import unet as U
            U._hbm('clip', 4 * self._numel,       # every gradient read once
                   'clamd_grad_norm_clip', ptr(self._clip_tab), len(params), ptr(self._chunks_dev), self._nchunks, ptr(self._hyper), self._clip,
                   ptr(self._clip_part), ptr(self._clip_out), ptr(self._tensor_norms), ptr(self._hyper_eff), _lib.stream_ptr())
        self._launch()
        return loss

    def _build_table(self, params, dev):
        rows = [self._row(p, self._anchor[i].data_ptr() if self._anchor is not None else 0) for i, p in enumerate(params)]
        numels = [p.numel() for p in params]
        self._tensors_dev, self._chunks_dev, self._nchunks = _lib.job_table(self._ROW_DT, rows, numels, dev, self._SIZEOF)
        self._numel = int(sum(numels))
        self._l2acc = torch.zeros(1 + self._nchunks, dtype=torch.float32, device=dev)
        self._ewcacc = self._importance_dev = None
        if self._importance is not None:
            self._importance_dev = torch.tensor([w.data_ptr() for w in self._importance], dtype=torch.int64).to(dev)
            self._ewcacc = torch.zeros(1 + self._nchunks, dtype=torch.float32, device=dev)
        self._path_dev = None
        if self._path is not None:
            for i, (p, w) in enumerate(zip(params, self._path)):
                if w.device != p.device:
                    raise RuntimeError(f'{self._NAME}: path integral {i} is on {w.device}, its parameter on {p.device}')
            self._path_dev = torch.tensor([w.data_ptr() for w in self._path], dtype=torch.int64).to(dev)
        self._clip_tab = self._clip_part = self._tensor_norms = None
        if self._clip is not None:
            lib = _lib.load()
            assert lib.clamd_sizeof_grad_tensor() == _GRAD_TENSOR_DT.itemsize
            chunk = lib.clamd_adam_chunk_elems()
            counts = [(n + chunk - 1) // chunk for n in numels]          # a row's jobs are consecutive in job_table's list
            firsts = np.cumsum([0] + counts)
            assert int(firsts[-1]) == self._nchunks
            table = np.array([(p.grad.data_ptr(), n, int(f), k) for p, n, f, k in zip(params, numels, firsts, counts)], dtype=_GRAD_TENSOR_DT)
            self._clip_tab = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
            self._clip_part = torch.zeros(self._nchunks, dtype=torch.float32, device=dev)
            self._tensor_norms = torch.zeros(len(params), dtype=torch.float32, device=dev)
            if self._clip_out is None or self._clip_out.device != dev:     # kept across rebuilds: a caller may hold the views below
                self._clip_out = torch.zeros(4, dtype=torch.float32, device=dev)
                self._hyper_eff = torch.zeros(8, dtype=torch.float32, device=dev)

    def _step_hyper(self):
        """The hyper buffer the step kernel reads: with clipping the copy whose gradient scale carries the coefficient."""
        return self._hyper if self._clip is None else self._hyper_eff

    def sync_hyper(self):
        """Upload the eight hyper-parameters (learning rate, ..., gradient scale, L2 and consolidation weights) to device memory if they
        changed on the host (LambdaLR writes param_groups[0]['lr']).  step() calls this; a replayed HIP graph of the step
        (tools/graphed_step.py) calls it before every replay, because the captured kernel reads the values from that device buffer."""
        hyper = self._hyper_tuple(self.param_groups[0]) + (float(self.grad_scale), float(self._l2_lambda), float(self._ewc_lambda), 0.0)
        if hyper != self._hyper_host:
            self._hyper.copy_(torch.tensor(hyper, dtype=torch.float32))
            self._hyper_host = hyper

    def note_replayed_step(self, n=1):
        """FusedAdam mirrors its device step counter here; nothing to do without one."""

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._table = None            # the restored state is re-homed into the flat buffers at the next step
        self._hyper_host = None
        self._state_dev = None

    # -- class-incremental head growth ---------------------------------------------------------------------
    @staticmethod
    def _grown(old, new_shape, fill):
        """`old` with rows appended along dim 0 up to new_shape; the new rows take `fill`'s (None: zero)."""
        out = torch.zeros(new_shape, dtype=old.dtype, device=old.device)
        out[:old.shape[0]].copy_(old)
        if fill is not None:
            out[old.shape[0]:].copy_(fill[old.shape[0]:])
        return out

    @torch.no_grad()
    def replace_params(self, mapping):
        """Class-incremental head growth (UNet.expand_classes): swaps parameter objects inside the group and re-homes their state.
        mapping: {old_param: new_param}; new_param has more rows along dim 0 and the same trailing shape (anything else: ValueError).
        The state of the leading rows is kept, the new rows start at zero, a shared step counter stays.  The L2 / consolidation anchor of
        the new rows is their current (initial) value and their importance zero: nothing pulls on classes the finished task never had.
        The importance list is replaced (grown copies); a Consolidation re-installs its own views after Consolidation.grow.  The path
        integrals grow the same way (old rows kept, new rows zero); a PathIntegral re-installs its views after PathIntegral.grow.  Flat state
        and device tables are laid out again at the next step."""
        params = self.param_groups[0]['params']
        index = {id(p): i for i, p in enumerate(params)}
        todo = []
        for old, new in mapping.items():
            if id(old) not in index:
                raise ValueError(f'{self._NAME}.replace_params: a key of the mapping is not a parameter of this optimiser')
            if old.dim() != new.dim() or old.dim() < 1 or new.shape[0] <= old.shape[0] or new.shape[1:] != old.shape[1:]:
                raise ValueError(f'{self._NAME}.replace_params: {tuple(old.shape)} -> {tuple(new.shape)} is not growth along dim 0')
            if new.device != old.device or new.dtype != old.dtype:
                raise ValueError(f'{self._NAME}.replace_params: the new parameter must keep the device and dtype')
            todo.append((index[id(old)], old, new))
        states = [self.state.get(p) for p in params]
        for i, old, new in todo:
            if states[i]:
                states[i] = self._grow_state(states[i], new.shape)
            if self._anchor is not None:
                self._anchor[i] = self._grown(self._anchor[i], new.shape, new.detach().float())
            if self._importance is not None:
                self._importance[i] = self._grown(self._importance[i], new.shape, None)
            if self._path is not None:
                self._path[i] = self._grown(self._path[i], new.shape, None)
            self.state.pop(old, None)
            params[i] = new
        for p, st in zip(params, states):
            if st:
                self.state[p] = self._rekeyed_state(st)
        self._state_dev = None
        self._table = None

    def _rekeyed_state(self, st):
        return dict(st)

    # -- the two anchor terms ------------------------------------------------------------------------------
    def set_l2_anchor(self, old_params, lam):
        """old_params: list of tensors aligned with this optimiser's parameters (a frozen task-1 snapshot).  With a consolidation set the
        anchor is shared (one pointer per tensor in the device table): it has to be the same snapshot."""
        anchor = [o.detach().contiguous().float() for o in old_params] if old_params is not None else None
        if anchor is not None and self._importance is not None:
            self._same_anchor(anchor)
        elif self._importance is None:
            self._anchor = anchor
        self._l2_on = anchor is not None
        self._l2_lambda = float(lam) if anchor is not None else 0.0
        self._table = None
        self._hyper_host = None

    def _same_anchor(self, anchor):
        """Setup-time check (compares on the device, so it synchronises; never on the step path)."""
        if len(anchor) != len(self._anchor) or not all(a.shape == b.shape and a.device == b.device and
                                                       (a.data_ptr() == b.data_ptr() or torch.equal(a, b))
                                                       for a, b in zip(anchor, self._anchor)):
            raise ValueError(f'{self._NAME}: the L2 anchor and the consolidation anchor must be the same snapshot (one anchor per tensor)')

    @property
    def l2_lambda(self):
        """Weight of the L2-to-old-weights term (0 when it is off)."""
        return self._l2_lambda if self._l2_on else 0.0

    def l2_penalty(self):
        """lam * sum ||theta - theta_old||^2 as accumulated by the LAST step (device scalar)."""
        return self._l2acc[:1] * self._l2_lambda

    def set_consolidation(self, old_params, importance, lam):
        """Elastic weight consolidation: every step adds lam * importance * (theta - old) to the gradient inside the optimiser's kernel.
        old_params / importance: lists of tensors aligned with this optimiser's parameters (same shapes, on the parameters' device; the
        importance fp32 and contiguous -- it is read in place, so a consolidate.Consolidation can update it between steps).
        importance >= 0 is the caller's contract: it is not checked (that would synchronise).  old_params None clears the term."""
        if old_params is None:
            self._importance, self._ewc_lambda = None, 0.0
            if not self._l2_on:
                self._anchor = None
            self._table = None
            self._hyper_host = None
            return
        params = self.param_groups[0]['params']
        old_params, importance = list(old_params), list(importance)
        if len(old_params) != len(params) or len(importance) != len(params):
            raise ValueError(f'{self._NAME}.set_consolidation: {len(params)} parameters, {len(old_params)} anchors, {len(importance)} importance tensors')
        for i, (p, o, w) in enumerate(zip(params, old_params, importance)):
            if o.shape != p.shape or w.shape != p.shape:
                raise ValueError(f'{self._NAME}.set_consolidation: parameter {i} has shape {tuple(p.shape)}, anchor {tuple(o.shape)}, '
                                 f'importance {tuple(w.shape)}')
            if w.dtype != torch.float32 or not w.is_contiguous():
                raise ValueError(f'{self._NAME}.set_consolidation: importance {i} must be contiguous fp32')
            if o.device != p.device or w.device != p.device:
                raise ValueError(f'{self._NAME}.set_consolidation: parameter {i} is on {p.device}, anchor on {o.device}, importance on {w.device}')
        if not float(lam) >= 0.0:
            raise ValueError(f'{self._NAME}.set_consolidation: lam must be >= 0')
        anchor = [o.detach().contiguous().float() for o in old_params]
        if self._l2_on:
            self._same_anchor(anchor)         # the L2 anchor stays: one pointer per tensor serves both terms
        else:
            self._anchor = anchor
        self._importance = [w.detach() for w in importance]
        self._ewc_lambda = float(lam)
        self._table = None
        self._hyper_host = None

    # -- the path integral (Synaptic Intelligence) -----------------------------------------------------------
    def set_path_integral(self, omega):
        """Synaptic Intelligence (Zenke et al. 2017): every step also does omega += -(grad * grad_scale) * (theta_new - theta_old) inside
        the optimiser's kernel, with the gradient as it is handed over (before weight decay and both pulls) -- +8 B / parameter.
        omega: list of contiguous fp32 tensors aligned with this optimiser's parameters (same shapes, on their device), written in place: a
        consolidate.PathIntegral owns them.  None switches tracking off: the step then launches exactly what it launched before.  omega
        is not optimiser state (state_dict() is unchanged); it composes with set_l2_anchor and set_consolidation in any order."""
        if omega is None:
            self._path = None
            self._table = None
            return
        params = self.param_groups[0]['params']
        omega = list(omega)
        if len(omega) != len(params):
            raise ValueError(f'{self._NAME}.set_path_integral: {len(params)} parameters, {len(omega)} path tensors')
        for i, (p, w) in enumerate(zip(params, omega)):
            if w.shape != p.shape:
                raise ValueError(f'{self._NAME}.set_path_integral: parameter {i} has shape {tuple(p.shape)}, path {tuple(w.shape)}')
            if w.dtype != torch.float32 or not w.is_contiguous():
                raise ValueError(f'{self._NAME}.set_path_integral: path {i} must be contiguous fp32')
            if w.device != p.device:
                raise ValueError(f'{self._NAME}.set_path_integral: parameter {i} is on {p.device}, path on {w.device}')
        self._path = [w.detach() for w in omega]
        self._table = None

    # -- clipping by the global gradient norm -------------------------------------------------------------------
    def set_grad_clip(self, max_norm):
        """torch.nn.utils.clip_grad_norm_(parameters, max_norm) inside the step, without rewriting a gradient: after the hooks and
        sync_hyper, one pass reads every gradient once (``clamd_grad_norm_clip``, 4 B / parameter), a finalize kernel forms
        coef = min(1, max_norm / (norm + 1e-6)) on the device, and the unchanged step kernel runs on a second hyper buffer whose gradient
        scale is grad_scale * coef.  Nothing is read back; the step stays bit-reproducible and can be captured in a graph (which keeps the
        max_norm it was captured with).  max_norm: > 0; float('inf') measures without clipping (coef == 1 exactly); None switches clipping
        off: the step then launches exactly what it launched before and nothing is allocated.
        - The norm is that of the gradient the step consumes: after grad_scale, i.e. after DDP's 1/world (ddp.GradSync).  Every rank computes
          it from identical all-reduced gradients (GradSync.wait is a pre_step_hook and has run), so no further collective is needed.
        - Weight decay and the L2 / consolidation pulls are added after clipping, as torch.optim does with weight decay.
        - The path integral (set_path_integral) sees the clipped gradient, as it would after an in-place clip_grad_norm_.
        - A non-finite norm propagates as in torch with error_if_nonfinite=False (a NaN norm gives a NaN coefficient and NaN parameters; an
          infinite one coefficient 0) and sets ``grad_nonfinite``.
        Device tensors of the LAST step while clipping is on: ``grad_norm``, ``clip_coef``, ``effective_grad_scale``, ``grad_nonfinite``
        (fp32[1] each) and ``tensor_grad_norms`` (fp32[ntensors], parameter order)."""
        if max_norm is not None:
            max_norm = float(max_norm)
            if not max_norm > 0.0:
                raise ValueError(f'{self._NAME}.set_grad_clip: max_norm must be > 0 (inf: measure only; None: off), not {max_norm}')
        self._clip = max_norm
        if max_norm is None:
            self._clip_tab = self._clip_part = self._clip_out = self._hyper_eff = self._tensor_norms = None
        self._table = None

    def _clip_stat(self, i):
        if self._clip is None or self._clip_out is None:
            raise RuntimeError(f'{self._NAME}: no step with gradient clipping has run (set_grad_clip)')
        return self._clip_out[i if isinstance(i, slice) else slice(i, i + 1)]

    @property
    def clip_state(self):
        """The four below in one device tensor, fp32[4]: norm, coefficient, effective gradient scale, non-finite flag."""
        return self._clip_stat(slice(0, 4))

    @property
    def grad_norm(self):
        """Global norm of the gradient the last step consumed, grad_scale included (device fp32[1])."""
        return self._clip_stat(0)

    @property
    def clip_coef(self):
        """min(1, max_norm / (grad_norm + 1e-6)) of the last step (device fp32[1])."""
        return self._clip_stat(1)

    @property
    def effective_grad_scale(self):
        """fp32(grad_scale) * clip_coef: the gradient scale the last step's kernel read (device fp32[1])."""
        return self._clip_stat(2)

    @property
    def grad_nonfinite(self):
        """1 when the last step's norm was infinite or NaN, else 0 (device fp32[1])."""
        return self._clip_stat(3)

    @property
    def tensor_grad_norms(self):
        """Per-parameter norms of the last step, grad_scale included, in parameter order (device fp32[ntensors])."""
        self._clip_stat(0)
        return self._tensor_norms

    def consolidation_penalty(self):
        """(lam / 2) * sum importance * (theta - theta_old)^2 as accumulated by the LAST step (device scalar)."""
        if self._ewcacc is None:
            raise RuntimeError(f'{self._NAME}.consolidation_penalty: no step with a consolidation has run')
        return self._ewcacc[:1] * (0.5 * self._ewc_lambda)


class FusedAdam(_FusedOptimizer):
    _NAME = 'FusedAdam'
    _ONE_GROUP = 'as trainer.py:108 builds'
    _ROW_DT = np.dtype([('p', 'u8'), ('g', 'u8'), ('m', 'u8'), ('v', 'u8'), ('old', 'u8'), ('n', 'i8')])
    _SIZEOF = 'clamd_sizeof_adam_tensor'

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0):
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None)
        super().__init__(params, defaults, grad_scale)

    def _init_state(self, params, dev):
        """Lays exp_avg / exp_avg_sq out in two flat buffers and re-homes what load_state_dict or replace_params left in self.state."""
        n = sum(p.numel() for p in params)
        prev = [self.state.get(p) for p in params]
        self._m = torch.zeros(n, dtype=torch.float32, device=dev)
        self._v = torch.zeros(n, dtype=torch.float32, device=dev)
        self._step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self._derived = torch.zeros(2, dtype=torch.float32, device=dev)
        off, steps0 = 0, set()
        self._step_host = torch.tensor(0.0)          # ONE host-side step counter shared by every parameter's state
        for p, st in zip(params, prev):
            k = p.numel()
            m, v = self._m[off:off + k].view_as(p), self._v[off:off + k].view_as(p)
            step0 = 0.0
            if st:     # state restored by load_state_dict before the first step
                m.copy_(st['exp_avg'])
                v.copy_(st['exp_avg_sq'])
                step0 = float(st['step'])
            self.state[p] = {'step': self._step_host, 'exp_avg': m, 'exp_avg_sq': v}
            steps0.add(step0)
            off += k
        if len(steps0) != 1:
            raise ValueError('FusedAdam needs one common step count across parameters')
        self._step_host.fill_(steps0.pop())
        self._step_dev.fill_(int(self._step_host))

    def _row(self, p, old):
        st = self.state[p]
        return (p.data_ptr(), p.grad.data_ptr(), st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr(), old, p.numel())

    def _hyper_tuple(self, group):
        return (float(group['lr']), float(group['betas'][0]), float(group['betas'][1]), float(group['eps']))

    def _grow_state(self, st, shape):
        return {'step': st['step'], 'exp_avg': self._grown(st['exp_avg'], shape, None), 'exp_avg_sq': self._grown(st['exp_avg_sq'], shape, None)}

    def _rekeyed_state(self, st):
        return dict(st, step=torch.tensor(float(self._step_host))) if hasattr(self, '_step_host') else dict(st)

    def note_replayed_step(self, n=1):
        """Host-side mirror of the device step counter after a graph replay executed the Adam kernel (n = -1 after the
        capture itself, which runs step() on the host without executing anything)."""
        self._step_host += n

    def _launch(self):
        from . import unet as U
        l2acc = ptr(self._l2acc) if self._l2_on else None
        ewc = self._importance is not None
        if self._path is not None:
            # the plain step's 28 B, the path integral read and written, the anchor and the importance read
            U._hbm('adam', (36 + (8 if ewc else 4 if self._anchor is not None else 0)) * self._numel,
                   'clamd_adam_step_tracked', ptr(self._tensors_dev), ptr(self._importance_dev) if ewc else None, ptr(self._path_dev),
                   ptr(self._chunks_dev), self._nchunks, ptr(self._step_hyper()), ptr(self._step_dev), ptr(self._derived),
                   ptr(self._ewcacc) if ewc else None, l2acc, _lib.stream_ptr())
        elif ewc:
            U._hbm('adam', 36 * self._numel,      # p, g, m, v, old, importance read; p, m, v written
                   'clamd_adam_step_consolidated', ptr(self._tensors_dev), ptr(self._importance_dev), ptr(self._chunks_dev), self._nchunks,
                   ptr(self._step_hyper()), ptr(self._step_dev), ptr(self._derived), ptr(self._ewcacc), l2acc, _lib.stream_ptr())
        else:
            U._hbm('adam', 28 * self._numel,      # p, g, m, v read; p, m, v written
                   'clamd_adam_step', ptr(self._tensors_dev), ptr(self._chunks_dev), self._nchunks, ptr(self._step_hyper()),
                   ptr(self._step_dev), ptr(self._derived), l2acc, _lib.stream_ptr())
        self._step_host += 1                # host-side mirror of the device counter (shared by all param states)


_SGD_TENSOR_DT = np.dtype([('p', 'u8'), ('g', 'u8'), ('buf', 'u8'), ('old', 'u8'), ('n', 'i8'), ('decay_mult', 'f4'), ('pad', 'f4')])


class FusedSGD(_FusedOptimizer):
    """Fused multi-tensor SGD with momentum, Nesterov and weight decay: ``torch.optim.SGD`` semantics (dampening 0, maximize off) in one
    launch of ``clamd_sgd_step`` over all parameters, with the same surface as FusedAdam (grad_scale, pre_step_hooks, sync_hyper,
    set_l2_anchor, set_consolidation, replace_params), so the trainer, ddp.GradSync and Consolidation work with either.

    One parameter group.  ``state[p] == {'momentum_buffer': view into one flat buffer}`` with momentum > 0, no state without; the
    ``state_dict()`` layout is torch.optim.SGD's, so optimiser checkpoints are interchangeable in both directions.  ``no_decay``: parameters
    of this optimiser whose weight decay is switched off (BatchNorm weights and biases) without a second group.  Hyper-parameters live in
    device memory (a replayed graph sees a new learning rate); per element, in this order:
        g = grad * grad_scale;  g += weight_decay * decay_mult * p;  d = p - old;  g += 2 * l2_lambda * d;  g += ewc_lambda * omega * d
        buf = momentum * buf + g;  p -= lr * (nesterov ? g + momentum * buf : buf)
    """
    _NAME = 'FusedSGD'
    _ONE_GROUP = 'the anchor and importance lists follow model.parameters()'
    _ROW_DT = _SGD_TENSOR_DT
    _SIZEOF = 'clamd_sizeof_sgd_tensor'

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, no_decay=(), grad_scale=1.0):
        if not lr >= 0.0:
            raise ValueError(f'FusedSGD: invalid learning rate {lr}')
        if not momentum >= 0.0:
            raise ValueError(f'FusedSGD: invalid momentum {momentum}')
        if not weight_decay >= 0.0:
            raise ValueError(f'FusedSGD: invalid weight_decay {weight_decay}')
        if dampening != 0:
            raise ValueError('FusedSGD: dampening is not supported (it must be 0)')
        if nesterov and momentum <= 0:
            raise ValueError('FusedSGD: Nesterov momentum requires a momentum and zero dampening')
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, maximize=False,
                        foreach=None, differentiable=False, fused=None)
        super().__init__(params, defaults, grad_scale)
        own = {id(p) for p in self.param_groups[0]['params']}
        self._no_decay = set()
        for p in no_decay:
            if id(p) not in own:
                raise ValueError('FusedSGD: a tensor of no_decay is not a parameter of this optimiser')
            self._no_decay.add(id(p))

    def _init_state(self, params, dev):
        """Lays the momentum buffers out in one flat buffer (each tensor's slice starts on 16 bytes, as the parameters themselves do; the
        kernel does not depend on it) and re-homes what load_state_dict or replace_params left in self.state."""
        prev = [self.state.get(p) for p in params]
        self._with_momentum = float(self.param_groups[0]['momentum']) > 0
        self._flat = None
        for p in params:
            self.state.pop(p, None)   # momentum 0: no state (a restored {'momentum_buffer': None} goes too)
        if not self._with_momentum:
            return
        self._flat = torch.zeros(sum((p.numel() + 3) // 4 * 4 for p in params), dtype=torch.float32, device=dev)
        off = 0
        for p, st in zip(params, prev):
            buf = self._flat[off:off + p.numel()].view_as(p)
            if st and st.get('momentum_buffer') is not None:      # absent or None: torch before its first step, starts at zero
                buf.copy_(st['momentum_buffer'])
            self.state[p] = {'momentum_buffer': buf}
            off += (p.numel() + 3) // 4 * 4

    def _row(self, p, old):
        buf = self.state[p]['momentum_buffer'].data_ptr() if self._with_momentum else 0
        return (p.data_ptr(), p.grad.data_ptr(), buf, old, p.numel(), 0.0 if id(p) in self._no_decay else 1.0, 0.0)

    def _hyper_tuple(self, group):
        if group['dampening'] != 0 or group['maximize']:
            raise ValueError('FusedSGD: dampening and maximize are not supported')
        return (float(group['lr']), float(group['momentum']), float(group['weight_decay']), 1.0 if group['nesterov'] else 0.0)

    def _grow_state(self, st, shape):
        if st.get('momentum_buffer') is None:
            return st
        return {'momentum_buffer': self._grown(st['momentum_buffer'], shape, None)}

    @torch.no_grad()
    def replace_params(self, mapping):
        """As _FusedOptimizer.replace_params; a no_decay flag follows the swapped parameter."""
        super().replace_params(mapping)
        for old, new in mapping.items():
            if id(old) in self._no_decay:
                self._no_decay.discard(id(old))
                self._no_decay.add(id(new))

    def _launch(self):
        from . import unet as U
        ewc = self._importance is not None
        # p, g read and p written; buf read and written; the anchor and the importance read
        per_param = 12 + (8 if self._with_momentum else 0) + (4 if self._anchor is not None else 0) + (4 if ewc else 0)
        tail = (ptr(self._chunks_dev), self._nchunks, ptr(self._step_hyper()), ptr(self._ewcacc) if ewc else None,
                ptr(self._l2acc) if self._l2_on else None, _lib.stream_ptr())
        if self._path is not None:      # the path integral read and written on top
            U._hbm('sgd', (per_param + 8) * self._numel, 'clamd_sgd_step_tracked', ptr(self._tensors_dev),
                   ptr(self._importance_dev) if ewc else None, ptr(self._path_dev), *tail)
        else:
            U._hbm('sgd', per_param * self._numel, 'clamd_sgd_step', ptr(self._tensors_dev), ptr(self._importance_dev) if ewc else None, *tail)
