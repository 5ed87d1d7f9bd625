"""Trainer counterpart for the hot loop of the reference (trainer.py:105-129 build_model, :132-265 train_val).

Same construction and ordering as the reference:
  model  = UNet(num_classes, in_dim=3, conv_dim=64)                       trainer.py:107 (num_classes is a knob here, Q8)
  optim  = Adam(model.parameters(), lr, betas=[beta1, beta2])             trainer.py:108-110 -> FusedAdam
           (cfg.optimizer='sgd', build-defined: FusedSGD with cfg.momentum, nesterov, weight_decay; cfg.lr_schedule='iteration': the
            polynomial decay stepped after every optimiser step over cfg.max_iters instead of once per epoch)
  sched  = LambdaLR(optim, lambda n: (1 - n/n_iters) ** lr_exp)           trainer.py:111-112
  c_loss = CrossEntropyLoss()                                             trainer.py:113
  per epoch: scheduler.step() FIRST (trainer.py:147), then for each batch
      outputs = model(inputs); zero_grad(); loss = c_loss(outputs, labels); loss.backward(); optim.step()   :172-176
Out of scope here: JPEG dumps, prints, checkpoint files; the every-10th-iteration statistics
(trainer.py:177-189) are computed on the GPU by metrics.argmax_confusion instead of .cpu() round trips.
Continual learning (config 4): ``begin_task2(c_old, ...)`` snapshots the model and switches the criterion to
DistillationCrossEntropy and/or enables the L2-to-old-weights term (both build-defined); ``freeze_bn=True`` also trains task 2 with
every BatchNorm in eval mode (running statistics, not updated); ``ewc_lambda > 0`` estimates the finished task's per-parameter importance
(``estimate_importance``) and enables elastic weight consolidation inside the Adam kernel (build-defined too, consolidate.py);
``cfg.path_integral=True`` tracks Synaptic Intelligence's path integral inside every optimiser step from the first one
(consolidate.PathIntegral, ``self.path``) and ``begin_task2(si_lambda=c)`` consolidates with it instead of the Fisher estimate.
Data parallel: ``sync_bn=True`` converts the model's BatchNorm layers to nn.SyncBatchNorm when a process group is initialised (statistics
of the global batch, syncbn.py).  ``begin_task2(pseudo_label=True)`` relabels the background of the new task's batches with the old model's
confident predictions (build-defined, pseudo.py); ``begin_task2(pod_lambda=...)`` adds Local POD distillation of the logits (build-defined,
pod.py); ``begin_task2(replay=M, replay_batch=R)`` keeps M exemplars of the finished task in an on-device memory and mixes R of them into
every batch (build-defined, replay.py).  ``cfg.augment=True`` (with augment_scale, augment_flip, augment_seed) rescales, crops or pads and
flips every training batch -- the replayed rows included -- in one launch before the forward pass (build-defined, augment.py); off by
default, and then nothing on the step's path changes.  ``cfg.loss='ce_dice'`` (build-defined, loss.DiceCrossEntropyLoss with dice_weight,
dice_smooth, dice_include_background, dice_present_only, dice_per_image) makes the step's criterion cross-entropy + soft Dice; the default
'ce' changes nothing.  ``begin_task2(pod_lambda=...)`` adds on top of it; not with distill_lambda > 0, unbiased=True or pseudo_adaptive=True
(those criteria have no Dice term, this one no per-image weight).  ``estimate_importance`` keeps differentiating the plain log-likelihood.
Data parallel: each rank's Dice sums cover its own batch, like non-synchronised BatchNorm; no collective is added.
"""
import os
import warnings
from types import SimpleNamespace

import torch
import torch.nn as nn
from torch.optim.lr_scheduler import LambdaLR

from .loss import CrossEntropyLoss, DiceCrossEntropyLoss, DistillationCrossEntropy, UnbiasedDistillationCrossEntropy
from .metrics import argmax_confusion, metrics_from_confusion
from .optim import FusedAdam, FusedSGD
from .consolidate import Consolidation, PathIntegral
from .pseudo import PseudoLabeler
from .pod import LocalPODLoss
from .replay import ReplayMemory
from .augment import RandomScaleCrop
from . import syncbn
from .unet import UNet


def default_config(**kw):
    """Defaults of main.py:64-105 for the flags the hot path reads."""
    cfg = dict(n_iters=10000, train_batch_size=2, lr=1e-4, lr_exp=0.9, beta1=0.5, beta2=0.99, h_image_size=512,
               w_image_size=256, num_classes=21, conv_dim=64, compute_dtype='fp32', stats_every=10, sync_bn=False,
               augment=False, augment_scale=(0.5, 2.0), augment_flip=True, augment_seed=0,
               optimizer='adam', momentum=0.9, nesterov=True, weight_decay=1e-4, decay_norm_and_bias=True, lr_schedule='epoch',
               max_iters=None, path_integral=False, si_xi=0.1,
               loss='ce', dice_weight=1.0, dice_smooth=1e-5, dice_include_background=True, dice_present_only=True, dice_per_image=False)
    cfg.update(kw)
    return SimpleNamespace(**cfg)


def make_scheduler(optim, cfg, iters_per_epoch=None):
    """The learning-rate schedule of cfg.lr_schedule on any optimiser.  'epoch' (the default, the reference's trainer.py:111-112):
    (1 - n/n_iters) ** lr_exp, stepped once at the start of every epoch.  'iteration' (build-defined, what the class-incremental
    segmentation papers train with): max(0, 1 - n/max_iters) ** lr_exp, stepped after every optimiser step; cfg.max_iters None means
    n_iters * iters_per_epoch."""
    kind = getattr(cfg, 'lr_schedule', 'epoch')
    if kind == 'epoch':
        return LambdaLR(optim, lr_lambda=lambda n: (1 - n / cfg.n_iters) ** cfg.lr_exp)
    if kind != 'iteration':
        raise ValueError(f"lr_schedule must be 'epoch' or 'iteration', not {kind!r}")
    max_iters = getattr(cfg, 'max_iters', None)
    if max_iters is None:
        if iters_per_epoch is None:
            raise ValueError("lr_schedule='iteration' needs max_iters or a loader with a length")
        max_iters = cfg.n_iters * iters_per_epoch
    if not max_iters > 0:
        raise ValueError('max_iters must be > 0')
    return LambdaLR(optim, lr_lambda=lambda n: max(0.0, 1 - n / max_iters) ** cfg.lr_exp)


def optimizer_kind(state_dict):
    """'adam' or 'sgd' from the per-parameter state keys of an optimiser state dict; None for an empty state (either loads it)."""
    for st in state_dict.get('state', {}).values():
        if 'exp_avg' in st:
            return 'adam'
        if 'momentum_buffer' in st:
            return 'sgd'
    return None


def check_optimizer_state(state_dict, kind):
    """Raises ValueError when a checkpoint's optimiser state was written by the other optimiser than `kind` ('adam' or 'sgd')."""
    found = optimizer_kind(state_dict)
    if found is not None and found != kind:
        raise ValueError(f"the checkpoint's optimizer_state was written by the {found!r} optimiser, this trainer runs {kind!r} "
                         f"(cfg.optimizer): an optimiser state loads only into its own kind")


class Trainer:
    def __init__(self, train_data_loader, cfg, device='cuda'):
        self.cfg = cfg
        self.train_data_loader = train_data_loader
        self.device = torch.device(device)
        self.start_epoch = 0
        self.old_model = None
        self.pseudo = None                # pseudo.PseudoLabeler once begin_task2(pseudo_label=True) ran
        self.pod = None                   # pod.LocalPODLoss once begin_task2(pod_lambda > 0) ran
        self.pod_channels = 0
        self.consolidation = None         # consolidate.Consolidation of the finished task(s) once begin_task2(ewc_lambda > 0) ran
        self.ewc_lambda = 0.0
        self.path = None                  # consolidate.PathIntegral when cfg.path_integral is set (build_model): tracked from the first step
        self.replay = None                # replay.ReplayMemory once begin_task2(replay > 0) ran
        self.replay_batch = 0             # exemplars mixed into every batch
        self.replay_boundary = None       # c_old of the last call that added a segment: the next segment's first class
        self.augment = None               # augment.RandomScaleCrop when cfg.augment is set (build_model)
        self.step_labels = None           # the labels the last train_step's loss was computed against, rows [0, B), before pseudo-labelling
        self.build_model()

    def build_model(self):
        cfg = self.cfg
        self.model = UNet(num_classes=cfg.num_classes, in_dim=3, conv_dim=cfg.conv_dim,
                          compute_dtype=cfg.compute_dtype).to(self.device)
        if getattr(cfg, 'sync_bn', False) and syncbn.initialized():
            self.model = nn.SyncBatchNorm.convert_sync_batchnorm(self.model)
        kind = getattr(cfg, 'optimizer', 'adam')
        if kind == 'adam':
            self.optim = FusedAdam(self.model.parameters(), lr=cfg.lr, betas=[cfg.beta1, cfg.beta2])
        elif kind == 'sgd':
            no_decay = []
            if not getattr(cfg, 'decay_norm_and_bias', True):      # every BatchNorm parameter and every bias
                for mod in self.model.modules():
                    if isinstance(mod, nn.modules.batchnorm._BatchNorm):
                        no_decay += list(mod.parameters(recurse=False))
                    elif getattr(mod, 'bias', None) is not None and isinstance(mod.bias, nn.Parameter):
                        no_decay.append(mod.bias)
            self.optim = FusedSGD(self.model.parameters(), lr=cfg.lr, momentum=getattr(cfg, 'momentum', 0.9),
                                  nesterov=getattr(cfg, 'nesterov', True), weight_decay=getattr(cfg, 'weight_decay', 1e-4),
                                  no_decay=no_decay)
        else:
            raise ValueError(f"optimizer must be 'adam' or 'sgd', not {kind!r}")
        self.path = None
        if getattr(cfg, 'path_integral', False):     # Synaptic Intelligence has to watch task 1: tracking is on from the first step
            self.path = PathIntegral(self.model.named_parameters(), xi=getattr(cfg, 'si_xi', 0.1))
            self.optim.set_path_integral(self.path.omega)
        self.per_iteration = getattr(cfg, 'lr_schedule', 'epoch') == 'iteration'
        loader = self.train_data_loader
        self.scheduler = make_scheduler(self.optim, cfg, len(loader) if self.per_iteration and hasattr(loader, '__len__') else None)
        self.c_loss = CrossEntropyLoss().to(self.device)
        self.likelihood_loss = self.c_loss       # estimate_importance differentiates the plain log-likelihood whatever the step's criterion
        kind = getattr(cfg, 'loss', 'ce')
        if kind == 'ce_dice':
            self.c_loss = DiceCrossEntropyLoss(1.0, getattr(cfg, 'dice_weight', 1.0), getattr(cfg, 'dice_smooth', 1e-5),
                                               getattr(cfg, 'dice_include_background', True), getattr(cfg, 'dice_present_only', True),
                                               getattr(cfg, 'dice_per_image', False)).to(self.device)
        elif kind != 'ce':
            raise ValueError(f"loss must be 'ce' or 'ce_dice', not {kind!r}")
        self.augment = None
        if getattr(cfg, 'augment', False):       # each rank draws its own scales, crops and flips
            rank = torch.distributed.get_rank() if torch.distributed.is_available() and torch.distributed.is_initialized() else 0
            self.augment = RandomScaleCrop(scale=getattr(cfg, 'augment_scale', (0.5, 2.0)), flip=getattr(cfg, 'augment_flip', True),
                                           ignore_index=self.c_loss.ignore_index, seed=int(getattr(cfg, 'augment_seed', 0)) + rank)

    def reset_grad(self):
        self.optim.zero_grad()

    def estimate_importance(self, data_loader, max_batches=None):
        """Diagonal empirical Fisher information of the current model over a loader -> consolidate.Consolidation (finished; its anchor is
        a clone of the current weights).  Every module in eval mode (BatchNorm on its running statistics, nothing updated), one
        CrossEntropyLoss backward per batch, the squared gradients averaged over the batches; no optimizer step.  A loader of batch size 1
        gives the per-image estimate, larger batches the square of the batch-mean gradient (consolidate.py).  Under an initialised process
        group every rank ends with the mean over all ranks' batches.  Each module's own mode is restored and the gradients are cleared."""
        model = self.model
        modes = [(mod, mod.training) for mod in model.modules()]
        sync, model.grad_sync = model.grad_sync, None      # the gradient exchange would average the gradients BEFORE they are squared
        cons = Consolidation(model.named_parameters())
        params = list(model.parameters())
        try:
            model.eval()
            for i, (images, masks) in enumerate(data_loader):
                if max_batches is not None and i >= max_batches:
                    break
                outputs = model(images.to(self.device, non_blocking=True))
                self.reset_grad()
                self.likelihood_loss(outputs, masks.to(self.device, non_blocking=True)).backward()
                cons.accumulate(params)
            cons.finish()
        finally:
            self.reset_grad()
            for mod, mode in modes:
                mod.training = mode
            model.grad_sync = sync
        return cons

    def _apply_consolidation(self):
        self.optim.set_consolidation(self.consolidation.anchor, self.consolidation.importance, self.ewc_lambda)

    def begin_task2(self, c_old, distill_lambda=1.0, temperature=2.0, l2_lambda=0.0, freeze_bn=False, ewc_lambda=0.0,
                    importance_loader=None, ewc_gamma=1.0, new_classes=0, unbiased=False, head_init='background',
                    pseudo_label=False, pseudo_bins=100, pseudo_adaptive=False, pseudo_min_factor=0.0, pseudo_loader=None,
                    pod_lambda=0.0, pod_levels=3, replay=0, replay_batch=0, replay_loader=None, replay_storage='uint8', replay_flip=True,
                    replay_min_pixels=1, replay_seed=0, si_lambda=0.0):
        """Freeze a snapshot of the current model (task 1) and regularise further training towards it.  freeze_bn: every BatchNorm of the
        trained model goes to eval mode -- task 2 normalises with task 1's running statistics and leaves them unchanged (the gradients
        still reach gamma and beta).  ewc_lambda > 0: elastic weight consolidation -- the importance of the finished task is estimated on
        importance_loader (default: the training loader) before anything of the new task is switched on, merged with the previous tasks'
        (importance <- ewc_gamma * previous + new, online EWC) when this is not the first call, and the Adam kernel adds
        ewc_lambda * importance * (theta - theta_old) to every gradient.
        Class-incremental step (build-defined): new_classes > 0 grows the trained model's head by that many outputs AFTER the importance
        estimate and the snapshot (the old model keeps its width; UNet.expand_classes(new_classes, head_init)), carrying Adam's moments and
        the anchors over; unbiased=True distils with UnbiasedDistillationCrossEntropy(c_old, distill_lambda) (no temperature) instead of
        DistillationCrossEntropy.  A later call (task 3) snapshots the grown model: c_old is then the grown width.
        Pseudo-labels (build-defined, pseudo.py): pseudo_label=True calibrates a PseudoLabeler(c_old, pseudo_bins, pseudo_adaptive,
        pseudo_min_factor) with the snapshot on pseudo_loader (default: the training loader -- it should hold the NEW task's data, whose
        old-class pixels are labelled 0); every step then runs the old model's forward, also with distill_lambda == 0, relabels the
        background pixels it is confident about, ignores the others, and (pseudo_adaptive) weights each image's loss by the accepted share.
        Not with unbiased=True (that criterion treats every label < c_old alike: pseudo-labels would change nothing), and pseudo_adaptive
        not with distill_lambda > 0 (DistillationCrossEntropy's kernel has no per-image weight).  The canonical setting is
        begin_task2(c_old, distill_lambda=0, pseudo_label=True, pseudo_adaptive=True).
        Local POD (build-defined, pod.py): pod_lambda > 0 keeps LocalPODLoss(pod_levels, square=False, normalize=True, lam=pod_lambda); every
        step then runs the old model's forward, also with distill_lambda == 0 and without pseudo-labels, and adds
        pod(outputs, old, channels=c_old, merge_extra=True) to the criterion's loss -- the old background against the new background plus
        the new classes.  It combines with every criterion above; PLOP's step is begin_task2(c_old, distill_lambda=0, pseudo_label=True,
        pseudo_adaptive=True, pod_lambda=...).  pod_lambda == 0 leaves the step as it is.
        Exemplar replay (build-defined, replay.py): replay > 0 adds a segment of that many slots to ``self.replay`` (a ReplayMemory with
        replay_storage, replay_flip and replay_seed, created on first use) for the FINISHED task's own classes -- [1, c_old) on the first
        call, [c_old of the previous such call, c_old) later -- and fills it from replay_loader (default: the training loader, with the
        same meaning as importance_loader) by the class-balanced policy with replay_min_pixels, before the snapshot, the criterion switch
        and the growing of the head.  Every step then starts with ``inputs, labels = self.replay.mix(inputs, labels, replay_batch)``
        (replay_batch >= 1 is required): the old model's forward, the pseudo-labels, the distillation terms and the loss all see the
        B + replay_batch rows, and so do the returned outputs; the caller's batch is rows [0, B).  replay == 0 leaves a memory from earlier
        calls (and its replay_batch, unless a new one >= 1 is given) in place and adds nothing.  Data parallelism: each rank keeps its own
        memory, filled from its own shard and sampled with replay_seed + rank; the gradients are averaged as always, no collective is
        added.
        Synaptic Intelligence (build-defined, consolidate.PathIntegral): si_lambda = c > 0 needs cfg.path_integral (the optimiser has been
        accumulating omega since the first step) and is refused together with ewc_lambda > 0 (one importance buffer; the combination is
        Riemannian Walk).  Where the EWC estimate would run, the path integral of the finished task becomes a Consolidation -- importance
        <- previous + max(0, omega) / ((theta - theta_start)^2 + si_xi), anchor = the current weights --, omega and theta_start restart, and
        the consolidation term runs with ewc_lambda = 2 c: consolidation_penalty() is c * sum Omega (theta - theta*)^2.  It composes with
        everything ewc_lambda composes with; si_lambda == 0 leaves an earlier consolidation in place; tracking goes on for the next boundary."""
        if not si_lambda >= 0:
            raise ValueError('si_lambda must be >= 0')
        if si_lambda > 0 and getattr(self, 'path', None) is None:
            raise ValueError('si_lambda > 0 needs cfg.path_integral=True: the path integral has to be tracked from the first step of the task')
        if si_lambda > 0 and ewc_lambda > 0:
            raise ValueError('si_lambda > 0 with ewc_lambda > 0: there is one importance buffer (the combination, Riemannian Walk, is not '
                             'provided)')
        if replay < 0 or replay_batch < 0:
            raise ValueError('replay and replay_batch must be >= 0')
        if replay > 0 and replay_batch < 1:
            raise ValueError('replay > 0 needs replay_batch >= 1 (the number of exemplars mixed into every batch)')
        if not pod_lambda >= 0:
            raise ValueError('pod_lambda must be >= 0')
        if pod_lambda > 0 and int(pod_levels) not in (1, 2, 3):
            raise ValueError('pod_levels must be 1, 2 or 3')
        if pod_lambda > 0 and c_old < 1:
            raise ValueError('pod_lambda > 0 needs c_old >= 1 (class 0, the background, is always an old class)')
        if pseudo_label and unbiased:
            raise ValueError('pseudo_label=True with unbiased=True: the unbiased cross-entropy treats every label below c_old alike, '
                             'so pseudo-labels would change nothing')
        if pseudo_label and pseudo_adaptive and distill_lambda > 0:
            raise ValueError('pseudo_adaptive=True with distill_lambda > 0: DistillationCrossEntropy has no per-image weight '
                             '(use distill_lambda=0, or pseudo_adaptive=False)')
        if getattr(getattr(self, 'cfg', None), 'loss', 'ce') == 'ce_dice':
            if unbiased:
                raise ValueError("loss='ce_dice' with unbiased=True: the Dice term is not defined inside the unbiased criterion "
                                 "(labels below c_old mean 'background or any old class' there)")
            if distill_lambda > 0:
                raise ValueError("loss='ce_dice' with distill_lambda > 0: DistillationCrossEntropy has no Dice term "
                                 "(use distill_lambda=0, with pod_lambda > 0 for distillation)")
            if pseudo_label and pseudo_adaptive:
                raise ValueError("loss='ce_dice' with pseudo_adaptive=True: DiceCrossEntropyLoss has no per-image weight "
                                 "(use pseudo_adaptive=False)")
        if replay > 0:
            self._fill_replay(c_old, replay, self.train_data_loader if replay_loader is None else replay_loader, replay_storage, replay_flip,
                              replay_min_pixels, replay_seed)
        if replay_batch >= 1:
            self.replay_batch = int(replay_batch)
        if ewc_lambda > 0:
            cons = self.estimate_importance(self.train_data_loader if importance_loader is None else importance_loader)
            cons.gamma = float(ewc_gamma)
            if self.consolidation is not None:
                cons.merge_from(self.consolidation, ewc_gamma)
            self.consolidation, self.ewc_lambda = cons, float(ewc_lambda)
        if si_lambda > 0:
            self.consolidation = self.path.consolidate(self.model.named_parameters(), previous=self.consolidation)
            self.path.restart(self.model.parameters())
            self.ewc_lambda = 2.0 * float(si_lambda)
        consolidated = ewc_lambda > 0 or si_lambda > 0
        # a fresh module with a CLONE of the state (not copy.deepcopy: that would duplicate the engine's multi-GB activation
        # buffers and, under data parallelism, the GradSync object with its process group and stream)
        m = self.model
        self.old_model = UNet(m.num_classes, m.in_dim, m.conv_dim, compute_dtype=m.compute_dtype).to(self.device)
        self.old_model.load_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()}, strict=True)
        self.old_model.eval()
        for p in self.old_model.parameters():
            p.requires_grad_(False)
        if unbiased:
            self.distill = UnbiasedDistillationCrossEntropy(c_old, distill_lambda)
        else:
            self.distill = DistillationCrossEntropy(c_old, temperature, distill_lambda) if distill_lambda > 0 else None
        self.pod = LocalPODLoss(pod_levels, square=False, normalize=True, lam=pod_lambda) if pod_lambda > 0 else None
        self.pod_channels = int(c_old)
        self.pseudo = None
        if pseudo_label:
            self.pseudo = PseudoLabeler(c_old, bins=pseudo_bins, adaptive=pseudo_adaptive, min_factor=pseudo_min_factor,
                                        ignore_index=self.c_loss.ignore_index)
            group = m.grad_sync.group if getattr(m, 'grad_sync', None) is not None else None
            self.pseudo.calibrate(self.old_model, self.train_data_loader if pseudo_loader is None else pseudo_loader, self.device, group=group)
        if consolidated:
            self.optim.set_l2_anchor(None, 0.0)        # an earlier task's L2 anchor is another snapshot than the new consolidation anchor
            self._apply_consolidation()
        if l2_lambda > 0:
            self.optim.set_l2_anchor(self.consolidation.anchor if consolidated else [p.detach().clone() for p in self.old_model.parameters()],
                                     l2_lambda)
        if new_classes > 0:
            self.grow_head(new_classes, head_init)
        if freeze_bn:
            for mod in m.modules():
                if isinstance(mod, nn.modules.batchnorm._BatchNorm):       # nn.BatchNorm2d and nn.SyncBatchNorm
                    mod.eval()

    def _fill_replay(self, c_old, capacity, loader, storage, flip, min_pixels, seed):
        """One more segment of the exemplar memory for the classes [previous boundary or 1, c_old), filled from `loader`."""
        lo = 1 if self.replay_boundary is None else self.replay_boundary
        rank = torch.distributed.get_rank() if torch.distributed.is_available() and torch.distributed.is_initialized() else 0
        mem = self.replay
        for images, masks in loader:
            x, y = images.to(self.device, non_blocking=True), masks.to(self.device, non_blocking=True)
            if mem is None:       # the image shape is the data's
                mem = ReplayMemory(c_old, tuple(x.shape[1:]), storage=storage, ignore_index=self.c_loss.ignore_index, flip=flip,
                                   seed=int(seed) + rank)
            if mem.open is None:
                mem.num_classes = max(mem.num_classes, int(c_old))      # the head has grown since the memory was created
                mem.add_task((lo, c_old), capacity, min_pixels)
            mem.observe(x, y)
        if mem is None or mem.open is None:
            raise ValueError('begin_task2(replay > 0): the replay loader gave no batch')
        self.replay = mem.finish()
        self.replay_boundary = int(c_old)

    def grow_head(self, n, init='background'):
        """UNet.expand_classes on the trained model with the optimiser state, the anchors and the consolidation carried over; cfg.num_classes
        (the confusion-matrix width of train_epoch) follows.  Under an initialised process group the grown head is broadcast from rank 0
        (init='default' draws the new rows from each rank's own RNG), so the replicas stay identical whatever their seeds."""
        m = self.model
        names = {id(p): k for k, p in m.named_parameters()}
        ow, ob, nw, nb = m.expand_classes(n, init)
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            group = m.grad_sync.group if m.grad_sync is not None else None
            for t in (nw, nb):
                torch.distributed.broadcast(t.data, src=0, group=group)
        # The order matters.  (1) The Consolidation grows first: it owns the importance (one flat buffer, laid out again) and the anchors,
        # and takes the new rows' anchor from the (broadcast) new parameters.  (2) replace_params swaps the parameter objects and re-homes
        # Adam's moments; it also grows the optimiser's own anchor / importance entries, which is all there is when only the L2 term is on.
        # (3) With a consolidation the optimiser must read the Consolidation's NEW importance views and anchors, so both terms are set
        # again from it (set_l2_anchor(None) first: set_consolidation compares a kept L2 anchor with the one it is given).
        if self.consolidation is not None:
            self.consolidation.grow(names[id(ow)], nw)
            self.consolidation.grow(names[id(ob)], nb)
        if self.path is not None:      # the same order for the path integral: its own buffers first, then the optimiser reads the new views
            self.path.grow(names[id(ow)], nw, ow)     # the old parameters too: start follows what the initialisation does to old rows
            self.path.grow(names[id(ob)], nb, ob)
        self.optim.replace_params({ow: nw, ob: nb})
        if self.path is not None:
            self.optim.set_path_integral(self.path.omega)
        if self.consolidation is not None and self.ewc_lambda > 0:
            l2 = self.optim.l2_lambda
            self.optim.set_l2_anchor(None, 0.0)
            self._apply_consolidation()
            if l2 > 0:
                self.optim.set_l2_anchor(self.consolidation.anchor, l2)
        self.cfg.num_classes = m.num_classes

    # ---- checkpoints: same file name and keys as trainer.py:68-102, but the model never leaves
    # the GPU: the reference does network.cpu() ... network.cuda() (a full D2H + H2D round trip of 124 MB every
    # epoch, trainer.py:75,80-81,258); here the state is copied into pinned host buffers on a side stream.
    def snapshot(self, epoch):
        """Starts an asynchronous device->pinned-host copy of model/optimizer state; returns a handle for write()."""
        if not hasattr(self, '_snap_stream'):
            self._snap_stream = torch.cuda.Stream()
            self._snap_bufs = {}
        st = self._snap_stream
        st.wait_stream(torch.cuda.current_stream())
        host = {}
        with torch.cuda.stream(st):
            for k, v in self.model.state_dict().items():
                buf = self._snap_bufs.get(k)
                if buf is None or buf.shape != v.shape or buf.dtype != v.dtype:
                    buf = self._snap_bufs[k] = torch.empty(v.shape, dtype=v.dtype, pin_memory=True)
                buf.copy_(v, non_blocking=True)
                host[k] = buf
            opt = self.optim.state_dict()
            opt_host = {'param_groups': opt['param_groups'],
                        'state': {i: {n: (t.to('cpu', non_blocking=True) if torch.is_tensor(t) and t.is_cuda else t)
                                      for n, t in s.items()} for i, s in opt['state'].items()}}
            cons_host = None
            if self.consolidation is not None:       # one optional key beside the reference's four
                cs = self.consolidation.state_dict()
                cons_host = {'anchor': {n: t.to('cpu', non_blocking=True) for n, t in cs['anchor'].items()},
                             'importance': {n: t.to('cpu', non_blocking=True) for n, t in cs['importance'].items()},
                             'lambda': self.ewc_lambda, 'gamma': cs['gamma'], 'n_batches': cs['n_batches']}
            path_host = None
            if self.path is not None:                # one more optional key: the running path integral and the task's starting weights
                ps = self.path.state_dict()
                path_host = {'omega': {n: t.to('cpu', non_blocking=True) for n, t in ps['omega'].items()},
                             'start': {n: t.to('cpu', non_blocking=True) for n, t in ps['start'].items()}, 'xi': ps['xi']}
            replay_host = None
            if self.replay is not None:              # a second optional key
                rs = self.replay.state_dict()
                replay_host = {k: (v.to('cpu', non_blocking=True) if torch.is_tensor(v) and v.is_cuda else v) for k, v in rs.items()}
                replay_host.update(batch=self.replay_batch, boundary=self.replay_boundary)
            done = torch.cuda.Event()
            done.record(st)
        snap = {'epoch': epoch + 1, 'model_state': host, 'optimizer_state': opt_host,
                'scheduler_state': self.scheduler.state_dict(), '_event': done}
        if cons_host is not None:
            snap['consolidation_state'] = cons_host
        if path_host is not None:
            snap['path_state'] = path_host
        if replay_host is not None:
            snap['replay_state'] = replay_host
        if self.augment is not None:                 # a third optional key: the configuration and the generator state (a host tensor)
            snap['augment_state'] = self.augment.state_dict()
        return snap

    def save_network(self, network_label, epoch_label, epoch, save_dir):
        """trainer.py:68-81: '<epoch_label>_net_<network_label>.pth' with keys epoch/model_state/optimizer_state/
        scheduler_state (loadable by the reference's load_network and by torch.optim.Adam); with elastic weight consolidation
        active one more key, consolidation_state (anchor, importance, lambda, gamma, n_batches), which the reference ignores; with an exemplar memory
        replay_state (ReplayMemory.state_dict() on the host, replay_batch and the class boundary), ignored by the reference too; with
        augmentation augment_state (RandomScaleCrop.state_dict(): configuration and generator state), likewise; with cfg.path_integral
        path_state (PathIntegral.state_dict(): omega and the task's starting weights by name, and xi), likewise."""
        snap = self.snapshot(epoch)
        snap.pop('_event').synchronize()
        snap['model_state'] = {k: v.clone() for k, v in snap['model_state'].items()}   # pinned buffers are reused
        path = os.path.join(save_dir, '%s_net_%s.pth' % (epoch_label, network_label))
        torch.save(snap, path)
        return path

    def load_network(self, network_label, epoch_label, save_dir):
        """trainer.py:84-102 (without the bare except that hides load errors there)."""
        path = os.path.join(save_dir, '%s_net_%s.pth' % (epoch_label, network_label))
        if not os.path.isfile(path):
            return False
        ck = torch.load(path, map_location='cpu', weights_only=False)
        self.model.load_state_dict(ck['model_state'])
        self.start_epoch = ck['epoch']
        check_optimizer_state(ck['optimizer_state'], getattr(self.cfg, 'optimizer', 'adam'))
        self.optim.load_state_dict(ck['optimizer_state'])
        self.scheduler.load_state_dict(ck['scheduler_state'])
        self.load_consolidation_state(ck.get('consolidation_state'))
        self.load_path_state(ck.get('path_state'))
        self.load_replay_state(ck.get('replay_state'))
        self.load_augment_state(ck.get('augment_state'))
        return True

    def load_path_state(self, state):
        """Restores what snapshot() stored under 'path_state' (None, e.g. a checkpoint without the key: nothing changes -- a path integral
        built by cfg.path_integral stays as built).  A trainer without one starts tracking with the restored state."""
        if state is None:
            return
        if self.path is None:
            self.path = PathIntegral(self.model.named_parameters(), xi=state['xi'])
        self.path.load_state_dict(state)
        self.optim.set_path_integral(self.path.omega)

    def load_augment_state(self, state):
        """Restores what snapshot() stored under 'augment_state' (None, e.g. a checkpoint without the key: nothing changes): the next step
        draws what the uninterrupted run would have drawn."""
        if state is None:
            return
        if self.augment is None:
            self.augment = RandomScaleCrop()
        self.augment.load_state_dict(state)

    def load_replay_state(self, state):
        """Restores what snapshot() stored under 'replay_state' (None, e.g. a checkpoint without the key: nothing changes)."""
        if state is None:
            return
        mem = ReplayMemory(state['num_classes'], state['image_shape'], storage=state['storage'], ignore_index=state['ignore_index'],
                           flip=state['flip'], seed=state['seed'])
        self.replay = mem.load_state_dict(state, device=self.device)
        self.replay_batch, self.replay_boundary = int(state['batch']), state['boundary']

    def load_consolidation_state(self, state):
        """Restores what snapshot() stored under 'consolidation_state' (None, e.g. a checkpoint without the key: nothing changes)."""
        if state is None:
            return
        cons = Consolidation(self.model.named_parameters())
        cons.load_state_dict(state)
        self.consolidation, self.ewc_lambda = cons, float(state['lambda'])
        self._apply_consolidation()

    def train_step(self, inputs, labels):
        """trainer.py:172-176.  With an exemplar memory the batch is first extended by replay_batch exemplars: everything below, and the
        returned outputs, cover B + replay_batch rows, the caller's batch being rows [0, B).  With cfg.augment the (mixed) batch is then
        rescaled, cropped or padded and flipped in one launch, exemplars included: everything below sees the augmented batch.
        ``self.step_labels`` keeps the labels the loss is computed against, rows [0, B), before pseudo-labelling: the caller's own tensor
        without augmentation."""
        self.step_labels = labels
        if self.replay is not None and self.replay_batch > 0:
            inputs, labels = self.replay.mix(inputs, labels, self.replay_batch)
        if self.augment is not None:
            inputs, labels = self.augment(inputs, labels)
            self.step_labels = labels[:self.step_labels.shape[0]]
        outputs = self.model(inputs)
        self.reset_grad()
        distill = getattr(self, 'distill', None) if self.old_model is not None else None
        pod = self.pod if self.old_model is not None else None
        if distill is not None or self.pseudo is not None or pod is not None:
            with torch.no_grad():
                old = self.old_model(inputs)
        nu = None
        if self.pseudo is not None:       # the caller's labels stay what they were (train_epoch's confusion matrix reads them)
            labels, nu = self.pseudo(old, labels)
        if distill is not None:
            loss = distill(outputs, labels, old)
        else:
            loss = self.c_loss(outputs, labels, nu) if nu is not None else self.c_loss(outputs, labels)
        if pod is not None:       # a second loss on the logits: the engine receives the summed NCHW gradient and converts it
            loss = loss + pod(outputs, old, channels=self.pod_channels, merge_extra=True)
        loss.backward()
        self.optim.step()
        if self.per_iteration:
            self.scheduler.step()
        return outputs, loss

    @torch.no_grad()
    def test(self, data_loader):
        """trainer.py:270-284: pixel accuracy (%) of the eval-mode model over a loader.  The arg-max of trainer.py:279 runs
        inside the head kernel (UNet.predict).  Unlike the reference (which never calls .train() again) the
        mode of every module is restored afterwards, each its own (frozen BatchNorm layers stay frozen)."""
        modes = [(mod, mod.training) for mod in self.model.modules()]
        self.model.eval()
        correct = torch.zeros((), dtype=torch.int64, device=self.device)
        total = 0
        for images, masks in data_loader:
            labels = masks.to(self.device, non_blocking=True)
            predicted = self.model.predict(images.to(self.device, non_blocking=True))
            total += labels.numel()
            correct += (predicted == labels).sum()
        for mod, mode in modes:
            mod.training = mode
        return 100.0 * float(correct) / max(total, 1)

    def train_epoch(self, epoch):
        if not self.per_iteration:                   # lr_schedule='iteration': train_step steps it after every optim.step()
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')          # torch warns that scheduler.step() precedes optim.step(); the
                self.scheduler.step()                    # reference does exactly that (trainer.py:147)
        conf = None
        losses = []
        for i, (images, masks) in enumerate(self.train_data_loader):
            inputs = images.to(self.device, non_blocking=True)
            labels = masks.to(self.device, non_blocking=True)
            outputs, loss = self.train_step(inputs, labels)
            if i % self.cfg.stats_every == 0:
                out = outputs.detach()
                labels = self.step_labels                # the caller's labels, or what the augmentation made of them
                if out.shape[0] != labels.shape[0]:      # replayed rows behind the caller's batch
                    out = out[:labels.shape[0]]
                c, _ = argmax_confusion(out, labels, self.cfg.num_classes)
                conf = c if conf is None else conf + c
                losses.append(loss.detach())
        stats = {}
        if conf is not None:
            oa, pc, miu, mx = metrics_from_confusion(conf)
            stats = dict(loss=float(torch.stack(losses).mean()), pixel_acc=float(oa), class_acc=float(pc),
                         mean_iu=float(miu), max_class_acc=float(mx), lr=self.optim.param_groups[0]['lr'])
        return stats

    def train_val(self, epochs=None):
        epoch = self.start_epoch
        out = []
        end = self.cfg.n_iters if epochs is None else min(self.cfg.n_iters, epoch + epochs)
        while epoch < end:
            out.append(self.train_epoch(epoch))
            epoch += 1
        self.start_epoch = epoch
        return out
