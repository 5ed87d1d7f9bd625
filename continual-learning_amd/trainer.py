"""Trainer counterpart for the hot loop of the reference (trainer.py:105-129 build_model, :132-265 train_val).

Same construction and ordering as the reference:
  model  = UNet(num_classes, in_dim=3, conv_dim=64)                       trainer.py:107 (num_classes is a knob here, Q8)
  optim  = Adam(model.parameters(), lr, betas=[beta1, beta2])             trainer.py:108-110 -> FusedAdam
  sched  = LambdaLR(optim, lambda n: (1 - n/n_iters) ** lr_exp)           trainer.py:111-112
  c_loss = CrossEntropyLoss()                                             trainer.py:113
  per epoch: scheduler.step() FIRST (trainer.py:147), then for each batch
      outputs = model(inputs); zero_grad(); loss = c_loss(outputs, labels); loss.backward(); optim.step()   :172-176
Out of scope here: JPEG dumps, prints, checkpoint files; the every-10th-iteration statistics (trainer.py:177-189)
are computed on the GPU by metrics.argmax_confusion instead of .cpu() round trips.
Configuration: ``default_config`` is the one table of defaults and ``complete_config`` fills what a caller's cfg lacks from it, so the
code below reads plain ``cfg.name``.  The build-defined switches are off by default, and nothing on the step's path changes then:
``optimizer='sgd'`` (FusedSGD with momentum, nesterov, weight_decay), ``lr_schedule='iteration'`` (make_scheduler), ``sync_bn``
(syncbn.py), ``augment`` (every training batch, replayed rows included, rescaled, cropped or padded and flipped in one launch
before the forward pass, augment.py), ``loss='ce_dice'`` (loss.DiceCrossEntropyLoss as the step's criterion: each rank's Dice sums cover
its own batch, and ``estimate_importance`` keeps the plain log-likelihood), ``class_weights`` / ``label_smoothing`` / ``focal_gamma``
(loss.CrossEntropyLoss with them as the step's criterion; ``set_class_weights`` sets the weights later, grow_head extends them with ones,
a checkpoint carries them; each rank divides by its own weight sum), ``path_integral`` (consolidate.PathIntegral: Synaptic
Intelligence's path integral, tracked inside every optimiser step from the first one), ``max_grad_norm`` (optim.set_grad_clip: the
global gradient norm clipped inside the optimiser step; nnU-Net trains with 12).
Continual learning (config 4): ``Trainer.begin_task2`` is the task boundary; its docstring numbers the stages once and places every
feature at its stage.  What a feature adds to the trainer is declared once, at the top of the class.
"""
import contextlib
import os
import warnings
from types import SimpleNamespace

import torch
import torch.nn as nn
from torch.optim.lr_scheduler import LambdaLR

from .loss import (CrossEntropyLoss, DiceCrossEntropyLoss, DistillationCrossEntropy, UnbiasedDistillationCrossEntropy, check_class_weight,
                   check_smoothing_and_gamma, class_weights)
from .metrics import argmax_confusion, metrics_from_confusion
from .optim import FusedAdam, FusedSGD
from .consolidate import Consolidation, PathIntegral
from .pseudo import PseudoLabeler
from .pod import LocalPODLoss
from .replay import ReplayMemory, class_pixel_counts
from .augment import RandomScaleCrop
from . import syncbn
from .unet import UNet


def default_config(**kw):
    """Defaults of main.py:64-105 for the flags the hot path reads."""
    cfg = dict(n_iters=10000, train_batch_size=2, lr=1e-4, lr_exp=0.9, beta1=0.5, beta2=0.99, h_image_size=512,
               w_image_size=256, num_classes=21, conv_dim=64, compute_dtype='fp32', stats_every=10, sync_bn=False,
               augment=False, augment_scale=(0.5, 2.0), augment_flip=True, augment_seed=0,
               optimizer='adam', momentum=0.9, nesterov=True, weight_decay=1e-4, decay_norm_and_bias=True, lr_schedule='epoch',
               max_iters=None, path_integral=False, si_xi=0.1, max_grad_norm=None,
               loss='ce', dice_weight=1.0, dice_smooth=1e-5, dice_include_background=True, dice_present_only=True, dice_per_image=False,
               class_weights=None, label_smoothing=0.0, focal_gamma=0.0)
    cfg.update(kw)
    return SimpleNamespace(**cfg)


def complete_config(cfg):
    """Sets every field of default_config() that `cfg` (any attribute namespace) lacks, on that same object, and returns it: a default
    is written in default_config and nowhere else.  The caller's object is kept: grow_head writes cfg.num_classes back to it."""
    for name, value in vars(default_config()).items():
        if not hasattr(cfg, name):
            setattr(cfg, name, value)
    return cfg


def make_scheduler(optim, cfg, iters_per_epoch=None):
    """The learning-rate schedule of cfg.lr_schedule on any optimiser.  'epoch' (the default, the reference's trainer.py:111-112): (1 - n/n_iters)
    ** lr_exp, stepped once at the start of every epoch.  'iteration' (build-defined, what the class-incremental segmentation papers train
    with): max(0, 1 - n/max_iters) ** lr_exp, stepped after every optimiser step; cfg.max_iters None means n_iters * iters_per_epoch."""
    kind = complete_config(cfg).lr_schedule
    if kind == 'epoch':
        return LambdaLR(optim, lr_lambda=lambda n: (1 - n / cfg.n_iters) ** cfg.lr_exp)
    if kind != 'iteration':
        raise ValueError(f"lr_schedule must be 'epoch' or 'iteration', not {kind!r}")
    max_iters = cfg.max_iters
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


def _host_copy(obj):
    """A nested state for a checkpoint: dicts, lists and tuples rebuilt, CUDA tensors copied out on the current stream, the rest as it is."""
    if isinstance(obj, dict):
        return {k: _host_copy(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_host_copy(v) for v in obj)
    if torch.is_tensor(obj) and obj.is_cuda:
        return obj.to('cpu', non_blocking=True)
    return obj


@contextlib.contextmanager
def _eval_mode(model):
    """model.eval() inside the block; on the way out, after an error too, every module gets its own training flag back."""
    modes = [(mod, mod.training) for mod in model.modules()]
    model.eval()
    try:
        yield
    finally:
        for mod, mode in modes:
            mod.training = mode


class Trainer:
    old_model = None           # the frozen snapshot of the finished task's model (begin_task2); this and the following: off until they are set
    distill = None             # the distillation criterion that replaces c_loss in the step (begin_task2(distill_lambda > 0 or unbiased))
    pseudo = None              # pseudo.PseudoLabeler once begin_task2(pseudo_label=True) ran
    pod = None                 # pod.LocalPODLoss once begin_task2(pod_lambda > 0) ran
    pod_channels = 0           # the c_old that loss compares
    consolidation = None       # consolidate.Consolidation of the finished task(s) once begin_task2(ewc_lambda > 0 or si_lambda > 0) ran
    ewc_lambda = 0.0           # the weight the optimiser applies it with
    path = None                # consolidate.PathIntegral when cfg.path_integral is set (build_model): tracked from the first step
    replay = None              # replay.ReplayMemory once begin_task2(replay > 0) ran
    replay_batch = 0           # exemplars mixed into every batch
    replay_boundary = None     # c_old of the last call that added a segment: the next segment's first class
    augment = None             # augment.RandomScaleCrop when cfg.augment is set (build_model)
    step_labels = None         # the labels the last train_step's loss was computed against, rows [0, B), before pseudo-labelling

    def __init__(self, train_data_loader, cfg, device='cuda'):
        self.cfg = complete_config(cfg)
        self.train_data_loader = train_data_loader
        self.device = torch.device(device)
        self.start_epoch = 0
        self.build_model()

    def build_model(self):
        cfg = self.cfg
        self.model = UNet(num_classes=cfg.num_classes, in_dim=3, conv_dim=cfg.conv_dim,
                          compute_dtype=cfg.compute_dtype).to(self.device)
        if cfg.sync_bn and syncbn.initialized():
            self.model = nn.SyncBatchNorm.convert_sync_batchnorm(self.model)
        self.optim = self._make_optimizer()
        self.path = PathIntegral(self.model.named_parameters(), xi=cfg.si_xi) if cfg.path_integral else None
        if self.path is not None:     # Synaptic Intelligence has to watch task 1: tracking is on from the first step
            self.optim.set_path_integral(self.path.omega)
        self.per_iteration = cfg.lr_schedule == 'iteration'
        loader = self.train_data_loader
        self.scheduler = make_scheduler(self.optim, cfg, len(loader) if self.per_iteration and hasattr(loader, '__len__') else None)
        self.c_loss = CrossEntropyLoss().to(self.device)
        self.likelihood_loss = self.c_loss       # estimate_importance differentiates the plain log-likelihood whatever the step's criterion
        if cfg.loss == 'ce_dice':
            self.c_loss = DiceCrossEntropyLoss(1.0, cfg.dice_weight, cfg.dice_smooth, cfg.dice_include_background, cfg.dice_present_only,
                                               cfg.dice_per_image).to(self.device)
        elif cfg.loss != 'ce':
            raise ValueError(f"loss must be 'ce' or 'ce_dice', not {cfg.loss!r}")
        eps, gamma = check_smoothing_and_gamma(cfg.label_smoothing, cfg.focal_gamma)
        weights = None if cfg.class_weights is None else check_class_weight(cfg.class_weights, cfg.num_classes)
        if weights is not None or eps > 0 or gamma > 0:      # a criterion of its own: likelihood_loss stays the plain one
            if cfg.loss == 'ce_dice':
                raise ValueError("loss='ce_dice' with class_weights, label_smoothing or focal_gamma: DiceCrossEntropyLoss's cross-entropy term "
                                 "is the plain one (use loss='ce')")
            self.c_loss = CrossEntropyLoss(weight=weights, label_smoothing=eps, focal_gamma=gamma).to(self.device)
        self.augment = RandomScaleCrop(scale=cfg.augment_scale, flip=cfg.augment_flip, ignore_index=self.c_loss.ignore_index,
                                       seed=int(cfg.augment_seed) + syncbn.rank()) if cfg.augment else None      # each rank draws its own

    def class_criterion_active(self):
        """Whether the step's criterion is the generalised cross-entropy (class weights, label smoothing or the focal term)."""
        return isinstance(self.c_loss, CrossEntropyLoss) and self.c_loss.generalised

    @property
    def class_weight(self):
        """The active class weights (a device fp32 [num_classes] tensor) or None."""
        return self.c_loss.weight if isinstance(self.c_loss, CrossEntropyLoss) else None

    def set_class_weights(self, weights_or_scheme, loader=None):
        """The step's class weights: a vector of num_classes finite numbers >= 0, or a scheme of loss.class_weights ('median_frequency',
        'inverse_log') with a loader of (images, masks) batches whose masks are counted on the device (replay.class_pixel_counts), or None
        for none.  May be called again, e.g. after grow_head with the new task's loader.  -> the weights (fp32 on the device) or None."""
        if self.cfg.loss != 'ce':
            raise ValueError("set_class_weights needs loss='ce': DiceCrossEntropyLoss's cross-entropy term is the plain one")
        if weights_or_scheme is not None and self.distill is not None:      # the step would run self.distill and never read them
            raise ValueError('set_class_weights after begin_task2(distill_lambda > 0 or unbiased=True): the step runs '
                             f'{type(self.distill).__name__}, which has no class weights (begin_task2 refuses the combination as well)')
        K = self.cfg.num_classes
        if isinstance(weights_or_scheme, str):
            if loader is None:
                raise ValueError(f'set_class_weights({weights_or_scheme!r}) needs a loader to count the classes on')
            counts = [class_pixel_counts(masks.to(self.device, non_blocking=True), K, self.c_loss.ignore_index) for _, masks in loader]
            if not counts:
                raise ValueError('set_class_weights: the loader gave no batch')
            weights = class_weights(torch.cat(counts).cpu(), weights_or_scheme)
        else:
            weights = None if weights_or_scheme is None else check_class_weight(weights_or_scheme, K)
        if self.c_loss is self.likelihood_loss:      # the step gets a criterion of its own: estimate_importance keeps the plain one
            self.c_loss = CrossEntropyLoss(self.c_loss.ignore_index).to(self.device)
        self.c_loss.set_weight(None if weights is None else weights.to(self.device))
        return self.c_loss.weight

    def _make_optimizer(self):
        optim = self._new_optimizer()
        optim.set_grad_clip(self.cfg.max_grad_norm)      # None: off, the step launches what it always did
        return optim

    def _new_optimizer(self):
        cfg = self.cfg
        if cfg.optimizer == 'adam':
            return FusedAdam(self.model.parameters(), lr=cfg.lr, betas=[cfg.beta1, cfg.beta2])
        if cfg.optimizer != 'sgd':
            raise ValueError(f"optimizer must be 'adam' or 'sgd', not {cfg.optimizer!r}")
        no_decay = []
        if not cfg.decay_norm_and_bias:      # every BatchNorm parameter and every bias
            for mod in self.model.modules():
                if isinstance(mod, nn.modules.batchnorm._BatchNorm):
                    no_decay += list(mod.parameters(recurse=False))
                elif getattr(mod, 'bias', None) is not None and isinstance(mod.bias, nn.Parameter):
                    no_decay.append(mod.bias)
        return FusedSGD(self.model.parameters(), lr=cfg.lr, momentum=cfg.momentum, nesterov=cfg.nesterov, weight_decay=cfg.weight_decay,
                        no_decay=no_decay)

    def _group(self):
        sync = self.model.grad_sync       # the process group of the gradient exchange; None (the default group) without one
        return sync.group if sync is not None else None

    def reset_grad(self):
        self.optim.zero_grad()

    def estimate_importance(self, data_loader, max_batches=None):
        """Diagonal empirical Fisher information of the current model over a loader -> consolidate.Consolidation (finished; its anchor is a
        clone of the current weights).  Every module in eval mode (BatchNorm on its running statistics, nothing updated), one CrossEntropyLoss
        backward per batch, the squared gradients averaged over the batches; no optimizer step.  A loader of batch size 1 gives the per-image
        estimate, larger batches the square of the batch-mean gradient (consolidate.py).  Under an initialised process group every rank ends
        with the mean over all ranks' batches.  Each module's own mode is restored and the gradients are cleared."""
        model = self.model
        sync, model.grad_sync = model.grad_sync, None      # the gradient exchange would average the gradients BEFORE they are squared
        cons = Consolidation(model.named_parameters())
        params = list(model.parameters())
        try:
            with _eval_mode(model):
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
            model.grad_sync = sync
        return cons

    def _install_consolidation(self, l2_lambda):
        """Hands self.consolidation to the optimiser, with the L2 term on its anchor when l2_lambda > 0.  An L2 anchor from before goes
        first: it is another snapshot than the consolidation's, and set_consolidation compares a kept L2 anchor with the one it is given."""
        self.optim.set_l2_anchor(None, 0.0)
        self.optim.set_consolidation(self.consolidation.anchor, self.consolidation.importance, self.ewc_lambda)
        if l2_lambda > 0:
            self.optim.set_l2_anchor(self.consolidation.anchor, l2_lambda)

    def begin_task2(self, c_old, distill_lambda=1.0, temperature=2.0, l2_lambda=0.0, freeze_bn=False, ewc_lambda=0.0,
                    importance_loader=None, ewc_gamma=1.0, new_classes=0, unbiased=False, head_init='background',
                    pseudo_label=False, pseudo_bins=100, pseudo_adaptive=False, pseudo_min_factor=0.0, pseudo_loader=None,
                    pod_lambda=0.0, pod_levels=3, replay=0, replay_batch=0, replay_loader=None, replay_storage='uint8', replay_flip=True,
                    replay_min_pixels=1, replay_seed=0, si_lambda=0.0):
        """The task boundary: freeze a snapshot of the current model (the finished task) and regularise further training towards it.
        The stages, in this order (every loader defaults to the training loader):
          1. every argument check (_check_task2, whose messages say what is refused and why): nothing has changed when one raises;
          2. replay fill: the exemplar memory takes its segment of the FINISHED task's data (_fill_replay), and replay_batch;
          3. consolidation of the finished task (_consolidate_finished_task): the EWC estimate and merge, or the path integral;
          4. the snapshot ``self.old_model`` (_freeze_old_model): the un-grown model, in eval mode, without gradients;
          5. the criteria: ``distill``, ``pod`` / ``pod_channels``, and ``pseudo`` with its calibration on the snapshot;
          6. the optimiser's anchors: the consolidation (_install_consolidation), or the L2 term alone on clones of the snapshot;
          7. head growth (grow_head: optimiser state, anchors, consolidation and path integral carried over), then the BatchNorm freeze.
        freeze_bn (stage 7): every BatchNorm of the trained model goes to eval mode: task 1's running statistics, unchanged; gamma and beta train.
        EWC (stages 3, 6): ewc_lambda > 0 estimates the finished task's importance on importance_loader, merges the previous tasks' into
        it on a later call (importance <- ewc_gamma * previous + new, online EWC), and the optimiser's kernel adds ewc_lambda * importance
        * (theta - theta_old) to every gradient.
        Class-incremental step (build-defined; stages 5, 7): new_classes > 0 grows the trained model's head by that many outputs
        (UNet.expand_classes(new_classes, head_init); the old model keeps its width, and a later call, task 3, snapshots the grown model: its
        c_old is the grown width); unbiased=True distils with UnbiasedDistillationCrossEntropy(c_old, distill_lambda), no temperature.
        Pseudo-labels (build-defined, pseudo.py; stage 5): pseudo_label=True calibrates a PseudoLabeler(c_old, pseudo_bins, pseudo_adaptive,
        pseudo_min_factor) on pseudo_loader (the NEW task's data, whose old-class pixels are labelled 0); every step then runs the old
        model's forward, also with distill_lambda == 0, relabels the background pixels it is confident about, ignores the others, and
        (pseudo_adaptive) weights each image's loss by the accepted share; canonical: distill_lambda=0, pseudo_label=True, pseudo_adaptive=True.
        Local POD (build-defined, pod.py; stage 5): pod_lambda > 0 keeps LocalPODLoss(pod_levels, square=False, normalize=True,
        lam=pod_lambda); every step then runs the old model's forward and adds pod(outputs, old, channels=c_old, merge_extra=True) to the
        criterion's loss -- the old background against the new background plus the new classes.  It combines with every criterion above:
        PLOP's step is the canonical pseudo-label setting with pod_lambda > 0.
        Exemplar replay (build-defined, replay.py; stage 2): replay > 0 adds a segment of that many slots to ``self.replay`` (a ReplayMemory
        with replay_storage, replay_flip and replay_seed + rank, created on first use; each rank keeps its own) for the finished task's own
        classes -- [1, c_old) on the first call, [c_old of the previous such call, c_old) later -- filled from replay_loader by the
        class-balanced policy with replay_min_pixels.  Every step then starts with ``self.replay.mix(inputs, labels, replay_batch)``: all
        that follows, and the returned outputs, see B + replay_batch rows, the caller's batch being rows [0, B).  replay == 0 leaves an
        earlier memory (and its replay_batch, unless a new one >= 1 is given) in place.
        Synaptic Intelligence (build-defined, consolidate.PathIntegral; stages 3, 6): si_lambda = c > 0 turns the finished task's path
        integral into the Consolidation -- importance <- previous + max(0, omega) / ((theta - theta_start)^2 + si_xi), anchor = the
        current weights --, omega and theta_start restart, and the term runs with ewc_lambda = 2 c: consolidation_penalty() is
        c * sum Omega (theta - theta*)^2.  si_lambda == 0 leaves an earlier consolidation in place."""
        self._check_task2(c_old, distill_lambda, ewc_lambda, unbiased, pseudo_label, pseudo_adaptive, pod_lambda, pod_levels, replay,
                          replay_batch, si_lambda)
        if replay > 0:
            self._fill_replay(c_old, replay, self.train_data_loader if replay_loader is None else replay_loader, replay_storage, replay_flip,
                              replay_min_pixels, replay_seed)
        if replay_batch >= 1:
            self.replay_batch = int(replay_batch)
        consolidated = self._consolidate_finished_task(ewc_lambda, importance_loader, ewc_gamma, si_lambda)
        self._freeze_old_model()
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
            self.pseudo.calibrate(self.old_model, self.train_data_loader if pseudo_loader is None else pseudo_loader, self.device,
                                  group=self._group())
        if consolidated:
            self._install_consolidation(l2_lambda)
        elif l2_lambda > 0:       # the L2 term alone pulls towards the snapshot itself
            self.optim.set_l2_anchor([p.detach().clone() for p in self.old_model.parameters()], l2_lambda)
        if new_classes > 0:
            self.grow_head(new_classes, head_init)
        if freeze_bn:
            for mod in self.model.modules():
                if isinstance(mod, nn.modules.batchnorm._BatchNorm):       # nn.BatchNorm2d and nn.SyncBatchNorm
                    mod.eval()

    def _check_task2(self, c_old, distill_lambda, ewc_lambda, unbiased, pseudo_label, pseudo_adaptive, pod_lambda, pod_levels, replay,
                     replay_batch, si_lambda):
        """Stage 1 of begin_task2: raises ValueError for what the boundary refuses; reads only."""
        if not si_lambda >= 0:
            raise ValueError('si_lambda must be >= 0')
        if si_lambda > 0 and self.path is None:
            raise ValueError('si_lambda > 0 needs cfg.path_integral=True: the path integral has to be tracked from the first step of the task')
        if si_lambda > 0 and ewc_lambda > 0:
            raise ValueError('si_lambda > 0 with ewc_lambda > 0: there is one importance buffer (the combination, Riemannian Walk, is not provided)')
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
        if self.class_criterion_active():
            if unbiased:
                raise ValueError('class_weights, label_smoothing or focal_gamma with unbiased=True: UnbiasedDistillationCrossEntropy has none '
                                 'of them (its kernel is another one; pseudo_label=True and pod_lambda > 0 combine with them)')
            if distill_lambda > 0:
                raise ValueError('class_weights, label_smoothing or focal_gamma with distill_lambda > 0: DistillationCrossEntropy has none '
                                 'of them (use distill_lambda=0, with pod_lambda > 0 for distillation)')
        if self.cfg.loss == 'ce_dice':
            if unbiased:
                raise ValueError("loss='ce_dice' with unbiased=True: the Dice term is not defined inside the unbiased criterion "
                                 "(labels below c_old mean 'background or any old class' there)")
            if distill_lambda > 0:
                raise ValueError("loss='ce_dice' with distill_lambda > 0: DistillationCrossEntropy has no Dice term "
                                 "(use distill_lambda=0, with pod_lambda > 0 for distillation)")
            if pseudo_label and pseudo_adaptive:
                raise ValueError("loss='ce_dice' with pseudo_adaptive=True: DiceCrossEntropyLoss has no per-image weight (use pseudo_adaptive=False)")

    def _consolidate_finished_task(self, ewc_lambda, importance_loader, ewc_gamma, si_lambda):
        """Stage 3 of begin_task2: self.consolidation and self.ewc_lambda from the Fisher estimate or the path integral; -> whether either ran."""
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
        return ewc_lambda > 0 or si_lambda > 0

    def _freeze_old_model(self):
        """Stage 4 of begin_task2: a fresh module with a CLONE of the state (not copy.deepcopy: that would duplicate the engine's multi-GB
        activation buffers and, under data parallelism, the GradSync object with its process group and stream)."""
        m = self.model
        self.old_model = UNet(m.num_classes, m.in_dim, m.conv_dim, compute_dtype=m.compute_dtype).to(self.device)
        self.old_model.load_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()}, strict=True)
        self.old_model.eval()
        for p in self.old_model.parameters():
            p.requires_grad_(False)

    def _fill_replay(self, c_old, capacity, loader, storage, flip, min_pixels, seed):
        """One more segment of the exemplar memory for the classes [previous boundary or 1, c_old), filled from `loader`."""
        lo = 1 if self.replay_boundary is None else self.replay_boundary
        mem = self.replay
        for images, masks in loader:
            x, y = images.to(self.device, non_blocking=True), masks.to(self.device, non_blocking=True)
            if mem is None:       # the image shape is the data's
                mem = ReplayMemory(c_old, tuple(x.shape[1:]), storage=storage, ignore_index=self.c_loss.ignore_index, flip=flip,
                                   seed=int(seed) + syncbn.rank())
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
        if syncbn.initialized():
            for t in (nw, nb):
                torch.distributed.broadcast(t.data, src=0, group=self._group())
        # The order matters.  (1) The Consolidation grows first: it owns the importance (one flat buffer, laid out again) and the anchors,
        # and takes the new rows' anchor from the (broadcast) new parameters.  (2) replace_params swaps the parameter objects and re-homes
        # Adam's moments; it also grows the optimiser's own anchor / importance entries, which is all there is when only the L2 term is on.
        # (3) With a consolidation the optimiser must read the Consolidation's NEW importance views and anchors: both terms are set again.
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
            self._install_consolidation(self.optim.l2_lambda)
        self.cfg.num_classes = m.num_classes
        w = self.class_weight
        if w is not None:             # the new classes weigh 1.0 until set_class_weights is called again
            self.c_loss.set_weight(torch.cat([w, w.new_ones(m.num_classes - w.numel())]))

    # ---- checkpoints: same file name and keys as trainer.py:68-102, but the model never leaves the GPU: the reference
    # does network.cpu() ... network.cuda() (124 MB each way every epoch, trainer.py:75,80-81,258); here a side stream copies the state out.
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
            snap = {'epoch': epoch + 1, 'model_state': host,
                    'optimizer_state': {'param_groups': opt['param_groups'], 'state': _host_copy(opt['state'])}}
            # the optional keys beside the reference's four, each while its object exists: its state_dict() on the host + the trainer's scalars
            if self.consolidation is not None:
                snap['consolidation_state'] = dict(_host_copy(self.consolidation.state_dict()), **{'lambda': self.ewc_lambda})
            if self.path is not None:                # the running path integral and the task's starting weights
                snap['path_state'] = _host_copy(self.path.state_dict())
            if self.replay is not None:
                snap['replay_state'] = dict(_host_copy(self.replay.state_dict()), batch=self.replay_batch, boundary=self.replay_boundary)
            if self.class_weight is not None:        # the active class weights (cfg.class_weights, set_class_weights, grow_head)
                snap['class_weight_state'] = {'weight': _host_copy(self.class_weight.detach().clone())}
            snap['_event'] = torch.cuda.Event()
            snap['_event'].record(st)
        snap['scheduler_state'] = self.scheduler.state_dict()
        if self.augment is not None:                 # the configuration and the generator state (a host tensor)
            snap['augment_state'] = self.augment.state_dict()
        return snap

    def save_network(self, network_label, epoch_label, epoch, save_dir):
        """trainer.py:68-81: '<epoch_label>_net_<network_label>.pth' with keys epoch/model_state/optimizer_state/scheduler_state (loadable by
        the reference's load_network and by torch.optim.Adam) and snapshot()'s optional keys, which the reference ignores: consolidation_state
        (anchor, importance, n_batches, gamma; lambda), path_state (omega, start, xi), replay_state (ReplayMemory.state_dict(); batch,
        boundary), augment_state (RandomScaleCrop.state_dict()) and class_weight_state (weight: the active class weights)."""
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
        check_optimizer_state(ck['optimizer_state'], self.cfg.optimizer)
        self.optim.load_state_dict(ck['optimizer_state'])
        self.scheduler.load_state_dict(ck['scheduler_state'])
        self.load_consolidation_state(ck.get('consolidation_state'))
        self.load_path_state(ck.get('path_state'))
        self.load_replay_state(ck.get('replay_state'))
        self.load_augment_state(ck.get('augment_state'))
        self.load_class_weight_state(ck.get('class_weight_state'))
        return True

    def load_class_weight_state(self, state):
        """Restores what snapshot() stored under 'class_weight_state' (None, e.g. a checkpoint without the key: nothing changes)."""
        if state is None:
            return
        n = int(state['weight'].numel())
        if n != self.cfg.num_classes:
            raise ValueError(f'the checkpoint carries class weights for {n} classes, this trainer has {self.cfg.num_classes}: it was written '
                             f'after grow_head -- build the Trainer with num_classes={n}, or grow its head, before load_network')
        self.set_class_weights(state['weight'])

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
        self.optim.set_consolidation(self.consolidation.anchor, self.consolidation.importance, self.ewc_lambda)

    def train_step(self, inputs, labels):
        """trainer.py:172-176.  With an exemplar memory the batch is first extended by replay_batch exemplars: everything below, and the
        returned outputs, cover B + replay_batch rows, the caller's batch being rows [0, B).  With cfg.augment the (mixed) batch is then
        rescaled, cropped or padded and flipped in one launch, exemplars included: everything below sees the augmented batch.  ``self.step_labels``
        keeps the labels the loss is computed against, rows [0, B), before pseudo-labelling: the caller's own tensor without augmentation."""
        self.step_labels = labels
        if self.replay is not None and self.replay_batch > 0:
            inputs, labels = self.replay.mix(inputs, labels, self.replay_batch)
        if self.augment is not None:
            inputs, labels = self.augment(inputs, labels)
            self.step_labels = labels[:self.step_labels.shape[0]]
        outputs = self.model(inputs)
        self.reset_grad()
        distill = self.distill if self.old_model is not None else None
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
        correct = torch.zeros((), dtype=torch.int64, device=self.device)
        total = 0
        with _eval_mode(self.model):
            for images, masks in data_loader:
                labels = masks.to(self.device, non_blocking=True)
                predicted = self.model.predict(images.to(self.device, non_blocking=True))
                total += labels.numel()
                correct += (predicted == labels).sum()
        return 100.0 * float(correct) / max(total, 1)

    def train_epoch(self, epoch):
        if not self.per_iteration:                   # lr_schedule='iteration': train_step steps it after every optim.step()
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')          # torch warns that scheduler.step() precedes optim.step(); the
                self.scheduler.step()                    # reference does exactly that (trainer.py:147)
        conf = None
        losses = []
        clipping = self.cfg.max_grad_norm is not None
        clips = []                                       # (iteration, device copy of the optimiser's norm, coefficient, scale, non-finite flag)
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
                if clipping:
                    clips.append((i, self.optim.clip_state.clone()))
        stats = {}
        if conf is not None:
            oa, pc, miu, mx = metrics_from_confusion(conf)
            stats = dict(loss=float(torch.stack(losses).mean()), pixel_acc=float(oa), class_acc=float(pc),
                         mean_iu=float(miu), max_class_acc=float(mx), lr=self.optim.param_groups[0]['lr'])
            if clipping:      # read here, with the other statistics: the step itself reads nothing back
                seen = torch.stack([c for _, c in clips]).cpu()
                for (i, _), row in zip(clips, seen):
                    if float(row[3]) != 0.0:
                        raise ValueError(f'epoch {epoch}, iteration {i}: the gradient norm is not finite ({float(row[0])})')
                stats.update(grad_norm=float(seen[:, 0].mean()), clipped=float((seen[:, 1] < 1).float().mean()))
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
