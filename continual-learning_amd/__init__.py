"""MI355X-native UNet segmentation train-step path (drop-in for the hot path of LorenzoFramba/Continual-Learning).

Import as ``continual_learning_amd`` (the directory name has a hyphen; ``continual_learning_amd.py`` at the repository
root is the import shim).  Everything compute-related goes through libclamd.so (hand-written HIP for gfx950).
"""
from . import _lib, ops, synth  # noqa: F401
from .unet import UNet, cpad, stage_table  # noqa: F401
from .loss import CrossEntropyLoss, DistillationCrossEntropy, UnbiasedDistillationCrossEntropy, DiceCrossEntropyLoss, class_weights  # noqa: F401
from .optim import FusedAdam, FusedSGD  # noqa: F401
from .consolidate import Consolidation, PathIntegral  # noqa: F401
from .pseudo import PseudoLabeler, thresholds_from_histogram  # noqa: F401
from .pod import LocalPODLoss  # noqa: F401
from .replay import ReplayMemory, class_pixel_counts  # noqa: F401
from .augment import RandomScaleCrop, augment_batch, params_from_draws  # noqa: F401
from .metrics import argmax_confusion, eval_metrics, metrics_from_confusion  # noqa: F401
from .trainer import Trainer, default_config  # noqa: F401
from . import augment, consolidate, data, ddp, pod, pseudo, replay, syncbn  # noqa: F401

__all__ = ['UNet', 'CrossEntropyLoss', 'DistillationCrossEntropy', 'UnbiasedDistillationCrossEntropy', 'DiceCrossEntropyLoss', 'class_weights', 'FusedAdam', 'FusedSGD', 'Consolidation', 'PathIntegral', 'PseudoLabeler', 'thresholds_from_histogram', 'LocalPODLoss', 'ReplayMemory', 'class_pixel_counts', 'replay', 'RandomScaleCrop', 'augment_batch', 'params_from_draws', 'augment', 'Trainer', 'default_config',
           'argmax_confusion', 'eval_metrics', 'metrics_from_confusion', 'data', 'ddp', 'synth']
