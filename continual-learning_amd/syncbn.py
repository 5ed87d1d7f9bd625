"""Synchronised BatchNorm: ``nn.SyncBatchNorm.convert_sync_batchnorm(model)`` on a UNet (or ``Trainer(cfg.sync_bn=True)``).

A converted train-mode layer normalises with the mean and variance of the GLOBAL batch, as torch's SyncBatchNorm does: the engine
(unet.py) and the stand-alone blocks (blocks.py) add the layer's partial rows into fp64 totals (clamd_bn_rows_total), all-reduce the
[2][Cp] totals plus the pixel count, and finalize from the result (clamd_bn_finalize_total, clamd_bn_bwd_finalize_total).  Layers in
eval mode, and every layer while no process group is initialised, run exactly as plain nn.BatchNorm2d.  With a group of world size 1
the all-reduce is the identity and the step is bit-identical to the unconverted model.

The BatchNorm sums never share a communicator with ddp.GradSync's gradient buckets: a group runs its collectives in order on one
internal stream, and a 16-KB BatchNorm sum on the critical chain would queue behind a multi-MB bucket.  Modules whose
``process_group`` is None use one dedicated group over the world (``dist.new_group``), created on first use -- at the same point of
the program on every rank -- and shared by every model of the process.
"""
import torch
import torch.distributed as dist
import torch.nn as nn

_DEDICATED = [None, None]      # (the default group it was made under, the dedicated BatchNorm group)


def initialized():
    return dist.is_available() and dist.is_initialized()


def rank():
    """This process's rank in the default group; 0 while no process group is initialised."""
    return dist.get_rank() if initialized() else 0


def bn_group():
    """The dedicated group over the world for the BatchNorm sums of modules whose process_group is None (made again after the
    default group was destroyed and initialised anew)."""
    world = dist.group.WORLD
    if _DEDICATED[0] is not world:
        _DEDICATED[:] = [world, dist.new_group()]
    return _DEDICATED[1]


def check_groups(named):
    """named: [(name, module)] of a model's BatchNorm layers.  Every nn.SyncBatchNorm must use the same process_group (or all None):
    returns it, or raises ValueError naming the layers that differ from the first one."""
    syncs = [(n, m) for n, m in named if isinstance(m, nn.SyncBatchNorm)]
    if not syncs:
        return None
    g0 = syncs[0][1].process_group
    odd = [n for n, m in syncs if m.process_group is not g0]
    if odd:
        raise ValueError(f'SyncBatchNorm layers of one model must share one process_group: {", ".join(odd)} use another group than '
                         f'{syncs[0][0]}')
    return g0


def resolve(named):
    """named: [(name, module)] of a model's BatchNorm layers in unit order.  Returns (group, flags): flags[i] is True where layer i is a
    train-mode nn.SyncBatchNorm and a process group is initialised (its statistics are all-reduced over `group`); (None, all False) when
    no layer is synchronised.  Raises ValueError on mixed process groups."""
    g = check_groups(named)
    flags = tuple(isinstance(m, nn.SyncBatchNorm) and bool(m.training) for _, m in named)
    if not any(flags) or not initialized():
        return None, (False,) * len(named)
    return (g if g is not None else bn_group()), flags


def all_reduce(buf, group):
    """The cross-rank sum of one layer's fp64 totals (in place, on the current stream's order)."""
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError('SyncBatchNorm: a synchronised BatchNorm step cannot be captured into a graph (the all-reduce of its statistics '
                           'runs outside the capture); capture an unconverted model or put the layers in eval mode')
    dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)
