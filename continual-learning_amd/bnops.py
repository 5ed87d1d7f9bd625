"""The BatchNorm finalize launch sequences, once: statistics rows -> scale / shift (forward) and backward sums -> k0, k1, k2 and the parameter
gradients (backward), each plain, synchronised (the sums of the global batch, syncbn.py) and eval-mode (running statistics).  The UNet
engine (engine.py) and the stand-alone blocks (blocks.py) both launch them through here.  Nothing is allocated: callers own every buffer.

`v`: the unit's seven per-channel rows (scale, shift, mean, istd, k0, k1, k2; rows 4-6 contiguous), any sequence of [Cout_p] fp32 tensors.
`dgamma`, `dbeta`, `dbias`: RAW device pointers (the engine writes into its flat gradient buffer); `dbias` None = not written here.
`s`: the stream pointer of every launch."""
from . import syncbn
from ._lib import call, ptr

BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def fwd_finalize(stats, rows, gamma, beta, rm, rv, nbt, v, cout_p, cout, count, training, s, sync_red=None, group=None):
    """v[0..3] of one BatchNorm over `count` pixels per channel.  Train mode: from the forward launch's partial rows `stats`, running
    statistics and num_batches_tracked updated inside the launch; with `sync_red` (fp64 [2 Cout_p + 1] scratch) this rank's totals and
    pixel count are summed over `group` first.  Eval mode: from the running statistics, nothing updated."""
    if training and sync_red is not None:
        call('clamd_bn_rows_total', ptr(stats), rows, 2, cout_p, count, None, ptr(sync_red), s)
        syncbn.all_reduce(sync_red, group)
        call('clamd_bn_finalize_total', ptr(sync_red), ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(v[0]), ptr(v[1]), ptr(v[2]), ptr(v[3]),
             cout_p, cout, BN_MOMENTUM, BN_EPS, ptr(nbt), s)
        return
    call('clamd_bn_finalize', ptr(stats) if training else None, rows, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(v[0]), ptr(v[1]), ptr(v[2]),
         ptr(v[3]), cout_p, cout, count, BN_MOMENTUM, BN_EPS, ptr(nbt) if training else None, s)


def bwd_finalize(sums, rows, nsums, gamma, v, dgamma, dbeta, dbias, cout_p, cout, count, s, sync=None, group=None):
    """Train mode: k0, k1, k2 (v[4..6]) and d gamma, d beta, d conv-bias from the partial rows `sums` [rows][nsums][Cout_p].  `sync` = fp64
    (totals [nsums][Cout_p], reduced [2 Cout_p + 1]) scratch: k0-k2 from sum g, sum g y and the count of all ranks of `group` (the collective
    sits between the sums and the apply pass), the parameter gradients from this rank's totals, as torch."""
    if sync is None:
        call('clamd_bn_bwd_finalize', ptr(sums), rows, ptr(gamma), ptr(v[2]), ptr(v[3]), ptr(v[4]), dgamma, dbeta, dbias, cout_p, cout, count, s)
        return
    tot, red = sync
    call('clamd_bn_rows_total', ptr(sums), rows, nsums, cout_p, count, ptr(tot), ptr(red), s)
    syncbn.all_reduce(red, group)
    call('clamd_bn_bwd_finalize_total', ptr(tot), ptr(red), ptr(gamma), ptr(v[2]), ptr(v[3]), ptr(v[4]), dgamma, dbeta, dbias, cout_p, cout, s)


def bwd_eval_finalize(part, rows, per_row, v, write_k, dgamma, dbeta, dbias, cout_p, cout, s):
    """Eval mode: the parameter gradients from `part` [rows][per_row][Cout_p] -- the three rows of clamd_bn_bwd_eval, or the sums a producing
    data-gradient launch accumulated; `write_k`: also k0 = scale, k1 = k2 = 0 into v[4..6], for the apply passes of train mode."""
    call('clamd_bn_bwd_eval_finalize', ptr(part), rows, per_row, ptr(v[0]), ptr(v[2]), ptr(v[3]), ptr(v[4]) if write_k else None,
         dgamma, dbeta, dbias, cout_p, cout, s)
