"""CPU: synchronised BatchNorm (nn.SyncBatchNorm) on the host side -- conversion keeps the model's parameters, buffers and state_dict; the
resolution of the synchronised layers (syncbn.resolve) follows torch's rules; the three kernel entry points are exported, declared in
include/clamd.h, bound in the ctypes table and check their arguments before any launch."""
import ctypes
import os
import re

import pytest
import torch
import torch.distributed as dist
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('clamd_bn_rows_total', 'clamd_bn_finalize_total', 'clamd_bn_bwd_finalize_total')


@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    return C


@pytest.fixture
def world1(tmp_path):
    """A gloo group of world size 1 in this process."""
    dist.init_process_group('gloo', init_method=f'file://{tmp_path}/pg', rank=0, world_size=1)
    try:
        yield
    finally:
        dist.destroy_process_group()


def _bns(model):
    return [(n, m) for n, m in model.named_modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)]


def test_convert_keeps_parameters_buffers_and_state_dict(C):
    torch.manual_seed(0)
    m = C.UNet(5, 3, 8)
    params = list(m.parameters())
    names = [n for n, _ in m.named_parameters()]
    bufs = dict(m.named_buffers())
    keys = list(m.state_dict().keys())
    assert len(keys) == 136
    m.enc3.block[3].eval()
    out = nn.SyncBatchNorm.convert_sync_batchnorm(m)
    assert out is m
    assert [n for n, _ in m.named_parameters()] == names
    assert all(a is b for a, b in zip(m.parameters(), params)) and len(list(m.parameters())) == len(params) == 82
    assert list(m.state_dict().keys()) == keys
    for n, b in m.named_buffers():
        assert b is bufs[n], n
    bns = _bns(m)
    assert len(bns) == 18 and all(type(b) is nn.SyncBatchNorm for _, b in bns)
    assert not m.enc3.block[3].training and m.enc3.block[6].training          # each layer keeps its mode
    assert C.ddp.convert_sync_batchnorm(C.UNet(5, 3, 8)).enc1[2].__class__ is nn.SyncBatchNorm


def test_resolve_without_process_group_does_nothing(C):
    assert not dist.is_initialized()
    m = nn.SyncBatchNorm.convert_sync_batchnorm(C.UNet(5, 3, 8))
    group, flags = C.syncbn.resolve(_bns(m))
    assert group is None and flags == (False,) * 18


def test_resolve_world1_group(C, world1):
    m = nn.SyncBatchNorm.convert_sync_batchnorm(C.UNet(5, 3, 8))
    group, flags = C.syncbn.resolve(_bns(m))
    assert flags == (True,) * 18
    # modules without a group: the dedicated BatchNorm group (not the default group GradSync reduces the gradients over), made once
    assert group is not None and group is not dist.group.WORLD
    assert dist.get_world_size(group) == 1
    assert C.syncbn.resolve(_bns(m))[0] is group
    # eval-mode layers are not synchronised; plain BatchNorm layers of a partly converted model neither
    m.enc2.block[3].eval()
    m.dec4.block[2] = nn.BatchNorm2d(8)
    names = [n for n, _ in _bns(m)]
    _, flags = C.syncbn.resolve(_bns(m))
    off = {n for n, f in zip(names, flags) if not f}
    assert off == {'enc2.block.3', 'dec4.block.2'}
    m.eval()
    assert C.syncbn.resolve(_bns(m)) == (None, (False,) * 18)
    # no SyncBatchNorm at all: nothing
    assert C.syncbn.resolve(_bns(C.UNet(5, 3, 8))) == (None, (False,) * 18)


def test_resolve_explicit_group_and_mixed_groups(C, world1):
    g1, g2 = dist.new_group(), dist.new_group()
    m = nn.SyncBatchNorm.convert_sync_batchnorm(C.UNet(5, 3, 8), g1)
    assert C.syncbn.resolve(_bns(m))[0] is g1
    m.dec2.block[5].process_group = g2
    m.last[2].process_group = None
    with pytest.raises(ValueError, match=r'dec2\.block\.5.*last\.2|last\.2.*dec2\.block\.5'):
        C.syncbn.resolve(_bns(m))
    m.dec2.block[5].eval()                    # a layer's mode does not excuse its group
    with pytest.raises(ValueError, match='process_group'):
        C.syncbn.resolve(_bns(m))


def test_trainer_config_flag(C):
    cfg = C.default_config()
    assert cfg.sync_bn is False


def test_sync_entry_points_exported_declared_and_bound(C):
    hdr = open(os.path.join(ROOT, 'include', 'clamd.h')).read()
    lib = ctypes.CDLL(C._lib.LIB_PATH)
    for n in NEW:
        assert re.search(r'\b%s\s*\(' % n, hdr), f'{n} not declared in include/clamd.h'
        assert hasattr(lib, n), f'{n} not exported by libclamd.so'
        assert n in C._lib.SIGNATURES, f'{n} missing from the ctypes table'


def test_sync_launchers_reject_bad_arguments_before_launching(C):
    """Every case is refused by a host check: status -1 (clamd_fail) with that check's own message.  A case that passed the checks would
    return -2 from the failed launch on a machine without a device, and fails here instead of reaching a kernel where there is one."""
    lib = C._lib.load()
    p = ctypes.c_void_p(0x1000)          # never dereferenced: every case below fails its checks on the host

    def refused(name, needle, *args):
        rc = getattr(lib, name)(*args)
        msg = lib.clamd_last_error().decode()
        assert rc == -1 and msg.startswith(name[len('clamd_'):] + ': ') and needle in msg, (name, args, rc, msg)

    for needle, rows, nrows, nk, Cp, count, tot, red in [('nk must be', p, 4, 3, 64, 8., p, p), ('nk must be', p, 4, 4, 64, 8., p, p),
                                                         ('nrows must be', p, 0, 2, 64, 8., p, p), ('nrows must be', None, 4, 2, 64, 8., p, p),
                                                         ('bad channel count', p, 4, 2, 60, 8., p, p),
                                                         ('nothing to write', p, 4, 5, 64, 8., None, None),
                                                         ('count must be positive', p, 4, 2, 64, 0., None, p)]:
        refused('clamd_bn_rows_total', needle, rows, nrows, nk, Cp, count, tot, red, None)
    for needle, red, Cp, C_, rm, rv in [('null argument', None, 64, 64, p, p), ('bad channel counts', p, 60, 60, p, p),
                                        ('bad channel counts', p, 64, 65, p, p), ('bad channel counts', p, 64, 0, p, p),
                                        ('running_mean and running_var go together', p, 64, 64, p, None)]:
        refused('clamd_bn_finalize_total', needle, red, p, p, rm, rv, p, p, p, p, Cp, C_, 0.1, 1e-5, None, None)
    # Cp = 48 is no case: the kernel is right for every multiple of 8 and the launcher takes it
    for needle, tot, red, Cp, C_ in [('null argument', None, p, 64, 64), ('null argument', p, None, 64, 64), ('bad channel counts', p, p, 60, 60),
                                     ('bad channel counts', p, p, 64, 65)]:
        refused('clamd_bn_bwd_finalize_total', needle, tot, red, p, p, p, p, p, p, None, Cp, C_, None)
