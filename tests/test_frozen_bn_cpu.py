"""CPU: the entry points of the eval-mode BatchNorm backward (frozen statistics) are exported, declared in include/clamd.h and bound in the
ctypes table, and their argument checks answer before any launch."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('clamd_bn_bwd_eval_rows', 'clamd_bn_bwd_eval', 'clamd_bn_bwd_eval_finalize')


@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    return C


def test_eval_bn_backward_symbols_exported_declared_and_bound(C):
    hdr = open(os.path.join(ROOT, 'include', 'clamd.h')).read()
    lib = ctypes.CDLL(C._lib.LIB_PATH)
    for n in NEW:
        assert re.search(r'\b%s\s*\(' % n, hdr), f'{n} not declared in include/clamd.h'
        assert hasattr(lib, n), f'{n} not exported by libclamd.so'
        assert n in C._lib.SIGNATURES, f'{n} missing from the ctypes table'
    C._lib.load()


def test_eval_rows_rejects_bad_sizes(C):
    lib = C._lib.load()
    assert lib.clamd_bn_bwd_eval_rows(2, 32, 48, 64, 0) > 0
    assert lib.clamd_bn_bwd_eval_rows(2, 32, 48, 64, 1) > 0
    assert lib.clamd_bn_bwd_eval_rows(2, 32, 48, 64, 1) <= lib.clamd_bn_bwd_eval_rows(2, 32, 48, 64, 0)
    # few channels: one row per 256 / (Cp / 8) pixels up to the cap; many channels: the cap shrinks with Cp (bounded row bytes)
    assert lib.clamd_bn_bwd_eval_rows(1, 8, 8, 64, 0) == 2
    assert lib.clamd_bn_bwd_eval_rows(16, 256, 256, 64, 0) == 2048
    assert lib.clamd_bn_bwd_eval_rows(16, 16, 16, 1024, 0) == 256
    for needle, args in [('bad sizes', (2, 32, 48, 48, 0)), ('bad sizes', (2, 32, 48, 4096, 0)), ('bad sizes', (2, 32, 48, 16, 0)),
                         ('bad sizes', (0, 32, 48, 64, 0)), ('bad sizes', (2, 0, 48, 64, 0)), ('bad sizes', (2, 32, -4, 64, 0)),
                         ('pooling needs even H, W', (2, 31, 48, 64, 1)), ('pooling needs even H, W', (2, 32, 47, 64, 1))]:
        assert lib.clamd_bn_bwd_eval_rows(*args) == -1, args
        assert 'bn_bwd_eval_rows: ' + needle in lib.clamd_last_error().decode(), args


def test_eval_launchers_reject_bad_arguments_before_launching(C):
    """Every case is refused by a host check: status -1 (clamd_fail) with that check's own message; a case that passed the checks would
    return -2 from the failed launch on a machine without a device."""
    L = C._lib
    lib = L.load()
    p = ctypes.c_void_p(0x1000)          # never dereferenced: every case below fails its checks on the host
    nr = lib.clamd_bn_bwd_eval_rows(2, 8, 8, 64, 0)
    nrp = lib.clamd_bn_bwd_eval_rows(2, 8, 8, 64, 1)          # pooled: the row count of the pooled grid, even H and W
    bad = [
        ('0 < C <= Cp', dict(Cp=48)), ('0 < C <= Cp', dict(C=65)), ('0 < C <= Cp', dict(C=0)), ('nrows must be', dict(nrows=nr + 1)),
        ('null argument', dict(ga=None)), ('pitches must be >= Cp', dict(y_ldc=32)), ('pitches must be >= Cp', dict(ga_ldc=32)),
        ('bad dtype', dict(dtype=7)), ('bad sizes', dict(B=0)),
        ('pooling needs even H, W', dict(gp=p, gp_ldc=64, nrows=nrp, W=7)), ('null argument', dict(gp=p, gp_ldc=64, nrows=nrp, shift=None)),
    ]
    for needle, b in bad:
        a = dict(ga=p, ga_ldc=64, gp=None, gp_ldc=0, y=p, y_ldc=64, scale=p, shift=p, gz=p, gz_ldc=64, rows=p, nrows=nr,
                 B=2, H=8, W=8, Cp=64, C=64, dtype=L.F32)
        a.update(b)
        rc = lib.clamd_bn_bwd_eval(a['ga'], a['ga_ldc'], a['gp'], a['gp_ldc'], a['y'], a['y_ldc'], a['scale'], a['shift'], a['gz'], a['gz_ldc'],
                                   a['rows'], a['nrows'], a['B'], a['H'], a['W'], a['Cp'], a['C'], a['dtype'], None)
        msg = lib.clamd_last_error().decode()
        assert rc == -1 and 'bn_bwd_eval: ' in msg and needle in msg, (b, rc, msg)
    # finalize: 3 (one-pass rows) or 5 (producer rows) sums only, C <= Cp, rows present
    for needle, nsums, nrows, Cp, C_ in [('nsums must be', 4, 8, 64, 64), ('nsums must be', 2, 8, 64, 64), ('nrows must be', 3, 0, 64, 64),
                                         ('bad channel counts', 3, 8, 64, 65), ('bad channel counts', 5, 8, 60, 60)]:
        rc = lib.clamd_bn_bwd_eval_finalize(p, nrows, nsums, p, p, p, None, p, p, p, Cp, C_, None)
        msg = lib.clamd_last_error().decode()
        assert rc == -1 and 'bn_bwd_eval_finalize: ' + needle in msg, (nsums, nrows, Cp, C_, rc, msg)
    rc = lib.clamd_bn_bwd_eval_finalize(p, 8, 3, None, p, p, None, p, p, p, 64, 64, None)
    assert rc == -1 and 'bn_bwd_eval_finalize: null argument' in lib.clamd_last_error().decode()
