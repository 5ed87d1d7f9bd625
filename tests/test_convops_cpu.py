"""The argument lists of continual-learning_amd/convops.py against the C ABI, without a GPU: every launch goes to a recorder instead of
the library, operands are plain integers.  Each recorded call must name an entry point of _lib.SIGNATURES, have as many arguments as its
signature and convert under every declared ctypes type; and per argument layout ONE literal tuple, written from the prototypes in
include/clamd.h (not from convops), pins where each operand and each geometry integer lands -- argument order is a condition of the ABI."""
import ctypes

import pytest

from continual_learning_amd import _lib, convops
from continual_learning_amd.plan import ALGOS

# operands: pointers 101.., every integer different so that a swap shows
X, V, WF, BIAS, Y, STATS, BN_Y, BN_SUMS, TUNE, S = 101, 102, 103, 104, 105, 106, 107, 108, 109, 110
X_LDC, Y_LDC, ROWS, FROWS, B, H, W, CIN_P, COUT_P, RELU, DT = 11, 12, 13, 14, 2, 16, 20, 64, 128, 3, 1
GZ, XW, VW, YT, WS, OUT = 201, 202, 203, 204, 205, 206
GZ_LDC, XW_LDC, WSB, RP, CP, R, C, SEG0, SEG0P = 21, 22, 4096, 128, 64, 120, 60, 30, 32
GEO = (B, H, W, CIN_P, COUT_P)
WGEO = (B, H, W, RP, CP, R, C, R, RP, SEG0, SEG0P)       # B, H, W, Rp, Cp, R, C, r_seg0, r_seg0p, c_seg0, c_seg0p


class Recorder:
    """`run(name, *args)` of convops: records, and checks the call against _lib.SIGNATURES."""

    def __init__(self):
        self.calls = []

    def __call__(self, name, *args):
        assert name in _lib.SIGNATURES, name
        argtypes = _lib.SIGNATURES[name][1]
        assert len(args) == len(argtypes), (name, len(args), len(argtypes))
        for i, (a, t) in enumerate(zip(args, argtypes)):
            try:
                t.from_param(a)
            except (TypeError, ctypes.ArgumentError) as e:
                raise AssertionError(f'{name}: argument {i} = {a!r} does not convert to {t.__name__}') from e
        self.calls.append((name, args))

    def only(self):
        assert len(self.calls) == 1, self.calls
        return self.calls.pop()


def test_recorder_refuses_what_ctypes_would_mangle():
    import torch
    rec = Recorder()
    good = [X, X_LDC, None, Y, Y_LDC, B, H, W, COUT_P, DT, S]
    rec('clamd_maxpool2x2', *good)
    for pos, bad in ((1, 11.0), (5, 2.0), (0, torch.zeros(1)), (10, torch.zeros(1))):     # a float for an int, a tensor for a pointer
        with pytest.raises(AssertionError, match=f'argument {pos} '):
            rec('clamd_maxpool2x2', *good[:pos], bad, *good[pos + 1:])
    with pytest.raises(AssertionError):
        rec('clamd_maxpool2x2', *good[:-1])
    with pytest.raises(AssertionError):
        rec('clamd_no_such_entry')


# forward with statistics rows / data gradient with the fused BatchNorm-backward sums (direct, pointwise) or plain (Winograd)
CONV = {
    # clamd_conv3x3(x, x_ldc, w_packed, bias, y, y_ldc, stats, bn_y, bn_sums, stat_rows, B, H, W, Cin_p, Cout_p, relu, m_fastest, dtype, tune, stream)
    'direct': ((X, X_LDC, WF, BIAS, Y, Y_LDC, STATS, None, None, ROWS, B, H, W, CIN_P, COUT_P, RELU, 1, DT, TUNE, S),
               (X, X_LDC, WF, None, Y, Y_LDC, None, BN_Y, BN_SUMS, FROWS, B, H, W, CIN_P, COUT_P, 0, 1, DT, TUNE, S)),
    # clamd_conv1x1(x, x_ldc, w_packed, bias, y, y_ldc, stats, bn_y, bn_sums, stat_rows, B, H, W, Cin_p, Cout_p, relu, dtype, stream)
    'pointwise': ((X, X_LDC, WF, BIAS, Y, Y_LDC, STATS, None, None, ROWS, B, H, W, CIN_P, COUT_P, RELU, DT, S),
                  (X, X_LDC, WF, None, Y, Y_LDC, None, BN_Y, BN_SUMS, FROWS, B, H, W, CIN_P, COUT_P, 0, DT, S)),
    # clamd_conv3x3_winograd*(x, x_ldc, w_wino, bias, y, y_ldc, stats, stat_rows, B, H, W, Cin_p, Cout_p, relu, tune, stream)
    'wino': ((X, X_LDC, WF, BIAS, Y, Y_LDC, STATS, ROWS, B, H, W, CIN_P, COUT_P, RELU, TUNE, S),
             (X, X_LDC, WF, None, Y, Y_LDC, None, 0, B, H, W, CIN_P, COUT_P, 0, TUNE, S)),
    # clamd_conv3x3_winograd*_pre(v, w_wino, bias, y, y_ldc, stats, stat_rows, B, H, W, Cin_p, Cout_p, relu, tune, stream)
    'pre': ((V, WF, BIAS, Y, Y_LDC, STATS, ROWS, B, H, W, CIN_P, COUT_P, RELU, TUNE, S),
            (V, WF, None, Y, Y_LDC, None, 0, B, H, W, CIN_P, COUT_P, 0, TUNE, S)),
}
WGRAD = {
    # clamd_wgrad(mode, a, a_ldc, b, b_ldc, workspace, ws_bytes, out, B, H, W, Rp, Cp, R, C, r_seg0, r_seg0p, c_seg0, c_seg0p, dtype, tune, stream)
    'direct': (0, GZ, GZ_LDC, XW, XW_LDC, WS, WSB, OUT) + WGEO + (DT, TUNE, S),
    # ... mode CLAMD_WGRAD_PW on the im2col'ed input: C and its first segment count the nine taps
    'pointwise': (1, GZ, GZ_LDC, XW, XW_LDC, WS, WSB, OUT, B, H, W, RP, CP, R, 540, R, RP, 270, SEG0P, DT, TUNE, S),
    # clamd_wgrad_winograd*(gz, gz_ldc, x, x_ldc, workspace, ws_bytes, out, B, H, W, Rp, Cp, R, C, r_seg0, r_seg0p, c_seg0, c_seg0p, tune, stream)
    'wino': (GZ, GZ_LDC, XW, XW_LDC, WS, WSB, OUT) + WGEO + (TUNE, S),
    # clamd_wgrad_winograd*_pre(gz, gz_ldc, v, yt, workspace, ws_bytes, out, B, H, W, Rp, Cp, R, C, r_seg0, r_seg0p, c_seg0, c_seg0p, tune, stream)
    'pre': (GZ, GZ_LDC, VW, YT, WS, WSB, OUT) + WGEO + (TUNE, S),
}


@pytest.mark.parametrize('family', sorted(ALGOS))
def test_unit_launches_of_every_family(family):
    algo, rec = ALGOS[family], Recorder()
    assert algo.layout in CONV
    fwd, dgrad = CONV[algo.layout]
    fused = (BN_Y, BN_SUMS, FROWS) if algo.layout in ('direct', 'pointwise') else None
    convops.conv3x3(rec, algo, X, X_LDC, V, WF, BIAS, Y, Y_LDC, STATS, ROWS, None, *GEO, RELU, DT, TUNE, S)
    assert rec.only() == (algo.conv, fwd)
    convops.conv3x3(rec, algo, X, X_LDC, V, WF, None, Y, Y_LDC, None, 0, fused, *GEO, 0, DT, TUNE, S)
    assert rec.only() == (algo.conv, dgrad)
    convops.conv3x3(rec, algo, X, X_LDC, V, WF, None, Y, Y_LDC, None, 0, None, *GEO, 0, DT, None, None)      # no statistics, no sums, NULL tuning and stream
    name, args = rec.only()
    assert len(args) == len(fwd) and BN_Y not in args and STATS not in args
    if fused is None:       # no epilogue for the sums: refused, not dropped
        with pytest.raises(ValueError):
            convops.conv3x3(rec, algo, X, X_LDC, V, WF, None, Y, Y_LDC, None, 0, (BN_Y, BN_SUMS, FROWS), *GEO, 0, DT, TUNE, S)
        assert not rec.calls
    if algo.wgrad is not None:
        for gz in ((GZ, None) if algo.pre else (GZ,)):       # None: the operand is already transformed
            convops.wgrad3x3(rec, algo, gz, GZ_LDC, XW, XW_LDC, VW, YT, WS, WSB, OUT, B, H, W, RP, CP, R, C, SEG0, SEG0P, DT, TUNE, S)
            want = WGRAD[algo.layout]
            assert rec.only() == (algo.wgrad, (gz,) + want[1:] if algo.pre else want)
    if algo.pre:
        # clamd_winograd*_transform_input(x, x_ldc, scale, shift, v, B, H, W, Cp, stream)
        for scale, shift in ((301, 302), (None, None)):
            convops.wino_transform(rec, algo, X, X_LDC, scale, shift, V, B, H, W, CIN_P, S)
            assert rec.only() == (algo.xform, (X, X_LDC, scale, shift, V, B, H, W, CIN_P, S))
        # clamd_wgrad_winograd*_pre_transform(gz, gz_ldc, yt, B, H, W, Rp, stream)
        convops.wgrad_transform(rec, algo, GZ, GZ_LDC, YT, B, H, W, RP, S)
        assert rec.only() == (algo.wg_xform, (GZ, GZ_LDC, YT, B, H, W, RP, S))


def test_grid_order_rule():
    assert convops.m_fastest(2, 16, 20, 128) == 1 and convops.m_fastest(2, 64, 64, 64) == 0
    assert convops.m_fastest(1, 24, 24, 64) == 0 and convops.m_fastest(1, 24, 24, 72) == 1      # 9 * 64 = 24 * 24: pixels fastest at a tie


CIN, COUT, DW, DB, LOGITS, PRED = 60, 120, 401, 402, 403, 404
TGEO = (B, H, W, CIN_P, COUT_P)


@pytest.mark.parametrize('fused', [None, (BN_Y, BN_SUMS, FROWS)])
def test_tails(fused):
    rec = Recorder()
    bn = fused or (None, None, 0)
    # clamd_convT2x2_fwd(x, x_ldc, w_packed, bias, y, y_ldc, B, h, w, Cin_p, Cout_p, dtype, stream)
    convops.convT_fwd(rec, X, X_LDC, WF, BIAS, Y, Y_LDC, *TGEO, DT, S)
    assert rec.only() == ('clamd_convT2x2_fwd', (X, X_LDC, WF, BIAS, Y, Y_LDC, B, H, W, CIN_P, COUT_P, DT, S))
    # clamd_conv1x1_logits(x, x_ldc, w_packed, bias, logits_nchw, B, H, W, Cin_p, Cout_p, num_classes, dtype, stream)
    convops.head_fwd(rec, X, X_LDC, WF, BIAS, LOGITS, None, *TGEO, COUT, DT, S)
    assert rec.only() == ('clamd_conv1x1_logits', (X, X_LDC, WF, BIAS, LOGITS, B, H, W, CIN_P, COUT_P, COUT, DT, S))
    # clamd_conv1x1_argmax(x, x_ldc, w_packed, bias, pred, logits_nchw, B, H, W, Cin_p, Cout_p, num_classes, dtype, stream)
    for logits in (None, LOGITS):
        convops.head_fwd(rec, X, X_LDC, WF, BIAS, logits, PRED, *TGEO, COUT, DT, S)
        assert rec.only() == ('clamd_conv1x1_argmax', (X, X_LDC, WF, BIAS, PRED, logits, B, H, W, CIN_P, COUT_P, COUT, DT, S))
    # clamd_convT2x2_dgrad(gy, gy_ldc, w_packed, gx, gx_ldc, bn_y, bn_sums, stat_rows, B, h, w, Cin_p, Cout_p, dtype, stream)
    convops.tail_dgrad(rec, 'convT', GZ, GZ_LDC, WF, OUT, X_LDC, fused, *TGEO, DT, S)
    assert rec.only() == ('clamd_convT2x2_dgrad', (GZ, GZ_LDC, WF, OUT, X_LDC) + bn + (B, H, W, CIN_P, COUT_P, DT, S))
    # the head's data gradient: clamd_conv1x1 from the Cout_p logits to the Cin_p input channels, no bias, ReLU or statistics
    convops.tail_dgrad(rec, 'head', GZ, GZ_LDC, WF, OUT, X_LDC, fused, *TGEO, DT, S)
    assert rec.only() == ('clamd_conv1x1', (GZ, GZ_LDC, WF, None, OUT, X_LDC, None) + bn + (B, H, W, COUT_P, CIN_P, 0, DT, S))
    # clamd_wgrad: CLAMD_WGRAD_UP2 (2) a = the layer's input, rows = Cin; CLAMD_WGRAD_PW (1) a = d logits, rows = K
    convops.tail_wgrad(rec, 'convT', X, X_LDC, GZ, GZ_LDC, WS, WSB, DW, B, H, W, CIN, CIN_P, COUT, COUT_P, DT, TUNE, S)
    assert rec.only() == ('clamd_wgrad', (2, X, X_LDC, GZ, GZ_LDC, WS, WSB, DW, B, H, W, CIN_P, COUT_P, CIN, COUT, CIN, CIN_P, COUT, COUT_P, DT, TUNE, S))
    convops.tail_wgrad(rec, 'head', X, X_LDC, GZ, GZ_LDC, WS, WSB, DW, B, H, W, CIN, CIN_P, COUT, COUT_P, DT, None, S)
    assert rec.only() == ('clamd_wgrad', (1, GZ, GZ_LDC, X, X_LDC, WS, WSB, DW, B, H, W, COUT_P, CIN_P, COUT, CIN, COUT, COUT_P, CIN, CIN_P, DT, None, S))
    # clamd_channel_sum(g, ldc, out, npix, Cp, C, dtype, workspace, ws_bytes, tune, stream): the convT gradient has 2h x 2w pixels
    for kind, npix in (('convT', B * 4 * H * W), ('head', B * H * W)):
        convops.tail_bias_grad(rec, kind, GZ, GZ_LDC, DB, B, H, W, COUT, COUT_P, DT, WS, WSB, TUNE, S)
        assert rec.only() == ('clamd_channel_sum', (GZ, GZ_LDC, DB, npix, COUT_P, COUT, DT, WS, WSB, TUNE, S))


def test_tail_workspace_covers_both_launches():
    lib = _lib.load()
    for kind, mode, rp, cp in (('convT', 2, 64, 32), ('head', 1, 32, 64)):
        want = max(lib.clamd_wgrad_workspace_bytes(mode, B, H, W, rp, cp, DT), lib.clamd_channel_sum_workspace_bytes(32))
        assert convops.tail_workspace_bytes(lib, kind, B, H, W, 64, 32, DT) == want > 0
    assert convops.workspace_floats(4096) == 1040


@pytest.mark.parametrize('gp, gp_ldc', [(None, 0), (501, 51)])      # the second gradient source: d pooled
def test_elementwise_launches(gp, gp_ldc):
    rec = Recorder()
    GA, GA_LDC, SC, SH, K012, SUMS, CP_, C_ = 601, 61, 602, 603, 604, 605, 64, 60
    # clamd_bn_apply(y, y_ldc, scale, shift, out, out_ldc, pooled, p_ldc, B, H, W, Cp, dtype, stream)
    for pooled, p_ldc in ((None, 0), (502, 52)):
        convops.bn_apply(rec, Y, Y_LDC, SC, SH, OUT, X_LDC, pooled, p_ldc, B, H, W, CP_, DT, S)
        assert rec.only() == ('clamd_bn_apply', (Y, Y_LDC, SC, SH, OUT, X_LDC, pooled, p_ldc, B, H, W, CP_, DT, S))
    # clamd_bn_bwd_reduce(ga, ga_ldc, gp, gp_ldc, y, y_ldc, scale, shift, sums, sum_rows, B, H, W, Cp, dtype, tune, stream)
    convops.bn_bwd_reduce(rec, GA, GA_LDC, gp, gp_ldc, Y, Y_LDC, SC, SH, SUMS, ROWS, B, H, W, CP_, DT, TUNE, S)
    assert rec.only() == ('clamd_bn_bwd_reduce', (GA, GA_LDC, gp, gp_ldc, Y, Y_LDC, SC, SH, SUMS, ROWS, B, H, W, CP_, DT, TUNE, S))
    # clamd_bn_bwd_apply(ga, ga_ldc, gp, gp_ldc, y, y_ldc, scale, shift, k012, gz, gz_ldc, B, H, W, Cp, dtype, stream)
    convops.bn_bwd_apply(rec, GA, GA_LDC, gp, gp_ldc, Y, Y_LDC, SC, SH, K012, GZ, GZ_LDC, B, H, W, CP_, DT, S)
    assert rec.only() == ('clamd_bn_bwd_apply', (GA, GA_LDC, gp, gp_ldc, Y, Y_LDC, SC, SH, K012, GZ, GZ_LDC, B, H, W, CP_, DT, S))
    # clamd_bn_bwd_apply_sums(ga, ga_ldc, y, y_ldc, k012, gz, gz_ldc, gz_rows, nrows, B, H, W, Cp, dtype, stream)
    convops.bn_bwd_apply_sums(rec, GA, GA_LDC, Y, Y_LDC, K012, GZ, GZ_LDC, SUMS, ROWS, B, H, W, CP_, DT, S)
    assert rec.only() == ('clamd_bn_bwd_apply_sums', (GA, GA_LDC, Y, Y_LDC, K012, GZ, GZ_LDC, SUMS, ROWS, B, H, W, CP_, DT, S))
    # clamd_bn_bwd_eval(ga, ga_ldc, gp, gp_ldc, y, y_ldc, scale, shift, gz, gz_ldc, rows, nrows, B, H, W, Cp, C, dtype, stream)
    convops.bn_bwd_eval(rec, GA, GA_LDC, gp, gp_ldc, Y, Y_LDC, SC, SH, GZ, GZ_LDC, SUMS, ROWS, B, H, W, CP_, C_, DT, S)
    assert rec.only() == ('clamd_bn_bwd_eval', (GA, GA_LDC, gp, gp_ldc, Y, Y_LDC, SC, SH, GZ, GZ_LDC, SUMS, ROWS, B, H, W, CP_, C_, DT, S))
    # clamd_maxpool2x2(x, x_ldc, sign, pooled, p_ldc, B, H, W, Cp, dtype, stream)
    for sign in (None, SC):
        convops.maxpool(rec, X, X_LDC, sign, 502, 52, B, H, W, CP_, DT, S)
        assert rec.only() == ('clamd_maxpool2x2', (X, X_LDC, sign, 502, 52, B, H, W, CP_, DT, S))
        # clamd_maxpool2x2_bwd(x, x_ldc, sign, gp, gp_ldc, gx, gx_ldc, B, H, W, Cp, dtype, stream)
        convops.maxpool_bwd(rec, X, X_LDC, sign, 501, 51, OUT, Y_LDC, B, H, W, CP_, DT, S)
        assert rec.only() == ('clamd_maxpool2x2_bwd', (X, X_LDC, sign, 501, 51, OUT, Y_LDC, B, H, W, CP_, DT, S))
