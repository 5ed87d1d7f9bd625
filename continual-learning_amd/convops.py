"""The argument lists of the convolution, BatchNorm-pass and pooling launches, once: the 3x3 unit in every kernel family of plan.ALGOS
(forward, data gradient, weight gradient, operand transforms), the two tail layers (ConvTranspose2d 2x2, the 1x1 head) and the elementwise
passes.  The UNet engine (engine.py) and the stand-alone blocks (blocks.py) both launch through here; tests/test_convops_cpu.py pins
every list against include/clamd.h.  Like bnops.py: nothing is allocated, callers own every buffer, `s` is the stream pointer.

`run(name, *args)`: the launcher -- `_lib.call`, or the engine's `_timed` / `_hbm` with tag, FLOPs and bytes bound.  Which stream, which
wait and what is timed stay with the caller; this module knows argument order only.
Operands are RAW device pointers (`_lib.ptr`; None = NULL); pitches and channel counts are in elements, `*_p` = padded.
`fused`: (bn_y, bn_sums, rows) of the BatchNorm-backward sums a data-gradient launch accumulates for the unit in front, or None."""
from . import _lib
from .plan import ALGOS


def m_fastest(B, H, W, cout_p):
    """Grid order of the direct 3x3 kernel: output channels fastest where the filters outweigh the pixels."""
    return 1 if 9 * cout_p > B * H * W else 0


def workspace_floats(nbytes):
    """fp32 elements of a weight-gradient / channel-sum workspace of `nbytes`, with the 16 floats of slack every caller has always added."""
    return nbytes // 4 + 16


# ---- one 3x3 unit: plan.Algo.layout picks the list
def conv3x3(run, algo, x, x_ldc, v, w, bias, y, y_ldc, stats, rows, fused, B, H, W, cin_p, cout_p, relu, dcode, tune, s):
    """Forward (w = forward filters, stats / rows = BatchNorm statistics rows or None) or data gradient (x = g_z, w = data-gradient filters,
    cin_p / cout_p exchanged) of family `algo`.  `v`: the transformed x a pre-transformed family reads instead of x; `bias`: [cout_p] or
    a folded BatchNorm's border-class table (relu 3)."""
    lay = algo.layout
    if lay == 'pre':
        if fused is None:
            return run(algo.conv, v, w, bias, y, y_ldc, stats, rows, B, H, W, cin_p, cout_p, relu, tune, s)
    elif lay == 'wino':
        if fused is None:
            return run(algo.conv, x, x_ldc, w, bias, y, y_ldc, stats, rows, B, H, W, cin_p, cout_p, relu, tune, s)
    else:
        bn_y, bn_sums, rows = fused or (None, None, rows)
        if lay == 'direct':
            return run(algo.conv, x, x_ldc, w, bias, y, y_ldc, stats, bn_y, bn_sums, rows, B, H, W, cin_p, cout_p, relu,
                       m_fastest(B, H, W, cout_p), dcode, tune, s)
        return run(algo.conv, x, x_ldc, w, bias, y, y_ldc, stats, bn_y, bn_sums, rows, B, H, W, cin_p, cout_p, relu, dcode, s)
    raise ValueError(f'{algo.conv}: the Winograd kernels have no BatchNorm-sums epilogue')


def wgrad3x3(run, algo, gz, gz_ldc, x, x_ldc, v, yt, ws, ws_bytes, out, B, H, W, Rp, Cp, R, C, c_seg0, c_seg0p, dcode, tune, s):
    """Weight gradient [R][C][3][3] of family `algo` into `out` (rows = output channels R / Rp, columns = input channels C / Cp, whose first
    concat segment is c_seg0 / c_seg0p).  Pre-transformed: `v` = the forward image, `yt` = the gradient-side operand, gz None = already there."""
    lay = algo.layout
    if lay == 'pre':
        run(algo.wgrad, gz, gz_ldc, v, yt, ws, ws_bytes, out, B, H, W, Rp, Cp, R, C, R, Rp, c_seg0, c_seg0p, tune, s)
    elif lay == 'wino':
        run(algo.wgrad, gz, gz_ldc, x, x_ldc, ws, ws_bytes, out, B, H, W, Rp, Cp, R, C, R, Rp, c_seg0, c_seg0p, tune, s)
    elif lay == 'direct':
        run(algo.wgrad, _lib.WGRAD_CONV3, gz, gz_ldc, x, x_ldc, ws, ws_bytes, out, B, H, W, Rp, Cp, R, C, R, Rp, c_seg0, c_seg0p, dcode, tune, s)
    else:      # im2col: x holds the 3x3 neighbourhoods, [R][C * 9] is already the (c * 9 + tap) K order of a pointwise weight gradient
        run(algo.wgrad, _lib.WGRAD_PW, gz, gz_ldc, x, x_ldc, ws, ws_bytes, out, B, H, W, Rp, Cp, R, 9 * C, R, Rp, 9 * c_seg0, c_seg0p, dcode, tune, s)


def wino_transform(run, algo, x, x_ldc, scale, shift, v, B, H, W, Cp, s):
    """x -> v of a pre-transformed family: the forward image (scale / shift: the BatchNorm in front, or None) or the data-gradient operand."""
    run(algo.xform, x, x_ldc, scale, shift, v, B, H, W, Cp, s)


def wgrad_transform(run, algo, gz, gz_ldc, yt, B, H, W, Rp, s):
    """gz -> yt, the gradient-side operand of a pre-transformed weight gradient."""
    run(algo.wg_xform, gz, gz_ldc, yt, B, H, W, Rp, s)


# ---- the tails: kind -> (clamd_wgrad mode, the layer's INPUT is the row operand, output pixels per input pixel); H, W: the input grid
_TAIL = {'convT': (_lib.WGRAD_UP2, True, 4), 'head': (_lib.WGRAD_PW, False, 1)}


def convT_fwd(run, x, x_ldc, w, bias, y, y_ldc, B, H, W, cin_p, cout_p, dcode, s):
    run('clamd_convT2x2_fwd', x, x_ldc, w, bias, y, y_ldc, B, H, W, cin_p, cout_p, dcode, s)


def head_fwd(run, x, x_ldc, w, bias, logits, pred, B, H, W, cin_p, kp, k, dcode, s):
    """fp32 NCHW logits; with `pred` (int64 [B,H,W]) the arg-max from the epilogue, and logits only if a buffer is given."""
    if pred is None:
        run('clamd_conv1x1_logits', x, x_ldc, w, bias, logits, B, H, W, cin_p, kp, k, dcode, s)
    else:
        run('clamd_conv1x1_argmax', x, x_ldc, w, bias, pred, logits, B, H, W, cin_p, kp, k, dcode, s)


def tail_dgrad(run, kind, g, g_ldc, w, gx, gx_ldc, fused, B, H, W, cin_p, cout_p, dcode, s):
    if kind == 'convT':
        bn_y, bn_sums, rows = fused or (None, None, 0)
        run('clamd_convT2x2_dgrad', g, g_ldc, w, gx, gx_ldc, bn_y, bn_sums, rows, B, H, W, cin_p, cout_p, dcode, s)
    else:
        conv3x3(run, ALGOS['im2col'], g, g_ldc, None, w, None, gx, gx_ldc, None, 0, fused, B, H, W, cout_p, cin_p, 0, dcode, None, s)


def tail_workspace_bytes(lib, kind, B, H, W, cin_p, cout_p, dcode):
    """What tail_wgrad and tail_bias_grad need of their shared workspace."""
    mode, x_rows, _ = _TAIL[kind]
    rp, cp = (cin_p, cout_p) if x_rows else (cout_p, cin_p)
    return max(lib.clamd_wgrad_workspace_bytes(mode, B, H, W, rp, cp, dcode), lib.clamd_channel_sum_workspace_bytes(cout_p))


def tail_wgrad(run, kind, x, x_ldc, g, g_ldc, ws, ws_bytes, dw, B, H, W, cin, cin_p, cout, cout_p, dcode, tune, s):
    """d weight in the parameter's own layout: [Cin][Cout][2][2] (convT) or [K][Cin][1][1] (head) from the layer's input x and output gradient g."""
    mode, x_rows, _ = _TAIL[kind]
    if x_rows:
        run('clamd_wgrad', mode, x, x_ldc, g, g_ldc, ws, ws_bytes, dw, B, H, W, cin_p, cout_p, cin, cout, cin, cin_p, cout, cout_p, dcode, tune, s)
    else:
        run('clamd_wgrad', mode, g, g_ldc, x, x_ldc, ws, ws_bytes, dw, B, H, W, cout_p, cin_p, cout, cin, cout, cout_p, cin, cin_p, dcode, tune, s)


def tail_bias_grad(run, kind, g, g_ldc, db, B, H, W, cout, cout_p, dcode, ws, ws_bytes, tune, s):
    run('clamd_channel_sum', g, g_ldc, db, B * _TAIL[kind][2] * H * W, cout_p, cout, dcode, ws, ws_bytes, tune, s)


# ---- elementwise passes; gp / gp_ldc: the second gradient source (d pooled, routed to its window's maximum), or None / 0
def bn_apply(run, y, y_ldc, scale, shift, out, out_ldc, pooled, p_ldc, B, H, W, Cp, dcode, s):
    """out = scale * y + shift at any pitch (concat placement) and, with `pooled`, its 2x2 max-pool."""
    run('clamd_bn_apply', y, y_ldc, scale, shift, out, out_ldc, pooled, p_ldc, B, H, W, Cp, dcode, s)


def bn_bwd_reduce(run, ga, ga_ldc, gp, gp_ldc, y, y_ldc, scale, shift, sums, rows, B, H, W, Cp, dcode, tune, s):
    run('clamd_bn_bwd_reduce', ga, ga_ldc, gp, gp_ldc, y, y_ldc, scale, shift, sums, rows, B, H, W, Cp, dcode, tune, s)


def bn_bwd_apply(run, ga, ga_ldc, gp, gp_ldc, y, y_ldc, scale, shift, k012, gz, gz_ldc, B, H, W, Cp, dcode, s):
    run('clamd_bn_bwd_apply', ga, ga_ldc, gp, gp_ldc, y, y_ldc, scale, shift, k012, gz, gz_ldc, B, H, W, Cp, dcode, s)


def bn_bwd_apply_sums(run, ga, ga_ldc, y, y_ldc, k012, gz, gz_ldc, gz_rows, nrows, B, H, W, Cp, dcode, s):
    """The two-sum form: no pooling, and the partial rows of sum g_z (the conv-bias gradient) beside g_z."""
    run('clamd_bn_bwd_apply_sums', ga, ga_ldc, y, y_ldc, k012, gz, gz_ldc, gz_rows, nrows, B, H, W, Cp, dcode, s)


def bn_bwd_eval(run, ga, ga_ldc, gp, gp_ldc, y, y_ldc, scale, shift, gz, gz_ldc, part, nrows, B, H, W, Cp, C, dcode, s):
    run('clamd_bn_bwd_eval', ga, ga_ldc, gp, gp_ldc, y, y_ldc, scale, shift, gz, gz_ldc, part, nrows, B, H, W, Cp, C, dcode, s)


def maxpool(run, x, x_ldc, sign, pooled, p_ldc, B, H, W, Cp, dcode, s):
    """`sign`: per-channel scale whose sign picks max or min (a BatchNorm folded into the readers), or None."""
    run('clamd_maxpool2x2', x, x_ldc, sign, pooled, p_ldc, B, H, W, Cp, dcode, s)


def maxpool_bwd(run, x, x_ldc, sign, gp, gp_ldc, gx, gx_ldc, B, H, W, Cp, dcode, s):
    run('clamd_maxpool2x2_bwd', x, x_ldc, sign, gp, gp_ldc, gx, gx_ldc, B, H, W, Cp, dcode, s)
