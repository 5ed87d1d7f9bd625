"""A numpy restatement of clamd_augment_batch's definition (include/clamd.h), the yardstick of tests/test_augment_*.py.

Coordinates are Python integers (unbounded, so nothing can wrap), the weights and the interpolation float64, labels taken by index.  Written
from the definition alone: per axis a list of (inside, nearest, tap0, tap1, weight) over the output pixels, then three lerps on gathered planes.
"""
import numpy as np

STEP_MIN, STEP_MAX = 1 << 13, 1 << 19


def axis(origin, step, N, flip=False):
    """Output pixel k of an axis of N pixels -> arrays inside [N] bool, nearest [N], tap0 [N], tap1 [N] (int64) and weight [N] (float64)."""
    inside, near, t0, t1, w = [], [], [], [], []
    for k in range(N):
        j = N - 1 - k if flip else k
        s = int(origin) + j * int(step)
        ins = 0 <= s + 32768 < N * 65536
        inside.append(ins)
        near.append((s + 32768) >> 16 if ins else 0)
        f = s >> 16                                   # Python's >> floors, like an arithmetic shift
        t0.append(min(max(f, 0), N - 1))
        t1.append(min(max(f + 1, 0), N - 1))
        w.append((s & 65535) / 65536.0)
    return np.array(inside, bool), np.array(near, np.int64), np.array(t0, np.int64), np.array(t1, np.int64), np.array(w, np.float64)


def augment_ref(images, labels, params, fill=0.0, ignore_index=-100):
    """images [B, C, H, W] (any float dtype) or None, labels int64 [B, H, W] or None, params: B rows of (step, y0, x0, flags) as Python ints
    -> (out_images float64 or None, out_labels int64 or None, inside bool [B, H, W], M float64 [B, C, H, W] or None).  M is the largest
    magnitude among each element's four taps (0 outside): what the error bound of the fp32 kernel scales with."""
    ref = labels if labels is not None else images
    B, H, W = ref.shape[0], ref.shape[-2], ref.shape[-1]
    inside = np.zeros((B, H, W), bool)
    out_x = M = out_y = None
    if images is not None:
        x = np.asarray(images, np.float64)
        out_x = np.full(x.shape, float(np.float32(fill)), np.float64)
        M = np.zeros(x.shape, np.float64)
    if labels is not None:
        out_y = np.full(labels.shape, ignore_index, np.int64)
    for b in range(B):
        step, y0, x0, flags = (int(v) for v in params[b])
        if not STEP_MIN <= step <= STEP_MAX:
            continue
        iy, ny, r0, r1, wy = axis(y0, step, H)
        ix, nx, c0, c1, wx = axis(x0, step, W, flip=bool(flags & 1))
        ins = iy[:, None] & ix[None, :]
        inside[b] = ins
        if labels is not None:
            out_y[b] = np.where(ins, np.asarray(labels[b])[ny[:, None], nx[None, :]], ignore_index)
        if images is not None:
            ta, tb = x[b][:, r0[:, None], c0[None, :]], x[b][:, r0[:, None], c1[None, :]]
            tc, td = x[b][:, r1[:, None], c0[None, :]], x[b][:, r1[:, None], c1[None, :]]
            top = ta + wx[None, None, :] * (tb - ta)
            bot = tc + wx[None, None, :] * (td - tc)
            out_x[b] = np.where(ins[None], top + wy[None, :, None] * (bot - top), out_x[b])
            M[b] = np.where(ins[None], np.maximum(np.maximum(np.abs(ta), np.abs(tb)), np.maximum(np.abs(tc), np.abs(td))), 0.0)
    return out_x, out_y, inside, M
