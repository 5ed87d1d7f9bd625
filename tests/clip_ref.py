"""Float64 NumPy restatement of clipping by the global gradient norm as clamd_grad_norm_clip computes it (torch.nn.utils.clip_grad_norm_,
norm_type 2, error_if_nonfinite off, applied to the gradient the step consumes), shared by test_clip_cpu.py, test_clip_grid_gpu.py and
test_clip_gpu.py.  Inputs may be fp32: everything is widened first.

    norm  = sqrt(sum over all tensors of sum g^2) * |grad_scale|
    coef  = min(1, max_norm / (norm + 1e-6)), a NaN norm giving NaN
    scale = grad_scale * coef          (what the step kernel multiplies every gradient by)"""
import numpy as np


def clip(grads, max_norm, grad_scale=1.0):
    """grads: list of arrays.  Returns dict(norm, tensor_norms, coef, scale), all float64."""
    gs = float(grad_scale)
    sums = [float((np.asarray(g, np.float64) ** 2).sum()) for g in grads]
    tensor_norms = np.sqrt(np.asarray(sums, np.float64)) * abs(gs)
    norm = float(np.sqrt(np.sum(np.asarray(sums, np.float64)))) * abs(gs)
    with np.errstate(invalid='ignore'):
        coef = np.float64(max_norm) / (np.float64(norm) + 1e-6)
    coef = float(coef) if np.isnan(coef) else min(1.0, float(coef))
    return dict(norm=norm, tensor_norms=tensor_norms, coef=coef, scale=gs * coef)


def clipped(grads, max_norm, grad_scale=1.0):
    """The gradients the step consumes: g * grad_scale * coef, float64."""
    s = clip(grads, max_norm, grad_scale)['scale']
    return [np.asarray(g, np.float64) * s for g in grads]
