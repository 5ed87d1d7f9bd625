"""Float64 NumPy restatement of Synaptic Intelligence's three formulas as the tracked kernels of csrc/optim.hip compute them, shared by
test_path_cpu.py, test_path_grid_gpu.py and test_path_gpu.py.  Inputs may be fp32: everything is widened first.

    per step    g_task = grad * grad_scale;  omega += -g_task * (p_new - p_old)     (the gradient BEFORE weight decay and both pulls)
    boundary    importance = decay * importance + max(0, omega) / ((p - start)^2 + xi)

The Adam step is oracle.np_unet.adam_step fed the gradient with the pulls added, the SGD step tests/sgd_ref.sgd_step."""
import numpy as np

import sgd_ref
from oracle import np_unet

EPS = 2.0 ** -24
FLT_QUANTUM = 2.0 ** -149


def _f(a):
    return None if a is None else np.asarray(a, np.float64)


def adam_step_tracked(p, grad, m, v, omega, step, old=None, importance=None, *, lr, beta1=0.5, beta2=0.99, eps=1e-8, grad_scale=1.0,
                      l2_lambda=0.0, ewc_lambda=0.0):
    """One tracked Adam step; `step` is the 1-based count after the increment.  old None: no anchor; importance None: no consolidation
    pull.  Returns dict(p, m, v, omega, l2, ewc): l2 = sum d^2 and ewc = sum importance d^2 over the weights before the step."""
    p, grad, m, v, omega, old, importance = (_f(a) for a in (p, grad, m, v, omega, old, importance))
    g_task = grad * grad_scale
    g, l2, ewc = g_task, 0.0, 0.0
    if old is not None:
        d = p - old
        g = g + 2.0 * l2_lambda * d
        l2 = float((d * d).sum())
        if importance is not None:
            g = g + ewc_lambda * importance * d
            ewc = float((importance * d * d).sum())
    p1, m1, v1 = np_unet.adam_step(p, g, m, v, step, lr, beta1, beta2, eps)
    return dict(p=p1, m=m1, v=v1, omega=omega - g_task * (p1 - p), l2=l2, ewc=ewc)


def sgd_step_tracked(p, grad, buf, omega, old=None, importance=None, *, grad_scale=1.0, **kw):
    """One tracked SGD step (keywords of sgd_ref.sgd_step).  Returns its dict with `omega` added."""
    p, grad, omega = _f(p), _f(grad), _f(omega)
    ref = sgd_ref.sgd_step(p, grad, buf, old, importance, grad_scale=grad_scale, **kw)
    ref['omega'] = omega - (grad * grad_scale) * (ref['p'] - p)
    return ref


def path_importance(importance, omega, p, start, *, decay=1.0, xi=0.1):
    """The task boundary."""
    importance, omega, p, start = (_f(a) for a in (importance, omega, p, start))
    return decay * importance + np.maximum(omega, 0.0) / ((p - start) ** 2 + xi)


def omega_from_kernel_values(omega0, grad, grad_scale, p0, p1):
    """What the kernel has to leave in omega given ITS OWN fp32 input p0 and output p1: omega0 - (grad * f32(grad_scale)) * (p1 - p0) in
    float64, and the bound on |got - want|: 5 * 2^-24 * (|omega0| + |grad * gs * (p1 - p0)|) + 4 * 2^-149 -- four fp32 roundings (the
    scaled gradient, the difference, the product, the sum), one more for second-order terms, and the denormal quantum."""
    omega0, grad, p0, p1 = (_f(a) for a in (omega0, grad, p0, p1))
    term = (grad * float(np.float32(grad_scale))) * (p1 - p0)
    return omega0 - term, 5 * EPS * (np.abs(omega0) + np.abs(term)) + 4 * FLT_QUANTUM
