"""Float64 NumPy restatement of the per-element formula of clamd_sgd_step (torch.optim.SGD with dampening 0 and maximize off, plus the two
build-defined pulls towards an anchor), shared by test_sgd_cpu.py and test_sgd_gpu.py.  Inputs may be fp32: everything is widened first."""
import numpy as np

EPS = 2.0 ** -24


def sgd_step(p, grad, buf=None, old=None, omega=None, *, lr, momentum=0.0, weight_decay=0.0, nesterov=False, grad_scale=1.0,
             decay_mult=1.0, l2_lambda=0.0, ewc_lambda=0.0):
    """One step.  buf None: no momentum buffer; old None: no anchor; omega None: no importance.  Returns dict(p, buf, l2, ewc, A, S):
    the new parameter and buffer (None without one), sum d^2 and sum omega d^2, and the magnitudes the error bounds are built from:
    A = |gs g| + wd |p| + 2 l2 |d| + ewc omega |d| and S = mu |buf| + A."""
    f = lambda a: None if a is None else np.asarray(a, np.float64)
    p, grad, buf, old, omega = f(p), f(grad), f(buf), f(old), f(omega)
    wd = float(weight_decay) * float(decay_mult)
    g = grad * grad_scale
    A = np.abs(g) + wd * np.abs(p)
    g = g + wd * p
    l2 = ewc = 0.0
    if old is not None:
        d = p - old
        g = g + 2.0 * l2_lambda * d
        A = A + 2.0 * l2_lambda * np.abs(d)
        l2 = float((d * d).sum())
        if omega is not None:
            g = g + ewc_lambda * omega * d
            A = A + ewc_lambda * omega * np.abs(d)
            ewc = float((omega * d * d).sum())
    S = A.copy()
    if buf is not None:
        S = momentum * np.abs(buf) + A
        buf = momentum * buf + g
        u = g + momentum * buf if nesterov else buf
    else:
        u = g
    return dict(p=p - lr * u, buf=buf, l2=l2, ewc=ewc, A=A, S=S)


def bounds(p_old, ref, *, lr, momentum):
    """The per-element bounds on |buf - ref| and |p - ref| from the number of fp32 roundings (E = 2^-24): at most 9 in the gradient, 2 in the
    buffer, 3 in the Nesterov combination and 2 in the update, with slack."""
    buf_bound = 12 * EPS * ref['S']
    p_bound = EPS * (np.abs(np.asarray(p_old, np.float64)) + np.abs(ref['p'])) + 32 * EPS * lr * (1 + momentum) * ref['S']
    return buf_bound, p_bound
