"""The generalised per-pixel cross-entropy of include/clamd.h (clamd_ce_class_fwd_bwd) restated in torch, in the dtype of the logits: class
weights, label smoothing, the focal term, image weights.  Loss parts from closed formulas, the gradient from its closed form (no autograd),
and the per-pixel gradient scale the GPU tests measure errors in.  float64: the reference.  float32: the restatement the bound of
tests/test_wce_grid_gpu.py is derived from."""
from types import SimpleNamespace

import torch


def wce(z, y, w=None, nu=None, eps=0.0, gamma=0.0, ignore_index=-100):
    """z [B,K,H,W] floating, y int64 [B,H,W], w [K] (None: ones), nu [B] (None: ones).  -> namespace:
    l3 = [loss, (1 - eps) nll / D, (eps / K) smo / D] (0-d tensors), grad = d loss / d z, s_px [B,H,W], D, W, valid, nvalid, nbad."""
    if eps > 0 and gamma > 0:
        raise ValueError('label smoothing and the focal term together are not defined')
    B, K = z.shape[:2]
    dt = z.dtype
    w = torch.ones(K, dtype=dt, device=z.device) if w is None else w.to(dt)
    nu = torch.ones(B, dtype=dt, device=z.device) if nu is None else nu.to(dt)
    inr = (y >= 0) & (y < K)
    valid = (y != ignore_index) & inr
    yc = y.clamp(0, K - 1)
    hot = torch.nn.functional.one_hot(yc, K).permute(0, 3, 1, 2).to(dt)
    lp = torch.log_softmax(z, 1)
    p = lp.exp()
    py = (p * hot).sum(1)
    q = (p * (1 - hot)).sum(1)                                   # summed over the other classes, never 1 - p_y
    # t = -log p_y; through q where q is small: t / q below needs t to an ulp of t, and -log_softmax rounds at the size of the logits
    t = torch.where(q < 0.5, -torch.log1p(-q), -(lp * hot).sum(1))
    wy = w[yc]
    v = valid.to(dt)
    nub = nu[:, None, None]
    D = (wy * v).sum()
    W = w.sum()
    qg = q ** gamma if gamma > 0 else torch.ones_like(q)
    nll = (v * nub * wy * qg * t).sum()
    smo = (v * nub * (w[None, :, None, None] * -lp).sum(1)).sum()
    ratio = torch.where(q > 0, t / torch.where(q > 0, q, torch.ones_like(q)), torch.ones_like(q))
    f = qg * (1 + gamma * py * ratio) if gamma > 0 else torch.ones_like(q)
    if float(D) > 0:
        parts = [(1 - eps) * nll / D, (eps / K) * smo / D]
        c = v * nub / D
    else:                                                         # the library's convention where torch gives NaN
        parts = [z.new_zeros(()), z.new_zeros(())]
        c = torch.zeros_like(v)
    grad = c[:, None] * ((1 - eps) * (wy * f)[:, None] * (p - hot) + (eps / K) * (W * p - w[None, :, None, None]))
    s_px = torch.maximum(c * ((1 - eps) * wy * f + eps * W / K), 2.0 ** -40 * c * wy)
    return SimpleNamespace(l3=[parts[0] + parts[1], parts[0], parts[1]], grad=grad, s_px=s_px, D=D, W=W, valid=valid,
                           nvalid=int(valid.sum()), nbad=int(((y != ignore_index) & ~inr).sum()))


def focal_by_autograd(z, y, w, gamma, ignore_index=-100):
    """loss and d loss / d z of the focal form by autograd through q^gamma * t with t = -log_softmax(z)_y (float64 only: in float32 this
    cancels terms gamma * t times larger than the result)."""
    K = z.shape[1]
    zz = z.detach().clone().requires_grad_()
    valid = (y != ignore_index) & (y >= 0) & (y < K)
    yc = y.clamp(0, K - 1)
    hot = torch.nn.functional.one_hot(yc, K).permute(0, 3, 1, 2).to(z.dtype)
    lp = torch.log_softmax(zz, 1)
    q = (lp.exp() * (1 - hot)).sum(1)
    t = -(lp * hot).sum(1)
    wy = w.to(z.dtype)[yc] * valid
    loss = (wy * q ** gamma * t).sum() / wy.sum()
    g, = torch.autograd.grad(loss, zz)
    return loss.detach(), g
