"""Cross-entropy + soft Dice as include/clamd.h defines it, in plain torch (any floating dtype, any device; no libclamd): the reference of
tests/test_dice_cpu.py and tests/test_dice_gpu.py.

Two independent statements:
  dice_ce(z, y, ...)            -> (total, ce, dice), the loss itself, to be differentiated by autograd;
  coefficients / closed_form    the header's closed form of the gradient: the per-group table {c_gk, a_gk} and
                                d total / d z_j = w_ce (p_j - [y = j]) / max(N, 1) + p_j (g_j - sum_k p_k g_k),  g_k = c_gk + [y = k] a_gk.
test_dice_cpu.py holds the second to the first in float64.  pixel_scale is the per-pixel gradient scale s_px of the GPU test's bound."""
import torch


def _valid(y, K, ignore_index):
    return (y != ignore_index) & (y >= 0) & (y < K)


def _one_hot(y, K, valid, dtype):
    return torch.nn.functional.one_hot(y.clamp(0, K - 1), K).permute(0, 3, 1, 2).to(dtype) * valid[:, None]


def group_sums(p, y, ignore_index=-100, per_image=False):
    """I, P, Y [G, K] of the probabilities p [B, K, H, W] over the valid pixels of each group (G = B with per_image, else 1)."""
    K = p.shape[1]
    valid = _valid(y, K, ignore_index)
    oh = _one_hot(y, K, valid, p.dtype)
    pv = p * valid[:, None]
    I, P, Y = (pv * oh).sum((2, 3)), pv.sum((2, 3)), oh.sum((2, 3))
    if not per_image:
        I, P, Y = I.sum(0, keepdim=True), P.sum(0, keepdim=True), Y.sum(0, keepdim=True)
    return I, P, Y


def class_set(Y, first_class=0, present_only=True):
    """S_g as a bool mask [G, K]."""
    K = Y.shape[1]
    S = torch.arange(K, device=Y.device)[None, :] >= first_class
    S = S.expand_as(Y)
    return S & (Y > 0) if present_only else S.clone()


def dice_ce(z, y, w_ce=1.0, w_dice=1.0, smooth=1e-5, first_class=0, present_only=True, per_image=False, ignore_index=-100):
    """-> (total, w_ce * CE, w_dice * L_dice), differentiable in z."""
    K = z.shape[1]
    valid = _valid(y, K, ignore_index)
    n = max(int(valid.sum()), 1)
    logp = torch.log_softmax(z, 1)
    nll = -(logp.gather(1, y.clamp(0, K - 1)[:, None])[:, 0]) * valid
    ce = nll.sum() / n
    I, P, Y = group_sums(torch.softmax(z, 1), y, ignore_index, per_image)
    S = class_set(Y, first_class, present_only)
    N, D = 2 * I + smooth, P + Y + smooth
    ok = D != 0
    dice = torch.where(ok, N / torch.where(ok, D, torch.ones_like(D)), torch.ones_like(D))
    nS = S.sum(1)
    term = torch.where(nS > 0, 1 - (dice * S).sum(1) / nS.clamp(min=1), torch.zeros_like(dice[:, 0]))
    L = term.mean()
    ce_w, dice_w = w_ce * ce, w_dice * L
    return ce_w + dice_w, ce_w, dice_w


def coefficients(z, y, w_dice=1.0, smooth=1e-5, first_class=0, present_only=True, per_image=False, ignore_index=-100):
    """The header's table: c, a [G, K] (zero outside S_g and where D == 0) and |S_g| [G], from softmax(z) in z's dtype."""
    I, P, Y = group_sums(torch.softmax(z, 1), y, ignore_index, per_image)
    S = class_set(Y, first_class, present_only)
    G = Y.shape[0]
    nS = S.sum(1)
    u = torch.where(nS > 0, w_dice / (G * nS.clamp(min=1).to(z.dtype)), torch.zeros(G, dtype=z.dtype, device=z.device))[:, None]
    N, D = 2 * I + smooth, P + Y + smooth
    live = S & (D != 0)
    Ds = torch.where(live, D, torch.ones_like(D))
    c = torch.where(live, u * N / (Ds * Ds), torch.zeros_like(D))
    a = torch.where(live, -2 * u / Ds, torch.zeros_like(D))
    return c, a, nS


def closed_form(z, y, w_ce=1.0, w_dice=1.0, smooth=1e-5, first_class=0, present_only=True, per_image=False, ignore_index=-100):
    """d total / d z by the header's closed form, in z's dtype."""
    B, K = z.shape[:2]
    valid = _valid(y, K, ignore_index)
    n = max(int(valid.sum()), 1)
    p = torch.softmax(z, 1)
    oh = _one_hot(y, K, valid, z.dtype)
    c, a, _ = coefficients(z, y, w_dice, smooth, first_class, present_only, per_image, ignore_index)
    if not per_image:
        c, a = c.expand(B, K), a.expand(B, K)
    g = c[:, :, None, None] + oh * a[:, :, None, None]
    dot = (p * g).sum(1, keepdim=True)
    return (w_ce * (p - oh) / n + p * (g - dot)) * valid[:, None]


def pixel_scale(z, y, grad_scale=1.0, w_ce=1.0, w_dice=1.0, smooth=1e-5, first_class=0, present_only=True, per_image=False, ignore_index=-100):
    """s_px [B, H, W] = grad_scale * (w_ce / max(N, 1) + 2 max_k (|a_gk| + c_gk)) on a valid pixel of group g, 0 elsewhere; and the valid
    and bad label counts."""
    B, K = z.shape[:2]
    valid = _valid(y, K, ignore_index)
    nvalid = int(valid.sum())
    nbad = int(((y != ignore_index) & ~((y >= 0) & (y < K))).sum())
    c, a, _ = coefficients(z, y, w_dice, smooth, first_class, present_only, per_image, ignore_index)
    m = (a.abs() + c).amax(1)
    if not per_image:
        m = m.expand(B)
    s = grad_scale * (w_ce / max(nvalid, 1) + 2 * m)[:, None, None] * valid
    return s, nvalid, nbad
