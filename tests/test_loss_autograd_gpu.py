"""GPU: the autograd contract every criterion of loss.py keeps, whichever entry point it launches.
  (a) d loss / d logits is, bit for bit, the d logits of a direct C-ABI call on the same inputs with grad_scale 1; an upstream gradient of
      0.5 gives that tensor times 0.5 (exact in fp32);
  (b) old logits, image weights and class weights that ask for a gradient receive none, and nothing is raised;
  (c) `parts` and `bad_labels` are left on the criterion (here: the direct call's own three numbers and counter).
B = 2, K = 5 at 8 x 12 (the four-pixel kernels) and at 7 x 9 (the one-pixel kernels and ce_kernel).  The kernels' values are held per element by
test_loss_grid_gpu.py, test_wce_grid_gpu.py and test_dice_gpu.py; this file holds what lies between them and autograd."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
B, K, C_OLD, IGN = 2, 5, 3, -100
W5 = [0.5, 2.0, 0.0, 1.25, 1.0]


@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    C._lib.load()
    return C


@pytest.fixture(scope='module', params=[(8, 12), (7, 9)], ids=['8x12', '7x9'])
def case(request):
    H, W = request.param
    g = torch.Generator().manual_seed(1000 * H + W)
    z = 3.0 * torch.randn(B, K, H, W, generator=g)
    y = torch.randint(0, K, (B, H, W), generator=g)
    y[0, 0, :3] = IGN
    y[1, 2, 1] = K + 2                          # neither a class nor ignore_index: counted, left out of the mean
    y[1, 3, 4] = -1
    old = 2.0 * torch.randn(B, C_OLD, H, W, generator=g)
    nu = torch.tensor([0.75, 1.5])
    return dict(H=H, W=W, z=z.to(DEV), y=y.to(DEV), old=old.to(DEV), nu=nu.to(DEV), w=torch.tensor(W5, device=DEV))


class _Direct:
    """The library called as loss.py calls it, without the NHWC copy and with grad_scale 1 -> (d logits, out3, bad label counter)."""

    def __init__(self, C, cs):
        self.L, self.lib, self.cs = C._lib, C._lib.load(), cs
        self.shape = (B, K, cs['H'], cs['W'], IGN)
        self.dl = torch.empty_like(cs['z'])
        self.out3 = torch.empty(3, dtype=torch.float32, device=DEV)

    def run(self, entry, lead=(), tail=(), count=True, wsb=None, nhwc=True):
        L, cs = self.L, self.cs
        wsb = self.lib.clamd_ce_workspace_bytes() if wsb is None else wsb
        ws = torch.empty(wsb // 4, dtype=torch.float32, device=DEV)
        s = L.stream_ptr()
        if count:
            L.call('clamd_ce_count', L.ptr(cs['y']), B, K, cs['H'], cs['W'], IGN, L.ptr(ws), wsb, s)
        L.call(entry, L.ptr(cs['z']), L.ptr(cs['y']), *lead, L.ptr(self.dl), *((None, 0, 0) if nhwc else ()), L.ptr(self.out3), L.ptr(ws), wsb,
               *self.shape, *tail, 1.0, s)
        torch.cuda.synchronize()
        off = self.lib.clamd_ce_bad_label_count_offset() // 4
        return self.dl, self.out3, int(ws[off:off + 1].view(torch.int32))

    def any_size(self, old=None, c_old=0, temperature=1.0, lam=0.0):
        kold = 0 if old is None else old.shape[1]
        return self.run('clamd_ce_fwd_bwd', (self.L.ptr(old), kold, c_old, float(temperature), float(lam)), count=False, nhwc=False)

    def plain(self):
        return self.run('clamd_ce_fwd_bwd_counted') if self.cs['H'] * self.cs['W'] % 4 == 0 else self.any_size()

    def weighted(self):
        return self.run('clamd_ce_fwd_bwd_weighted', (self.L.ptr(self.cs['nu']),))

    def classes(self, w, eps, gamma, nu=None):
        return self.run('clamd_ce_class_fwd_bwd', (self.L.ptr(w), self.L.ptr(nu)), (float(eps), float(gamma)), count=False,
                        wsb=self.lib.clamd_ce_class_workspace_bytes())

    def unbiased(self, old, lam):
        kold = 0 if old is None else old.shape[1]
        return self.run('clamd_ce_unbiased_fwd_bwd', (self.L.ptr(old), kold, C_OLD, float(lam)))

    def dice(self, per_image):
        wsb = self.lib.clamd_ce_dice_workspace_bytes(B, K, self.cs['H'], self.cs['W'], int(per_image))
        return self.run('clamd_ce_dice_fwd_bwd', (), (1.0, 0.5, 1e-5, 1, 1, int(per_image)), count=False, wsb=wsb)


# name -> (criterion(C, leaves), the forward's further arguments out of `leaves`, the direct call); `leaves`: the case's old logits, image
# weights and class weights as leaf tensors that ask for a gradient
ONES = torch.ones(K)
CRITERIA = {
    'plain': (lambda C, v: C.CrossEntropyLoss(), (), lambda d, v: d.plain()),
    'plain_image_weight': (lambda C, v: C.CrossEntropyLoss(), ('nu',), lambda d, v: d.weighted()),
    'class_weights': (lambda C, v: C.CrossEntropyLoss(weight=v['w']), (), lambda d, v: d.classes(v['w'].detach(), 0.0, 0.0)),
    'smoothing': (lambda C, v: C.CrossEntropyLoss(label_smoothing=0.1), (), lambda d, v: d.classes(ONES.to(DEV), 0.1, 0.0)),
    'focal': (lambda C, v: C.CrossEntropyLoss(focal_gamma=2.0), (), lambda d, v: d.classes(ONES.to(DEV), 0.0, 2.0)),
    'class_weights_image_weight': (lambda C, v: C.CrossEntropyLoss(weight=v['w']), ('nu',),
                                   lambda d, v: d.classes(v['w'].detach(), 0.0, 0.0, v['nu'].detach())),
    'distillation': (lambda C, v: C.DistillationCrossEntropy(C_OLD, temperature=2.0, lam=0.5), ('old',),
                     lambda d, v: d.any_size(v['old'].detach(), C_OLD, 2.0, 0.5)),
    'unbiased_old': (lambda C, v: C.UnbiasedDistillationCrossEntropy(C_OLD, lam=10.0), ('old',), lambda d, v: d.unbiased(v['old'].detach(), 10.0)),
    'unbiased': (lambda C, v: C.UnbiasedDistillationCrossEntropy(C_OLD, lam=10.0), (), lambda d, v: d.unbiased(None, 10.0)),
    'dice': (lambda C, v: C.DiceCrossEntropyLoss(1.0, 0.5, include_background=False, per_image=True), (), lambda d, v: d.dice(True)),
}


@pytest.mark.parametrize('name', list(CRITERIA))
def test_gradient_is_the_kernels_d_logits(C, case, name):
    make, extra, direct = CRITERIA[name]
    want_dl, want_out3, want_bad = (t.clone() if torch.is_tensor(t) else t for t in direct(_Direct(C, case), case))
    assert want_bad == 2
    for up in (1.0, 0.5):
        leaves = {k: case[k].clone().requires_grad_() for k in ('old', 'nu', 'w')}
        crit = make(C, leaves)
        z = case['z'].clone().requires_grad_()
        args = [leaves[k] for k in extra]
        loss = crit(z, case['y'], *args)
        got = torch.autograd.grad(loss if up == 1.0 else up * loss, [z] + args, allow_unused=True)                     # (b): nothing raised ...
        torch.cuda.synchronize()
        assert all(g is None for g in got[1:]) and all(t.grad is None for t in leaves.values())      # ... and nothing received
        assert torch.equal(got[0], want_dl * torch.tensor(up, dtype=torch.float32, device=DEV))      # (a)
        assert float(loss.detach()) == float(want_out3[0])
        assert torch.equal(crit.parts, want_out3)                                                 # (c)
        assert crit.bad_labels.dtype == torch.int32 and crit.bad_labels.shape == (1,) and int(crit.bad_labels) == want_bad
