"""The reference's building blocks as stand-alone custom ops (models/unet.py:8-38: DownBlock = MaxPool, Conv-ReLU-BN x 2; UpBlock =
Conv-ReLU-BN x 2, ConvTranspose; :50-55 / :66-72 the plain first and last sequences).

``UNet.forward`` runs the whole network as ONE autograd Function over a planned engine (unet.py) -- that is the measured path.  A child
called on its own (``model.enc2(x)``, ``model.dec1.block(x)``: feature probes, unit tests of one block) runs here: one
``torch.autograd.Function`` per block over the same libclamd kernels (generic direct convolutions, BatchNorm statistics rows, fused
BatchNorm passes, stand-alone max-pool), NCHW fp32 in and out like every visible tensor of this package, buffers allocated per call.
No stock-torch operator is involved and there is no CPU path.
"""
import torch

from . import _lib, bnops, convops, syncbn
from ._lib import call, ptr
from .ops import PackTable, TORCH_DT, cpad, from_nhwc, to_nhwc
from .plan import ALGOS

DIRECT = ALGOS['igemm']      # the generic direct kernels run every 3x3 convolution here, whatever the engine would plan

def _stream():
    return _lib.stream_ptr()


class _BlockFn(torch.autograd.Function):
    """forward(x, plan, *params): plan = (ops, dcode, buffers, group); ops = [('pool',), ('crb', k, training, sync), ..., ('convT',) | ('head',)]
    (`training`: that BatchNorm module's own mode -- batch statistics, or its running statistics and no update; `sync`: a train-mode
    nn.SyncBatchNorm whose sums are all-reduced over `group`, syncbn.py);
    params = (conv.weight, conv.bias, bn.weight, bn.bias) per 'crb' in order, then (weight, bias) of the tail."""

    @staticmethod
    def forward(ctx, x, plan, *params):
        ops, dcode, buffers, group = plan
        T = TORCH_DT[dcode]
        dev = x.device
        s = _stream()
        B, C, H, W = x.shape
        cur = to_nhwc(x.contiguous().float(), dcode)          # [B,H,W,cpad(C)]
        saved, pi = [], 0
        for op in ops:
            if op[0] == 'pool':
                if (H | W) & 1:
                    raise ValueError('MaxPool2d(2,2) block: H and W must be even')
                out = torch.empty(B, H // 2, W // 2, cur.shape[-1], dtype=T, device=dev)
                convops.maxpool(call, ptr(cur), cur.shape[-1], None, ptr(out), out.shape[-1], B, H, W, cur.shape[-1], dcode, s)
                saved.append(('pool', cur, H, W))
                cur, H, W = out, H // 2, W // 2
            elif op[0] == 'crb':
                w, b, gamma, beta = params[pi:pi + 4]
                rm, rv, nbt = buffers[op[1]]
                training, sync = op[2], op[3]
                pi += 4
                cout, cin = w.shape[0], w.shape[1]
                cin_p, cout_p = cur.shape[-1], cpad(cout)
                wf = torch.zeros(9 * cout_p * cin_p, dtype=T, device=dev)
                wd = torch.zeros(9 * cin_p * cout_p, dtype=T, device=dev)
                bias_p = torch.zeros(cout_p, dtype=torch.float32, device=dev)
                tab = PackTable(dcode)
                tab.conv3x3(w.detach(), wf, wd, [(cin, cin_p)], cout)
                tab.vector(b.detach(), bias_p, cout)
                tab.finalize(dev).run(dcode, s)
                rows = _lib.stat_rows(_lib.OP_CONV3X3, B, H, W, cin_p, cout_p, dcode)
                y = torch.empty(B, H, W, cout_p, dtype=T, device=dev)
                stats = torch.empty(rows, 2, cout_p, dtype=torch.float32, device=dev) if training else None
                convops.conv3x3(call, DIRECT, ptr(cur), cin_p, None, ptr(wf), ptr(bias_p), ptr(y), cout_p, ptr(stats), rows, None, B, H, W,
                                cin_p, cout_p, 1, dcode, None, s)
                vec = torch.zeros(7, cout_p, dtype=torch.float32, device=dev)       # scale, shift, mean, istd, k0, k1, k2
                # sync: the statistics of the global batch (as in the UNet engine)
                red = torch.empty(2 * cout_p + 1, dtype=torch.float64, device=dev) if sync else None
                bnops.fwd_finalize(stats, rows, gamma.detach(), beta.detach(), rm, rv, nbt, vec, cout_p, cout, float(B * H * W), training or sync, s, red, group)
                out = torch.empty_like(y)
                convops.bn_apply(call, ptr(y), cout_p, ptr(vec[0]), ptr(vec[1]), ptr(out), cout_p, None, 0, B, H, W, cout_p, dcode, s)
                saved.append(('crb', cur, y, vec, wd, gamma.detach(), training, sync, (cin, cin_p, cout, cout_p, H, W)))
                cur = out
            elif op[0] == 'convT':
                w, b = params[pi:pi + 2]
                pi += 2
                cin, cout = w.shape[0], w.shape[1]
                cin_p, cout_p = cur.shape[-1], cpad(cout)
                wf = torch.zeros(4 * cout_p * cin_p, dtype=T, device=dev)
                wd = torch.zeros(cin_p * 4 * cout_p, dtype=T, device=dev)
                bias_p = torch.zeros(cout_p, dtype=torch.float32, device=dev)
                tab = PackTable(dcode)
                tab.convT(w.detach(), wf, wd, cin, cout)
                tab.vector(b.detach(), bias_p, cout)
                tab.finalize(dev).run(dcode, s)
                out = torch.empty(B, 2 * H, 2 * W, cout_p, dtype=T, device=dev)
                convops.convT_fwd(call, ptr(cur), cin_p, ptr(wf), ptr(bias_p), ptr(out), cout_p, B, H, W, cin_p, cout_p, dcode, s)
                saved.append(('convT', cur, wd, (cin, cin_p, cout, cout_p, H, W)))
                cur, H, W = out, 2 * H, 2 * W
            else:                                       # 'head': 1x1 convolution, fp32 NCHW logits straight from the epilogue
                w, b = params[pi:pi + 2]
                pi += 2
                k, cin = w.shape[0], w.shape[1]
                cin_p, kp = cur.shape[-1], cpad(k)
                wf = torch.zeros(kp * cin_p, dtype=T, device=dev)
                wd = torch.zeros(cin_p * kp, dtype=T, device=dev)
                bias_p = torch.zeros(kp, dtype=torch.float32, device=dev)
                tab = PackTable(dcode)
                tab.head(w.detach(), wf, wd, cin, k)
                tab.vector(b.detach(), bias_p, k)
                tab.finalize(dev).run(dcode, s)
                logits = torch.empty(B, k, H, W, dtype=torch.float32, device=dev)
                convops.head_fwd(call, ptr(cur), cin_p, ptr(wf), ptr(bias_p), ptr(logits), None, B, H, W, cin_p, kp, k, dcode, s)
                saved.append(('head', cur, wd, (cin, cin_p, k, kp, H, W)))
                cur = None
        ctx.saved_ops, ctx.dcode, ctx.B, ctx.cin0, ctx.group = saved, dcode, B, C, group
        if cur is None:
            return logits
        last = ops[-1]
        cout = params[-2].shape[1] if last[0] == 'convT' else params[-4].shape[0]
        return from_nhwc(cur, cout, dcode)

    @staticmethod
    def backward(ctx, gout):
        dcode, B = ctx.dcode, ctx.B
        lib = _lib.load()
        T = TORCH_DT[dcode]
        dev = gout.device
        s = _stream()
        grads = []
        g = None                                                        # NHWC gradient w.r.t. the current op's output
        gout = gout.contiguous().float()
        for rec in reversed(ctx.saved_ops):
            kind = rec[0]
            if kind in ('head', 'convT'):      # the tail: data gradient, then d weight in the parameter's own layout and d bias
                _, x, wd, (cin, cin_p, cout, cout_p, H, W) = rec
                gy = to_nhwc(gout, dcode, cp=cout_p) if g is None else g
                gx = torch.empty(B, H, W, cin_p, dtype=T, device=dev)
                convops.tail_dgrad(call, kind, ptr(gy), cout_p, ptr(wd), ptr(gx), cin_p, None, B, H, W, cin_p, cout_p, dcode, s)
                wsb = convops.tail_workspace_bytes(lib, kind, B, H, W, cin_p, cout_p, dcode)
                ws = torch.empty(convops.workspace_floats(wsb), dtype=torch.float32, device=dev)
                dw = torch.empty((cout, cin, 1, 1) if kind == 'head' else (cin, cout, 2, 2), dtype=torch.float32, device=dev)
                db = torch.empty(cout, dtype=torch.float32, device=dev)
                convops.tail_wgrad(call, kind, ptr(x), cin_p, ptr(gy), cout_p, ptr(ws), wsb, ptr(dw), B, H, W, cin, cin_p, cout, cout_p, dcode, None, s)
                convops.tail_bias_grad(call, kind, ptr(gy), cout_p, ptr(db), B, H, W, cout, cout_p, dcode, ptr(ws), wsb, None, s)
                grads = [dw, db] + grads
                g = gx
            elif kind == 'crb':
                _, x, y, vec, wd, gamma, training, sync, (cin, cin_p, cout, cout_p, H, W) = rec
                ga = to_nhwc(gout, dcode, cp=cout_p) if g is None else g
                dgamma, dbeta, dbias = (torch.empty(cout, dtype=torch.float32, device=dev) for _ in range(3))
                gz = torch.empty(B, H, W, cout_p, dtype=T, device=dev)
                if training:
                    rows = _lib.stat_rows(_lib.OP_BN_BWD_REDUCE, B, H, W, 0, cout_p, dcode)
                    sums = torch.empty(rows, lib.clamd_bn_bwd_nsums(), cout_p, dtype=torch.float32, device=dev)
                    convops.bn_bwd_reduce(call, ptr(ga), cout_p, None, 0, ptr(y), cout_p, ptr(vec[0]), ptr(vec[1]), ptr(sums), rows,
                                          B, H, W, cout_p, dcode, None, s)
                    scratch = None
                    if sync:   # g_z from the sums of the global batch; d gamma, d beta, d conv-bias from this rank's own (as torch)
                        red = torch.empty(2 * cout_p + 1, dtype=torch.float64, device=dev)
                        scratch = (torch.empty(lib.clamd_bn_bwd_nsums(), cout_p, dtype=torch.float64, device=dev), red)
                    bnops.bwd_finalize(sums, rows, lib.clamd_bn_bwd_nsums(), gamma, vec, ptr(dgamma), ptr(dbeta), ptr(dbias), cout_p, cout,
                                       float(B * H * W), s, scratch, ctx.group)
                    convops.bn_bwd_apply(call, ptr(ga), cout_p, None, 0, ptr(y), cout_p, ptr(vec[0]), ptr(vec[1]), ptr(vec[4]), ptr(gz), cout_p,
                                         B, H, W, cout_p, dcode, s)
                else:      # running statistics: one pass writes g_z and the rows of the parameter gradients
                    rows = lib.clamd_bn_bwd_eval_rows(B, H, W, cout_p, 0)
                    if rows <= 0:
                        _lib.check(rows, 'clamd_bn_bwd_eval_rows')
                    er = torch.empty(rows, 3, cout_p, dtype=torch.float32, device=dev)
                    convops.bn_bwd_eval(call, ptr(ga), cout_p, None, 0, ptr(y), cout_p, ptr(vec[0]), ptr(vec[1]), ptr(gz), cout_p, ptr(er), rows,
                                        B, H, W, cout_p, cout, dcode, s)
                    bnops.bwd_eval_finalize(er, rows, 3, vec, False, ptr(dgamma), ptr(dbeta), ptr(dbias), cout_p, cout, s)
                gx = torch.empty(B, H, W, cin_p, dtype=T, device=dev)
                convops.conv3x3(call, DIRECT, ptr(gz), cout_p, None, ptr(wd), None, ptr(gx), cin_p, None, 0, None, B, H, W, cout_p, cin_p, 0, dcode, None, s)
                wsb = DIRECT.wg_ws(lib, B, H, W, cout_p, cin_p, dcode)
                ws = torch.empty(convops.workspace_floats(wsb), dtype=torch.float32, device=dev)
                dw = torch.empty(cout, cin, 3, 3, dtype=torch.float32, device=dev)
                convops.wgrad3x3(call, DIRECT, ptr(gz), cout_p, ptr(x), cin_p, None, None, ptr(ws), wsb, ptr(dw), B, H, W, cout_p, cin_p, cout, cin,
                                 cin, cin_p, dcode, None, s)
                grads = [dw, dbias, dgamma, dbeta] + grads
                g = gx
            else:                                                       # 'pool'
                _, x, H, W = rec
                cp = x.shape[-1]
                gp = to_nhwc(gout, dcode, cp=cp) if g is None else g
                gx = torch.empty(B, H, W, cp, dtype=T, device=dev)
                convops.maxpool_bwd(call, ptr(x), cp, None, ptr(gp), cp, ptr(gx), cp, B, H, W, cp, dcode, s)
                g = gx
        gin = from_nhwc(g, ctx.cin0, dcode) if ctx.needs_input_grad[0] else None
        return (gin, None) + tuple(grads)


def run_block(seq, st, dcode, x):
    """Runs the layers of one stage of the UNet table (unet.stage_table) on x [B,C,H,W] (fp32, GPU)."""
    if not x.is_cuda:
        raise RuntimeError('continual-learning_amd blocks run only on GPU tensors: there is no CPU fallback')
    if x.dim() != 4:
        raise ValueError(f'expected [B,C,H,W], got {tuple(x.shape)}')
    ops, params, buffers = [], [], []
    if st['pool']:
        ops.append(('pool',))
    group, sync = syncbn.resolve([(str(bi), seq[bi]) for _, bi, _, _ in st['convs']])
    for (ci, bi, cin, cout), sy in zip(st['convs'], sync):
        conv, bn = seq[ci], seq[bi]
        ops.append(('crb', len(buffers), bool(bn.training), sy))
        params += [conv.weight, conv.bias, bn.weight, bn.bias]
        buffers.append((bn.running_mean, bn.running_var, bn.num_batches_tracked))
    if st['tail'] is not None:
        kind, ti, _, _ = st['tail']
        ops.append((kind,))
        params += [seq[ti].weight, seq[ti].bias]
    if x.shape[1] != st['convs'][0][2]:
        raise ValueError(f'expected {st["convs"][0][2]} input channels, got {x.shape[1]}')
    return _BlockFn.apply(x, (ops, dcode, buffers, group), *params)
