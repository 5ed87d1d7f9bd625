"""bench.py -- images/sec of the UNet 256x256 bs16 train step (BASELINE.json metric) on N MI355X GPUs.

    python bench.py --gpus 1 --steps 10 --warmup 3
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
           bench.py --gpus N --steps K --warmup W
    python bench.py --gpus N ...          (no launcher: bench.py starts the N rank processes itself, see _spawn_ranks)

One step = trainer.py:172-176 on one synthetic batch that is already resident in HBM: forward -> zero_grad ->
cross-entropy -> backward -> Adam, all on libclamd's HIP kernels.  Default workload = BASELINE.json configs[1]
(UNet(21,3,64) 256x256 bs16 fp32, single task); ``--dtype bf16`` selects configs[2]'s arithmetic.  With N > 1 every
rank trains its own 16 images (weak scaling) and gradients are all-reduced over RCCL/xGMI, overlapped with backward.
Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the --steps steps and prints the headline.  ``--full`` adds everything else the line
can carry, each measured after the timed steps: per-launch kernel timing with the roofline and the sustained-MFMA
calibration, the committed PMC traffic figures, the golden-logits parity forward, the further dtypes of ``--also`` and the
CPU baseline.  ``--dump-outputs DIR`` writes what the last timed step computed (see dump_outputs) as DIR/<name>.npy.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
if int(os.environ.get('WORLD_SIZE', '1')) > 1:
    # Before the HIP runtime starts: streams are multiplexed onto this many hardware queues in creation order and a kernel
    # waits behind whatever shares its queue.  A rank has the default stream, the engine's second stream, GradSync's stream
    # and whatever RCCL creates; 8 queues keep RCCL's kernels off the two compute queues (no effect at N = 1: measured).
    os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

FLOP_PER_IMAGE_256 = 289_281_146_880          # train step, SURVEY.md §8d / BASELINE.md
PEAK = {'fp32': 157.3, 'bf16': 2500.0, 'bf16x3': 2500.0 / 3}   # dense MFMA TFLOP/s (MI355X_MICROARCH.md:42-43); bf16x3
#                                                              # issues 3 bf16 MFMAs per algorithmic multiply-add
DTYPE_NAME = {'fp32': 'f32', 'bf16': 'bf16', 'bf16x3': 'bf16x3 (hi/lo bf16 pair storage, three bf16 MFMAs per product, f32 accumulate)'}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--dtype', default='fp32', choices=['fp32', 'bf16', 'bf16x3'])
    ap.add_argument('--batch', type=int, default=16, help='images per GPU')
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--conv-dim', type=int, default=64)
    ap.add_argument('--num-classes', type=int, default=21)
    ap.add_argument('--full', action='store_true',
                    help='also measure and check what the headline does not need (kernel timing + roofline, PMC traffic, parity, '
                         '--also dtypes, CPU baseline); the --no-* switches and --also below apply to such a run')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write what the last timed step computed as DIR/<name>.npy (float32, a fixed seeded sample of large arrays)')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-kernel-timing', action='store_true', help='skip the per-launch HIP events')
    ap.add_argument('--no-parity', action='store_true', help='skip the extra golden-logits forward (profiling runs: keeps foreign launches out of the trace)')
    ap.add_argument('--also', default=None,
                    help="comma list of further dtypes measured after the main run and reported under 'also' ('' = none)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error('--steps must be at least 1')
    if args.warmup < 0:
        ap.error('--warmup must not be negative')
    return args


def _spawn_ranks(n):
    """`python bench.py --gpus N` without torch.distributed.run: start the N rank processes here -- fresh Python processes with
    RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in their environment, one per GPU -- BEFORE this process has made any GPU call
    (importing torch does not initialise HIP; the parent never does).  Rank 0 inherits stdout and prints the one JSON line.
    A rank that dies takes the others down and the exit code is non-zero."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    alive = list(procs)
    while alive:
        for p in list(alive):
            code = p.poll()
            if code is None:
                continue
            alive.remove(p)
            if code != 0 and rc == 0:
                rc = code
                for q in alive:                      # the exact children started above, by handle
                    q.terminate()
        time.sleep(0.05)
    sys.exit(rc if rc >= 0 else 1)


def golden_logits_error(model, device):
    """Parity on the driver line: rel L2 of the logits of `model`'s dtype against the reference capture of BASELINE configs[1]
    (tests/golden/unet_cd64_c21_256.npz, generated by importing the reference's models/unet.py; closed-form weights and the
    synthetic batch are regenerated here).  One extra train-mode forward of a fresh model, outside the timed region."""
    import numpy as np
    import continual_learning_amd as C
    path = os.path.join(ROOT, 'tests', 'golden', 'unet_cd64_c21_256.npz')
    if not os.path.exists(path):
        return None
    g = np.load(path)
    m = C.UNet(21, 3, 64, compute_dtype=model.compute_dtype)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items() if not k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))}
    sd = m.state_dict()
    sd.update({k: torch.from_numpy(v) for k, v in C.synth.closed_form_state(shapes, 0).items()})
    m.load_state_dict(sd, strict=True)
    m = m.to(device).train()
    x = torch.from_numpy(C.synth.images(1234, 16, 3, 256, 256)).to(device)
    with torch.no_grad():
        out = m(x)
    sub = out.reshape(-1)[::int(g['logits_flat_stride'])].double().cpu().numpy()
    ref = g['logits'].astype(np.float64)
    del m, out
    return float(np.linalg.norm(sub - ref) / np.linalg.norm(ref))


DUMP_SAMPLE = 1 << 22            # elements kept of a larger dumped array: 16 MB in float32


def _dump_sample(flat, seed):
    """A 1-D device tensor as float32 on the host: whole up to DUMP_SAMPLE elements, else the elements at a fixed seeded set of
    positions (sorted; the same for every build, given the length)."""
    import numpy as np
    n = flat.numel()
    if n > DUMP_SAMPLE:
        idx = np.unique(np.random.default_rng(seed).integers(0, n, DUMP_SAMPLE))
        flat = flat[torch.from_numpy(idx).to(flat.device)]
    return flat.detach().float().cpu().numpy()


def dump_outputs(path, model, out, loss):
    """--dump-outputs: what one train step hands its caller, right after the last timed step -- the loss, the logits, the parameters
    after Adam and their gradients (both flattened in named_parameters order and sampled at the same positions) and the BatchNorm
    running statistics -- as float32 .npy files: three samples of at most 16 MB each and two small arrays."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    params = list(model.parameters())
    arrays = {
        'loss': loss.detach().float().cpu().numpy(),
        'logits': _dump_sample(out.reshape(-1), 1),
        'params': _dump_sample(torch.cat([p.detach().reshape(-1).float() for p in params]), 2),
        'grads': _dump_sample(torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1).float() for p in params]), 2),
        'bn_running_stats': _dump_sample(torch.cat([b.reshape(-1).float() for n, b in model.named_buffers()
                                                    if n.endswith(('running_mean', 'running_var'))]), 3),
    }
    for name, a in arrays.items():
        np.save(os.path.join(path, name + '.npy'), np.asarray(a, dtype=np.float32))


def run(args, dtype, rank, world, device, timing=True, dist_on=False, dump=None):
    import continual_learning_amd as C
    from continual_learning_amd import unet as U
    torch.manual_seed(1234)
    model = C.UNet(args.num_classes, 3, args.conv_dim, compute_dtype=dtype).to(device).train()
    opt = C.FusedAdam(model.parameters(), lr=1e-4, betas=[0.5, 0.99])
    crit = C.CrossEntropyLoss()
    sync = None
    if dist_on:
        C.ddp.broadcast_parameters(model)
        sync = C.ddp.GradSync(model, opt, timing=True)
    x = torch.from_numpy(C.synth.images(1234, args.batch, 3, args.size, args.size, first_image=rank * args.batch)).to(device)
    y = torch.from_numpy(C.synth.labels(1234, args.batch, args.size, args.size, args.num_classes,
                                        first_image=rank * args.batch)).to(device)

    def step():
        out = model(x)                  # trainer.py:172
        opt.zero_grad()                 # :173
        loss = crit(out, y)             # :174
        loss.backward()                 # :175
        opt.step()                      # :176
        return out, loss

    for _ in range(args.warmup):
        out, loss = step()
    torch.cuda.synchronize()
    if sync is not None:
        sync.exposed_ms()               # drop the warm-up's wait events
        sync.launches = 0
    if dist_on:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out, loss = step()
    torch.cuda.synchronize()
    if dist_on:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    comm = None
    if dist_on:
        exposed = sync.exposed_ms() / args.steps
        t = torch.tensor([dt, exposed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t[0])
        comm = dict(C.ddp.rccl_settings(), rccl_ranks=world, collectives_per_step=sync.launches // args.steps,
                    gradient_bytes_per_step=4 * sum(p.numel() for p in model.parameters()),
                    exchange_dtype=sync.grad_dtype, buckets=sync.bucket_report(),
                    exposed_comm_ms_per_step=round(float(t[1]), 4), cu_reserve=model.tuning.cu_reserve,
                    wino_persist=model.tuning.wino_persist,
                    note='exposed = HIP-event time the compute stream waits in GradSync.wait() before Adam, max over ranks; '
                         'buckets = bytes on the wire per rank and launch offset from the start of the last backward pass (rank 0)')
    if dump and rank == 0:
        dump_outputs(dump, model, out, loss)        # before the instrumented steps below move the weights again
    del out
    # Per-launch HIP-event timing of the MFMA kernels: a SEPARATE pass of 2 steps right after the timed region
    # (an event pair around each of ~54 launches per step costs ~5 ms of dispatch bubbles per fp32 step, which would
    # distort `value`); events are recorded on the stream the kernels are launched on.
    events = []
    if timing:
        U.KERNEL_TIMING = events
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        U.KERNEL_TIMING = None
    kern = {}
    for tag, flops, e0, e1, nbytes, _unit, frac in events:
        k = kern.setdefault(tag, [0.0, 0.0, 0, 0.0, 0.0])
        k[4] += flops * frac
        k[0] += e0.elapsed_time(e1) * 1e-3
        k[1] += flops
        k[2] += 1
        k[3] += nbytes
    eng = next(iter(model._engines.values()))
    kern['_deficit_per_image'] = eng.executed_flop_deficit() / args.batch
    kern['_forms'] = sorted({('F(4x4,3x3)' if u.f44 else ('F(2x4,3x3)' if u.w24 else 'F(2x2,3x3)')) for u in eng.convs if u.wino})
    kern['_pre'] = sum(int(u.pre_f) + int(u.pre_d) for u in eng.convs)
    kern['_logits_err'] = golden_logits_error(model, device) if (rank == 0 and args.full and not args.no_parity and (args.size, args.batch, args.conv_dim, args.num_classes) == (256, 16, 64, 21)) else None
    return dt, float(loss.detach()), kern, comm


def pmc_traffic(dtype, size, batch, conv_dim):
    """HBM bytes per launch of the conv3x3 kernel from the committed rocprofv3 PMC passes of the SAME workload
    (profiles/*traffic_<dtype>*.json, written by tools/pmc_summary.py with a `workload` record; FETCH_SIZE x2 gfx950
    correction applied).  A running process cannot read PMC counters of its own kernels, so this is the profile of the
    same command; None when no profile of this exact (dtype, size, batch, conv_dim) is committed."""
    import glob
    d = None
    for f in sorted(glob.glob(os.path.join(ROOT, 'profiles', f'*traffic_{dtype}*.json')), reverse=True):
        c = json.load(open(f))
        if c.get('workload') == {'dtype': dtype, 'size': size, 'batch': batch, 'conv_dim': conv_dim}:
            d = c
            d['_file'] = os.path.basename(f)
            break
    if d is None:
        return None
    tot, n = 0.0, 0
    names = ('wino_kernel<', 'wino24_kernel<', 'wino24g_kernel<', 'wino24h_kernel<', 'wino44g_kernel<') if dtype == 'fp32' else ('igemm_ws_kernel<', 'igemm_pws_kernel<')
    for k, v in d['kernels'].items():
        if (dtype != 'fp32' and k.startswith('igemm_kernel<') and k.replace(' ', '').split(',')[1:3] == ['0', '0']) or k.startswith(names):
            tot += (v['hbm_read_bytes_per_launch'] + v['hbm_write_bytes_per_launch']) * v['launches']
            n += v['launches']
    return (round(tot / n), d['_file']) if n else None


def mfma_sustained(dtype, device):
    """TFLOP/s the matrix pipes sustain in a bare MFMA loop on pseudo-random register operands (clamd_debug_mfma_rate: the instruction
    the conv kernels of `dtype` use, one wave per SIMD, every CU), measured here and now with HIP events.  bf16 loops on real data are
    power-limited on MI355X well below the nominal 2.5 PFLOP/s; the fp32 loop is not.  A calibration beside `peak`, never a replacement."""
    import continual_learning_amd as C
    lib = C._lib.load()
    if not hasattr(lib, 'clamd_debug_mfma_rate'):      # a library built without the measurement scaffolding (include/clamd_debug.h)
        return None
    dc = {'fp32': C._lib.F32, 'bf16': C._lib.BF16, 'bf16x3': C._lib.BF16}[dtype]
    sink = torch.empty(65536, device=device)
    iters = 20000 if dtype != 'fp32' else 4000
    best = None
    for r in range(4):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        flop = lib.clamd_debug_mfma_rate(dc, iters, sink.data_ptr(), C._lib.stream_ptr())
        e1.record()
        e1.synchronize()
        if flop <= 0:
            return None
        if r:                                   # the first launch loads the kernel and lets the clock settle
            t = flop / (e0.elapsed_time(e1) * 1e-3) / 1e12
            best = t if best is None else max(best, t)
    return round(best, 1)


ELEMS_PER_IMAGE_256 = 250e6                    # activation elements a train step moves per image
N_PARAMS = 31_044_821


MFMA_KERNELS = {'fp32': ('wino_kernel<', 'wino24_kernel<', 'wino24g_kernel<', 'wino24h_kernel<', 'wino24n_kernel<', 'wino44g_kernel<', 'wino_wgrad_kernel', 'wino24_wgrad_kernel<',
                         'wino24g_wgrad_kernel', 'wino24g_wgrad_sk_kernel'),
                'bf16': ('igemm_ws_kernel<', 'igemm_pws_kernel<', 'wgrad_dma_kernel<', 'wgrad_kernel<bf16_t, 0'),
                'bf16x3': ('igemm_ws_kernel<', 'igemm_pws_kernel<', 'wgrad_kernel<split_t, 0')}


def step_traffic(dtype, size, batch, conv_dim, conv_alg_bytes_per_step=None):
    """Memory traffic of ONE train step from the committed PMC profile of the same workload, beside the algorithmic bytes of SURVEY.md 8d
    (250 M activation elements per image x e + Adam's 28 B per parameter + three reads of the weights x e; bf16x3 stores an activation as
    two bf16 halves: e = 4).  What the counters (FETCH_SIZE x 2 + WRITE_SIZE: the L2's fabric-side requests, MI355X_MICROARCH.md, HBM) measure
    is every byte that MISSES L2 -- `l2_fabric_bytes_per_step` -- whether the 256-MB Infinity Cache or HBM serves it; rocprofv3 on gfx950 exposes
    no counter behind the Infinity Cache (TCC_EA0_RDREQ_DRAM counts requests by DESTINATION, not by hit or miss).  HBM bytes are therefore
    reported as bounds: upper = the fabric bytes; lower = the fabric bytes minus the RE-READS of the 3x3 MFMA kernels (their fabric bytes beyond
    the algorithmic operand bytes of the same launches, `conv_alg_bytes_per_step`): those are operand tiles fetched again by another XCD or
    output slab within one launch, whose working set (<= 130 MB) fits the Infinity Cache.  None without a committed profile of this exact
    workload (a process cannot read the PMC counters of its own kernels)."""
    import glob
    if conv_dim != 64:
        return None
    want = {'dtype': dtype, 'size': size, 'batch': batch, 'conv_dim': conv_dim}
    for f in sorted(glob.glob(os.path.join(ROOT, 'profiles', f'*traffic_{dtype}*.json')), reverse=True):
        c = json.load(open(f))
        if c.get('workload') == want and c.get('hbm_bytes_per_step_all_kernels'):
            e = 2 if dtype == 'bf16' else 4
            alg = batch * ELEMS_PER_IMAGE_256 * (size / 256.0) ** 2 * e + N_PARAMS * 28 + 3 * N_PARAMS * e
            fab = c['hbm_bytes_per_step_all_kernels']
            out = {'l2_fabric_bytes_per_step': int(fab), 'algorithmic_bytes_per_step': int(alg), 'fabric_over_algorithmic': round(fab / alg, 3),
                   'traffic_source': 'profiles/' + os.path.basename(f),
                   'traffic_note': ('l2_fabric = FETCH_SIZE x 2 + WRITE_SIZE over all kernels of a step: bytes that miss L2, Infinity-Cache hits included (no '
                                    'counter behind the Infinity Cache is exposed); hbm_bytes_per_step_bounds = [fabric minus the 3x3 MFMA kernels\' re-reads '
                                    '(served by the Infinity Cache if it holds their <= 130-MB working sets), fabric]')}
            if conv_alg_bytes_per_step:
                conv_fab = sum(v['hbm_bytes_per_step'] for k, v in c['kernels'].items() if k.startswith(MFMA_KERNELS[dtype]))
                reread = max(0.0, conv_fab - conv_alg_bytes_per_step)
                out['mfma_kernels_fabric_bytes_per_step'] = int(conv_fab)
                out['mfma_kernels_algorithmic_bytes_per_step'] = int(conv_alg_bytes_per_step)
                out['hbm_bytes_per_step_bounds'] = [int(fab - reread), int(fab)]
                out['hbm_over_algorithmic_bounds'] = [round((fab - reread) / alg, 3), round(fab / alg, 3)]
            return out
    return None


def main():
    args = parse()
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if world == 1 and args.gpus > 1 and 'RANK' not in os.environ:
        _spawn_ranks(args.gpus)                                 # never returns
    if world != args.gpus:
        sys.exit(f'--gpus {args.gpus} does not match WORLD_SIZE={world}')
    if not torch.cuda.is_available():
        sys.exit('bench.py needs an MI355X (no CPU fallback for the product path)')
    # Rehearsal switch for 1-GPU boxes (tests/test_bench_ddp_gpu.py): CLAMD_BENCH_BACKEND=gloo lets N ranks share one
    # card (RCCL refuses two ranks on one device).  The driver's multi-GPU runs never set it.
    backend = os.environ.get('CLAMD_BENCH_BACKEND', 'nccl')
    if backend != 'nccl':
        local = local % torch.cuda.device_count()
    torch.cuda.set_device(local)
    device = torch.device('cuda', local)
    # CLAMD_BENCH_FORCE_DIST=1: rehearse the N > 1 code path (RCCL communicator with the channel cap, GradSync, comm record)
    # with ONE rank on a one-GPU box; the driver's runs never set it
    dist_on = world > 1 or bool(os.environ.get('CLAMD_BENCH_FORCE_DIST'))
    if dist_on:
        if backend == 'nccl':
            import continual_learning_amd as C
            C.ddp.init_rccl(device)                             # "nccl" IS RCCL on ROCm; caps the channel count
        else:
            dist.init_process_group(backend)

    dt, loss, kern, comm = run(args, args.dtype, rank, world, device, timing=args.full and not args.no_kernel_timing, dist_on=dist_on,
                               dump=args.dump_outputs)
    images = args.batch * world * args.steps
    value = images / dt
    scale = (args.size / 256.0) ** 2 * (args.conv_dim / 64.0) ** 2
    flop_img = FLOP_PER_IMAGE_256 * scale

    out = {
        'metric': 'images/sec UNET 256x256 bs16 train step' if (args.size, args.batch) == (256, 16) else
                  f'images/sec UNET {args.size}x{args.size} bs{args.batch} train step', 'value': round(value, 2), 'unit': 'images/sec',
        'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': round(dt / args.steps * 1e3, 3),
        'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': DTYPE_NAME[args.dtype],
        'data': 'synthetic (splitmix64 images U(-1,1), blocky 21-class labels), random-init weights',
        'config': {'workload': f'UNet({args.num_classes},3,{args.conv_dim}) {args.size}x{args.size} bs{args.batch}/GPU '
                               f'{args.dtype} train step (fwd + CE + bwd + Adam), BASELINE.json configs['
                               f'{4 if (args.size, args.batch) == (512, 32) else 2 if args.dtype == "bf16" else 1}]',
                   'global_batch': args.batch * world, 'parallelism': f'dp{world}', 'final_loss': round(loss, 5)},
    }
    # whole step against the MFMA peak: EXECUTED multiply-adds (the fp32 path runs every 3x3 convolution but enc1.0 as
    # Winograd F(2x2,3x3): 16/36 of the algorithmic FLOPs); the algorithmic rate and the reduction are separate fields
    deficit = kern.pop('_deficit_per_image', 0.0)
    forms = kern.pop('_forms', [])
    npre = kern.pop('_pre', 0)
    lerr = kern.pop('_logits_err', None)
    if lerr is not None:
        out['logits_rel_l2_vs_golden'] = float(f'{lerr:.3e}')
        out['logits_parity_note'] = ('rel L2 of the train-mode logits against the reference capture of BASELINE configs[1] '
                                     '(tests/golden/unet_cd64_c21_256.npz); north_star bound 1e-3')
    wino = deficit > 0
    exec_img = flop_img - deficit
    out['step_algorithmic_tflops'] = round(value * flop_img / 1e12, 2)
    out['step_executed_tflops'] = round(value * exec_img / 1e12, 2)
    out['step_frac_of_mfma_peak'] = round(value * exec_img / 1e12 / (PEAK[args.dtype] * world), 4)
    out['algorithmic_speedup'] = round(flop_img / exec_img, 4)
    if comm is not None:
        out['comm'] = comm
    if args.full:
        conv_alg = (kern.get('igemm_conv3x3', (0, 0, 0, 0, 0))[3] + kern.get('wgrad_conv3x3', (0, 0, 0, 0, 0))[3]) / 2 if kern else None
        out.update(step_traffic(args.dtype, args.size, args.batch, args.conv_dim, conv_alg) or
                   {'l2_fabric_bytes_per_step': None, 'algorithmic_bytes_per_step': None, 'fabric_over_algorithmic': None})
    if kern:
        # dominant kernel = the 3x3 implicit-GEMM (forward + data-gradient launches share one kernel template)
        sec, flops, n, nbytes, xflops = kern.get('igemm_conv3x3', (0, 0, 0, 0, 0))
        if sec > 0:
            alg = flops / sec / 1e12
            ach = xflops / sec / 1e12                          # FLOP/s the MFMA pipe executes
            tr = pmc_traffic(args.dtype, args.size, args.batch, args.conv_dim)
            out['roofline'] = {'bound': 'mfma', 'achieved': round(ach, 2), 'peak': PEAK[args.dtype], 'unit': 'TFLOP/s',
                               'frac': round(ach / PEAK[args.dtype], 4), 'traffic': tr[0] if tr else None,
                               'traffic_source': ('profiles/' + tr[1]) if tr else None,
                               'kernel': (f'conv3x3 fwd + dgrad launches: clamd::wino44g_kernel / clamd::wino24g_kernel (pre-transformed input, {npre} launches per step) / '
                                          f'clamd::wino24_kernel / clamd::wino_kernel (Winograd {" / ".join(forms)} on v_mfma_f32_32x32x2_f32)' if wino else
                                          'conv3x3 implicit GEMM, fwd + dgrad launches: clamd::igemm_pws_kernel<T,TW> (persistent, <= 256 input '
                                          'channels) and clamd::igemm_ws_kernel<T,TW,MT> (> 256 input channels)'),
                               'launches': n, 'avg_launch_ms': round(sec / n * 1e3, 4),
                               'algorithmic_bytes_per_launch': round(nbytes / n),
                               'ms_per_step': round(sec / 2 * 1e3, 3),
                               'timing': ('HIP events around every launch, 2 instrumented steps after the timed region; those two steps '
                                          'keep every kernel on one stream (unet.WGRAD_STREAM overlap off), so a launch is timed alone')}
            sus = mfma_sustained(args.dtype, device)
            if sus:
                out['roofline']['sustained_mfma_tflops_measured'] = sus
                out['roofline']['frac_of_sustained'] = round(ach / sus, 4)
                out['roofline']['sustained_note'] = ('bare loop of the same MFMA instruction on pseudo-random register operands, every CU, timed in this process '
                                                     '(clamd_debug_mfma_rate): what the pipes sustain under the power limit; `peak` stays the nominal figure')
            xsec, _, xn, xbytes, _ = kern.get('wino_transform', (0, 0, 0, 0, 0))
            if xn:
                # the HBM-bound input transforms of the pre-transformed launches are NOT inside `achieved`: their own line
                out['roofline']['input_transforms'] = {'bound': 'hbm', 'launches': xn, 'ms_per_step': round(xsec / 2 * 1e3, 3),
                                                       'achieved': round(xbytes / xsec / 1e9, 1), 'peak': 8000.0, 'unit': 'GB/s',
                                                       'frac': round(xbytes / xsec / 8e12, 4),
                                                       'kernel': 'clamd::wino24_xform_kernel (B^T d B once per tensor: reads the activation, writes 3x its size)'}
                out['roofline']['frac_including_transforms'] = round(xflops / (sec + xsec) / 1e12 / PEAK[args.dtype], 4)
            if wino:
                # `achieved` / `frac` = EXECUTED multiply-adds (MFMA pipe utilisation); the algorithmic (direct-convolution)
                # rate is reported beside it
                out['roofline']['algorithmic_tflops'] = round(alg, 2)
                out['roofline']['algorithmic_speedup'] = round(flops / xflops, 4)
                out['roofline']['note'] = ('Winograd: F(2x4,3x3) executes 24 MFMA multiply-adds per 2x4 output tile and channel pair instead of '
                                           '72 (F(2x2,3x3): 16 instead of 36); achieved/frac count the EXECUTED multiply-adds, '
                                           'algorithmic_tflops the direct-convolution ones')
        # the HBM-bound kernel families of the step ("report HBM fraction separately for the HBM-bound kernels"): per family the
        # launches, their time (each launch alone, HIP events, single stream) and their ALGORITHMIC bytes -- every tensor a family has to
        # read or write, once; a second pass over the same tensor (the BatchNorm-backward reduce in front of its apply pass, a bias-gradient
        # channel sum beside its weight gradient) is charged 0 bytes, so `frac` falls with every pass fusion has not removed yet
        fam = {k[4:]: v for k, v in kern.items() if isinstance(k, str) and k.startswith('hbm:')}
        if fam:
            label = {'bn_fwd': 'A5/A6 BatchNorm apply (+ max-pool, concat placement) and stand-alone pooling passes', 'bn_bwd': 'A5/A6 BatchNorm / ReLU / pool backward: reduce + apply passes',
                     'convT': 'A7 ConvTranspose2d forward, data gradient, weight + bias gradient', 'head': 'A9 1x1 head forward, data gradient, weight + bias gradient',
                     'loss': 'A10 cross-entropy forward + backward', 'adam': 'A13 Adam', 'enc1.0': 'enc1.0: im2col + pointwise convolution + its weight gradient'}
            hk = {}
            for k, (fsec, _, fn, fbytes, _) in fam.items():
                hk[k] = {'what': label.get(k, k), 'launches_per_step': fn // 2, 'ms_per_step': round(fsec / 2 * 1e3, 4),
                         'algorithmic_bytes_per_step': int(fbytes // 2), 'achieved': round(fbytes / fsec / 1e9, 1) if fsec > 0 else None,
                         'peak': 8000.0, 'unit': 'GB/s', 'frac': round(fbytes / fsec / 8e12, 4) if fsec > 0 else None}
            out['hbm_kernels'] = hk
            out['hbm_kernels_note'] = ('algorithmic bytes / time of every launch of the family timed alone (HIP events, 2 instrumented single-stream steps); '
                                       'peak = 8 TB/s spec (a float4 copy measures 6.29 TB/s on this part)')
        sec, flops, n, _, xflops = kern.get('wgrad_conv3x3', (0, 0, 0, 0, 0))
        if sec > 0:
            alg = flops / sec / 1e12
            ach = xflops / sec / 1e12
            out['roofline_wgrad'] = {'bound': 'mfma', 'achieved': round(ach, 2), 'peak': PEAK[args.dtype],
                                     'unit': 'TFLOP/s', 'frac': round(ach / PEAK[args.dtype], 4), 'launches': n,
                                     'avg_launch_ms': round(sec / n * 1e3, 4), 'ms_per_step': round(sec / 2 * 1e3, 3),
                                     'note': 'wgrad kernel + its split-K reduce kernel (pre-transformed launches: + the gradient-side transform)'}
            if wino:
                out['roofline_wgrad']['algorithmic_tflops'] = round(alg, 2)
                out['roofline_wgrad']['algorithmic_speedup'] = round(flops / xflops, 4)
    # further dtypes (--full only): by default on the single-GPU run only (the N-GPU scaling runs measure the headline dtype and nothing else)
    also = (args.also if args.also is not None else ('bf16x3,bf16' if not dist_on else '')) if args.full else ''
    for other in [d for d in also.split(',') if d and d != args.dtype]:
        dt2, loss2, k2, _ = run(args, other, rank, world, device, timing=not args.no_kernel_timing)
        v2 = images / dt2
        o = {'dtype': DTYPE_NAME[other], 'value': round(v2, 2), 'ms_per_step': round(dt2 / args.steps * 1e3, 3),
             'step_frac_of_mfma_peak': round(v2 * flop_img / 1e12 / (PEAK[other] * world), 4),
             'final_loss': round(loss2, 5)}
        k2alg = (k2.get('igemm_conv3x3', (0, 0, 0, 0, 0))[3] + k2.get('wgrad_conv3x3', (0, 0, 0, 0, 0))[3]) / 2 if k2 else None
        o.update(step_traffic(other, args.size, args.batch, args.conv_dim, k2alg) or {})
        k2.pop('_deficit_per_image', None); k2.pop('_forms', None); k2.pop('_pre', None)
        le2 = k2.pop('_logits_err', None)
        if le2 is not None:
            o['logits_rel_l2_vs_golden'] = float(f'{le2:.3e}')
        sec, flops, n, _, _x = k2.get('igemm_conv3x3', (0, 0, 0, 0, 0))
        if sec > 0:
            o['conv3x3_igemm_tflops'] = round(flops / sec / 1e12, 1)
            o['conv3x3_igemm_frac_of_peak'] = round(flops / sec / 1e12 / PEAK[other], 4)
            sus = mfma_sustained(other, device)
            if sus:
                o['mfma_sustained_tflops_measured'] = sus      # bare bf16 MFMA loop on random operands, here and now: the power-limited ceiling
                o['conv3x3_igemm_frac_of_sustained'] = round(flops * (3 if other == 'bf16x3' else 1) / sec / 1e12 / sus, 4)
        sec, flops, n, _, _x = k2.get('wgrad_conv3x3', (0, 0, 0, 0, 0))
        if sec > 0:
            o['conv3x3_wgrad_tflops'] = round(flops / sec / 1e12, 1)
        out.setdefault('also', []).append(o)
    if rank == 0 and not dist_on and args.full and not args.no_cpu_baseline:
        from oracle import torch_cpu as TC                       # the checker timed as the reported CPU baseline
        xb = x_cpu = None
        import continual_learning_amd as C
        xb = torch.from_numpy(C.synth.images(1234, args.batch, 3, args.size, args.size))
        yb = torch.from_numpy(C.synth.labels(1234, args.batch, args.size, args.size, args.num_classes))
        # 1 warm-up + best of 3 steps on the BASELINE workload (~25 s of CPU work on 16 cores); larger
        # workloads (config 5 is 8x the work) get one timed step so the run stays bounded
        cb = TC.time_cpu_baseline(batch=args.batch, size=args.size, num_classes=args.num_classes, conv_dim=args.conv_dim,
                                  steps=3 if args.size * args.size * args.batch <= 256 * 256 * 16 else 1, warmup=1,
                                  images=xb, labels=yb)
        out['cpu_baseline'] = {'value': round(cb['value'], 3), 'unit': 'images/sec', 'cores': cb['cores'],
                               'kind': 'port', 'sample': cb['sample']}
    if rank == 0:
        print(json.dumps(out), flush=True)
    if dist_on:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
